/*
 * pdplqr.h -- C ABI of the MI355X-native PDP-LQR solver (libpdplqr.so).
 *
 * This is the drop-in boundary for the reference's solver protocol
 *     update_problem_data -> backward -> forward
 * of Luyao787/PDP-LQR (header-only C++/Eigen/OpenMP).  Every entry point below
 * names the reference interface it replaces (file:line, relative to the
 * reference root).  The C++ facade headers under include/clqr/ (same class
 * names as the reference) and the Python host mirror (pdp-lqr_amd/pdplqr) are
 * the only callers.  No torch or HIP types cross this boundary: plain
 * pointers, sizes and int status codes (0 = ok, < 0 = error; no exceptions).
 *
 * Data layout at the boundary ("reference layout"): every per-stage block is
 * Eigen column-major, blocks are stage-major, problems are batch-major.  With
 * n = nx, m = nu, s = n + m, nc_k = constraint rows of stage k:
 *   E   [batch][N][n*s]            E_k = [B A]          (lqr_model.hpp:14)
 *   c   [batch][N][n]                                   (lqr_model.hpp:15)
 *   H   [batch][N*s*s + n*n]       H_k = [R S; S^T Q], then Q_N (lqr_model.hpp:18,33)
 *   h   [batch][N*s + n]           h_k = [r; q], then q_N
 *   D   [batch][sum_k nc_k*dim_k]  D_k = [Du Dx] (dim_k = s, or n at k = N)
 *   ws  [batch][N*s + n]           w_k = [u_k; x_k], then x_N
 *   ys, zs, rho, inv_rho [batch][sum_k nc_k]
 *   x0  [batch][n]
 * Pointers are host or device memory as the `mem` argument says; host buffers
 * are borrowed for the call only (copied to device before the call returns
 * or, for outputs, after the stream has drained).  One HIP stream per handle;
 * a handle is not thread-safe.
 */
#ifndef PDPLQR_H
#define PDPLQR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PDPLQR_VERSION_MAJOR 0
#define PDPLQR_VERSION_MINOR 2

/* status codes */
#define PDPLQR_OK 0
#define PDPLQR_ERR_INVALID (-1)     /* bad argument / configuration            */
#define PDPLQR_ERR_HIP (-2)         /* HIP runtime error (message in last_error) */
#define PDPLQR_ERR_ALLOC (-3)       /* device allocation failed                 */
#define PDPLQR_ERR_STATE (-4)       /* protocol order violated                  */
#define PDPLQR_ERR_UNSUPPORTED (-5) /* shape/solver not supported by this build */
#define PDPLQR_ERR_NUMERIC (-6)     /* factorization failure (QDLDL path)       */

/* memory location of pointer arguments */
#define PDPLQR_MEM_HOST 0
#define PDPLQR_MEM_DEVICE 1

/* solver kinds: the three reference solvers */
#define PDPLQR_SOLVER_SERIAL 0   /* LQRSolver          (lqr_solver.hpp:9-77)            */
#define PDPLQR_SOLVER_PARALLEL 1 /* LQRParallelSolver  (lqr_solver_parallel.hpp:19-238) */
#define PDPLQR_SOLVER_KKT 2      /* QDLDLSolver        (qdldl_solver.hpp:14-151)        */

/* CondensedSystemSolverType (lqr_solver_parallel.hpp:14-17) */
#define PDPLQR_CONDENSED_LU 0
#define PDPLQR_CONDENSED_CHOLESKY 1

typedef struct pdplqr_handle_s *pdplqr_handle;

/* Construction arguments.  Replaces the solver constructors
 *   LQRSolver(const LQRModel&)                                  lqr_solver.hpp:11,31-39
 *   LQRParallelSolver(model, num_segments, load_balancing, type) lqr_solver_parallel.hpp:22-25,64-113
 *   QDLDLSolver(const LQRModel&)                                qdldl_solver.hpp:17,36-45
 * plus the LQRModel dimensions (lqr_model.hpp:74-80).  `batch` independent
 * problems of identical shape are solved together (new: the reference has no
 * batch API).  `ncs` (N+1 entries, shared by the batch) may be NULL (all 0). */
typedef struct {
    int32_t nx, nu, N;
    int32_t batch;
    int32_t solver;          /* PDPLQR_SOLVER_*                                   */
    int32_t num_segments;    /* PARALLEL: reference segment count (>= 1)          */
    int32_t load_balancing;  /* PARALLEL: alpha = 1.55 segmentation (:70)         */
    int32_t condensed_type;  /* PARALLEL: PDPLQR_CONDENSED_*                      */
    int32_t device;          /* HIP device ordinal                                 */
    int32_t keep_factors;    /* keep L_k, lp_k per stage (needed by
                                backward_without_factorization and the value
                                function getter); 0 = keep only the rollout
                                gains K_k, d_k                                     */
    const int32_t *ncs;      /* N+1 constraint counts or NULL                      */
    double rho_dyn;          /* KKT: lambda regularization, reference 1e-6 (:38)   */
    double kkt_sigma;        /* KKT: sigma frozen into the matrix, reference 1e-6 (:39) */
    int32_t segment_len;     /* PARALLEL: device sub-segment length (0 = auto).  Every
                                reference segment is refined into pieces of at most this
                                many stages; results are identical up to rounding. */
    int32_t num_devices;     /* PARALLEL: > 1 splits the horizon into num_devices
                                contiguous slices, one per GPU, driven by this one
                                handle (replaces the OpenMP team of
                                LQRParallelSolver, lqr_solver_parallel.hpp:22-25,102-113):
                                slice backward on every device, one RCCL all-gather of
                                the slice elements (3 nx^2 + 2 nx doubles per problem),
                                slice forward.  0 or 1: one device (`device`).
                                backward_without_factorization all-gathers only the
                                slices' (f, p) (2 nx doubles per problem,
                                lqr_solver_parallel.hpp:207-210); admm_solve runs its
                                vectors on the first device around the slices' protocol
                                calls.  With num_devices > 1 the shard_* calls are
                                unsupported, `device` is ignored, and set_stream takes
                                the caller's stream on devices[0] (see below).  num_devices = 1 with a non-NULL
                                `devices` runs the same split with one slice (RCCL
                                communicator of one rank). */
    const int32_t *devices;  /* num_devices HIP ordinals, or NULL = 0 .. num_devices - 1.
                                A device may repeat (same-device rehearsal: the exchange
                                then uses device copies, as with PDPLQR_MD_P2P=1). */
} pdplqr_config;

/* Fill `cfg` with the reference defaults (keep_factors = 1, load_balancing = 1,
 * CHOLESKY, rho_dyn = kkt_sigma = 1e-6).
 * Shape limits of this build (the reference is size-generic, lqr_kernel.hpp:104-147):
 * nx + nu <= 256 for every solver: up to 32 on MFMA tiles in one wavefront,
 * 33..64 on register tiles or LDS-resident stage matrices, one 256-thread
 * block per problem / segment / element (kernels_big.hip, kernels_wide.hip);
 * KKT rows per stage <= 64 past the block LDL^T tiles; 65..256 on
 * global-memory stage and element matrices (kernels_xl.hip, kernels_xl_par.hip:
 * every protocol call, pdplqr_admm_solve and the horizon-shard calls; KKT rows
 * per stage <= 256 there).  pdplqr_create returns
 * PDPLQR_ERR_UNSUPPORTED past them. */
void pdplqr_config_init(pdplqr_config *cfg);

int pdplqr_create(const pdplqr_config *cfg, pdplqr_handle *out);
int pdplqr_destroy(pdplqr_handle h);

/* Thread-local message of the last failing call ("" if none). */
const char *pdplqr_last_error(void);

/* Stream control (hipStream_t passed as void*). NULL = the handle's own stream.
   Switching makes the new stream wait (an event, no host sync) for what the
   handle queued on the old one, e.g. set_model's upload: the event is recorded
   on the OLD stream, so that stream must still be alive when the handle
   switches away from it (switch before destroying a stream the handle uses).
   num_devices > 1: the stream is the caller's, on devices[0] (else
   PDPLQR_ERR_INVALID); the slices keep their own streams, wait (an event) for
   the caller's stream before reading device inputs, and the caller's stream
   waits for the slices' work at the end of every call, forward's device
   outputs included -- no host synchronisation.  NULL (the default): device
   inputs are read after a drain of every slice device, and forward returns
   with ws complete. */
int pdplqr_set_stream(pdplqr_handle h, void *hip_stream);
void *pdplqr_get_stream(pdplqr_handle h);
int pdplqr_synchronize(pdplqr_handle h);

/* Problem data, reference layout.  Replaces filling LQRModel::nodes[k].{E,c,H,h,D_con}
 * (lqr_model.hpp:8-64,85-88) and the solver's `const LQRModel& model_` read
 * (lqr_solver.hpp:25).  D may be NULL when all nc_k = 0.  For the KKT solver the
 * matrix is frozen here, as QDLDLSolver freezes it at construction (qdldl_solver.hpp:40-42). */
int pdplqr_set_model(pdplqr_handle h, const double *E, const double *c, const double *H, const double *hv,
                     const double *D, int mem);

/* The same upload restricted to the arrays in `mask` (PDPLQR_MODEL_*; the other
 * pointers are ignored and may be NULL).  The reference reads its model lazily
 * -- H, h when update_problem_data copies them (lqr_solver.hpp:41-56), E, c,
 * D_con when backward / forward run (lqr_kernel.hpp:118-119,186-188) -- so the
 * C++ facade re-uploads exactly the arrays a call reads, and only those that
 * changed.  An upload of E, c or D alone keeps the protocol state (a backward
 * may follow the update directly); H or h needs a new update_problem_data. */
#define PDPLQR_MODEL_E 1
#define PDPLQR_MODEL_C 2
#define PDPLQR_MODEL_H 4
#define PDPLQR_MODEL_HV 8
#define PDPLQR_MODEL_D 16
#define PDPLQR_MODEL_ALL 31
int pdplqr_set_model_arrays(pdplqr_handle h, int mask, const double *E, const double *c, const double *H,
                            const double *hv, const double *D, int mem);

/* Model bytes copied host -> device by set_model / set_model_arrays since the
 * handle was created (device-memory uploads are not counted). */
int pdplqr_get_model_upload_bytes(pdplqr_handle h, int64_t *bytes);

/* LQRSolver::update_problem_data(ws, ys, zs, inv_rho_vecs, sigma)      lqr_solver.hpp:41-56
 * LQRParallelSolver::update_problem_data                               lqr_solver_parallel.hpp:115-140
 * QDLDLSolver::update_problem_data -> KKTSystem::form_rhs              qdldl_solver.hpp:80-86, kkt.hpp:224-300
 * ys/zs/inv_rho may be NULL when all nc_k = 0. */
int pdplqr_update_problem_data(pdplqr_handle h, const double *ws, const double *ys, const double *zs,
                               const double *inv_rho, double sigma, int mem);

/* LQRSolver::backward(rho_vecs)                                         lqr_solver.hpp:58-63
 * LQRParallelSolver::backward(rho_vecs)                                 lqr_solver_parallel.hpp:142-146
 * QDLDLSolver::backward(inv_rho_vecs) -- NOTE the KKT solver takes the  qdldl_solver.hpp:88-109
 * INVERSE rho vectors, as the reference's does. */
int pdplqr_backward(pdplqr_handle h, const double *rho, int mem);

/* LQRSolver::backward_without_factorization                            lqr_solver.hpp:65-70
 * LQRParallelSolver::backward_without_factorization                    lqr_solver_parallel.hpp:148-154
 * Requires keep_factors = 1 and a preceding pdplqr_backward. */
int pdplqr_backward_without_factorization(pdplqr_handle h, const double *rho, int mem);

/* LQRSolver::forward(x0, ws)                                            lqr_solver.hpp:72-77
 * LQRParallelSolver::forward(x0, ws)                                    lqr_solver_parallel.hpp:213-238
 * QDLDLSolver::forward(x0, ws)                                          qdldl_solver.hpp:111-151
 * Writes every ws entry (ws[0].x = x0 included).  Host `ws` is written after
 * the stream drains; device `ws` is written asynchronously on the stream. */
int pdplqr_forward(pdplqr_handle h, const double *x0, double *ws, int mem);

/* LQRSolver::clear_workspace (lqr_solver.hpp:12-14) */
int pdplqr_clear_workspace(pdplqr_handle h);

/* Value function of problem b at stage k: P = Lxx Lxx^T (n x n, column-major)
 * and p = lp.tail(n), from the serial workspace (lqr_solver.hpp:24-26 keeps it
 * protected; the condensed systems form P the same way, condensed_system.hpp:69,188).
 * SERIAL solver with keep_factors = 1 only.  Host outputs. */
int pdplqr_get_value_function(pdplqr_handle h, int32_t b, int32_t k, double *P, double *p);

/* Adjoint solve (new: the reference has no such call).  For a scalar loss l on
 * the solution w* of the problem the handle last factored,
 *     min sum 1/2 w_k^T H~_k w_k + h~_k^T w_k   s.t. x_{k+1} = E_k w_k + c_k, x_0 = x0
 * (H~ = H + sigma I, h~ = h - sigma w of update_problem_data), writes
 * dl/dE, dl/dc, dl/dH, dl/dh, dl/dx0 in the boundary layouts of E, c, H, h, x0,
 * given `ws` (the solution the last forward returned) and `gws` = dl/dws
 * ([batch][N*s + n]).  gH is the gradient with respect to the symmetric matrix
 * (dl = <gH, dH> for symmetric dH; sigma does not enter it).  One
 * backward_without_factorization and one forward on the cached factor give the
 * adjoint solution, one streamed pass the gradients.
 * Any output may be NULL: its work and traffic are skipped.  All non-NULL
 * pointers live in `mem`.  SERIAL solver, keep_factors = 1, one device, no
 * constraint rows, nx + nu <= 64 (PDPLQR_ERR_UNSUPPORTED otherwise); needs a
 * preceding pdplqr_backward (PDPLQR_ERR_STATE).  The handle's state is
 * unchanged: forward, backward_without_factorization and get_value_function
 * behave as if the call had not happened. */
int pdplqr_adjoint(pdplqr_handle h, const double *ws, const double *gws, double *gE, double *gc, double *gH,
                   double *gh, double *gx, int mem);

/* pdplqr_adjoint for a PARALLEL (segmented) handle (new).  Arguments, layouts,
 * the NULL-skips-work rule and the gradients are pdplqr_adjoint's (gH with
 * respect to the symmetric matrix, exactly symmetric, sigma not in it); `ws`
 * is the solution of the problem the handle last factored (it need not come
 * from this handle's forward, and no forward has to precede the call).  The
 * adjoint solution costs one segmented backward_without_factorization and one
 * segmented forward (log depth in the horizon); the per-stage costates, which
 * a PARALLEL handle does not cache, are recovered by one wave per device
 * segment walking back from the boundary costates of the suffix scans, in a
 * form whose rounding does not grow along a segment.
 * PARALLEL solver of either condensed type, keep_factors = 1, one device, no
 * constraint rows, nx + nu <= 64 (PDPLQR_ERR_UNSUPPORTED otherwise); needs a
 * preceding pdplqr_backward, and a handle driven by the pdplqr_shard_* calls
 * must hold the last shard (PDPLQR_ERR_STATE); NULL ws or gws is
 * PDPLQR_ERR_INVALID.  A refused call writes nothing.  The handle's state is
 * unchanged: forward returns the bits it returned before, and
 * update_problem_data -> backward_without_factorization -> forward behave as
 * if the call had not happened.  Device buffers: nothing waits for the device. */
int pdplqr_adjoint_parallel(pdplqr_handle h, const double *ws, const double *gws, double *gE, double *gc,
                            double *gH, double *gh, double *gx, int mem);

/* The adjoint of the penalised x-update (new): pdplqr_adjoint for handles with
 * constraint rows.  The handle last factored
 *     H~_k = H_k + sigma I + D_k^T R D_k,   h~_k = h_k - sigma wbar_k - D_k^T R g_k
 * with R = diag(rho) (the vector given to pdplqr_backward, passed again here;
 * NULL only when no stage has rows) and g = zs - inv_rho o ys as
 * update_problem_data left it; `ws` is the solution forward returned.  The loss
 * may depend on the solution and on the rows' values:
 *     gws = dl/dws [batch][N*s + n],  gvs = dl/d(D ws) [batch][sum nc_k] (NULL = 0),
 * and the adjoint solve runs on the cached factor with the right-hand side
 * gws + D^T gvs.  gE, gc, gH, gh, gx are as in pdplqr_adjoint (gH with respect
 * to the model's H).  With r = D_k v_k (v the adjoint solution, = gh) and
 * e = D_k w_k - g_k per row:
 *     gD   [batch][sum nc_k*dim_k]  (rho o e) v_k^T + (rho o r + gvs_k) w_k^T, in D's layout
 *     gg   [batch][sum nc_k]        -rho o r : the gradient of the penalty target g
 *     grho [batch][sum nc_k]        r o e    : the gradient of rho with g held fixed
 * The inputs of update_problem_data follow from these without further outputs:
 *     dl/dzs = gg,  dl/dys = -inv_rho o gg,  dl/dinv_rho = -ys o gg,  dl/dwbar = -sigma gh.
 * Any output may be NULL: its work and traffic are skipped.  Preconditions and
 * the unchanged handle state are pdplqr_adjoint's, except that rows are allowed;
 * without rows the results equal pdplqr_adjoint's bit for bit.  A stage whose rows
 * do not fit the rows kernel's 40 KB LDS tile (32 bytes per row plus 16 (nx + nu))
 * is PDPLQR_ERR_UNSUPPORTED.  A refused call
 * writes nothing. */
int pdplqr_adjoint_rows(pdplqr_handle h, const double *ws, const double *rho, const double *gws, const double *gvs,
                        double *gE, double *gc, double *gH, double *gh, double *gx, double *gD, double *gg,
                        double *grho, int mem);

/* Per-problem factorization status after backward: 0 = ok, otherwise 1 + the
 * first stage whose Cholesky met a non-positive pivot (the reference ignores
 * Eigen's LLT info, lqr_kernel.hpp:89,126).  `flags` has `batch` entries, host. */
int pdplqr_get_status(pdplqr_handle h, int32_t *flags);

/* Segmentation actually used by a PARALLEL handle (lqr_solver_parallel.hpp:64-88):
 * idx_start/Nseg each hold num_segments entries, host. */
int pdplqr_get_segments(pdplqr_handle h, int32_t *idx_start, int32_t *Nseg);

/* ---------------------------------------------------------------------- */
/* Horizon sharding across GPUs (new; the reference is one process).       */
/* A PARALLEL handle built with pdplqr_config.N = the LOCAL slice length   */
/* solves its slice; ranks exchange one segment element each (RCCL over    */
/* xGMI, done by the caller) between the two phases:                        */
/*   pdplqr_shard_backward   -> element (F, C, f, P, p) in `elem_out`       */
/*   all-gather of elements across ranks                                    */
/*   pdplqr_shard_forward    <- every rank's element, this rank's index     */
/* Element layout (doubles): F[n*n] C[n*n] f[n] P[n*n] p[n] (3n^2+2n).      */
/* ---------------------------------------------------------------------- */
int pdplqr_shard_element_size(pdplqr_handle h);
int pdplqr_shard_backward(pdplqr_handle h, const double *rho, int is_last_shard, double *elem_out, int mem);
/* LQRParallelSolver::backward_without_factorization (lqr_solver_parallel.hpp:148-154,190-211)
 * on the slice: keep_factors = 1 and a preceding pdplqr_shard_backward with the same
 * is_last_shard.  Writes the whole element; only its f and p differ from the
 * factorising call's (F, C, P bit-identical), so ranks need to exchange only
 * f, p (2n doubles per problem) and keep the rest of the last all-gather. */
int pdplqr_shard_backward_without_factorization(pdplqr_handle h, const double *rho, int is_last_shard,
                                                double *elem_out, int mem);
int pdplqr_shard_forward(pdplqr_handle h, const double *x0, const double *elems_all, int32_t num_shards,
                         int32_t shard_id, double *ws, int mem);

/* The slicing of a num_devices = R split (pdplqr_config.num_devices), host
 * arithmetic only (no device call): per slice r, 8 int64 at out[8 r]:
 * N0, N1 (stages [N0, N1)), last (holds the real terminal), y0 / ny_stages (its
 * stages' constraint rows in the full y vector), nc_terminal (its terminal's
 * rows: nc_N for the last slice, 0 otherwise), d0 / nd_stages (its stages'
 * entries in the full D array).  ncs: N+1 entries or NULL. */
int pdplqr_multidev_plan(int32_t N, int32_t R, const int32_t *ncs, int32_t nx, int32_t nu, int64_t *out);

/* ---------------------------------------------------------------------- */
/* ADMM outer loop for conic LQ (new).  The         */
/* reference stores e_lb <= D_con w <= e_ub (lqr_model.hpp:21-24) and       */
/* solves the ADMM x-update (update_problem_data / backward / forward,      */
/* lqr_solver.hpp:41-77), but the outer loop is absent (README.md:8).       */
/* This runs it on the device for the whole batch: OSQP's iteration        */
/* (Stellato et al. 2020, Algorithm 1) with the dynamics solved exactly by  */
/* the handle's solver, projection onto [lb, ub], sigma fixed, rho fixed or */
/* adapted by OSQP's rule (settings.adaptive_rho), and                     */
/* the ADMM residuals of admm.hip's header.  Works with all three solver    */
/* kinds; iterations >= 2 reuse the first iteration's factorization         */
/* (backward_without_factorization with keep_factors = 1).                  */
/* ---------------------------------------------------------------------- */
typedef struct {
    double sigma;        /* proximal weight (lqr_example.cpp:170: 1e-6)            */
    double alpha;        /* over-relaxation, 0 < alpha < 2 (OSQP default 1.6)      */
    int32_t max_iter;    /* iteration cap                                          */
    int32_t check_every; /* termination test period (one 4-byte D2H read each)     */
    double eps_abs, eps_rel; /* tolerances (OSQP defaults 1e-3); 0 = run max_iter  */
    int32_t adaptive_rho;    /* 1: OSQP's rho update at each termination test (a  */
                             /* per-problem scale of rho, then one refactorization) */
    double adaptive_rho_tolerance; /* rescale when the estimate leaves [1/tol, tol] (5) */
} pdplqr_admm_settings;

void pdplqr_admm_settings_init(pdplqr_admm_settings *s);

/* x0 [batch][n]; lb, ub, rho [batch][ny] (e_lb, e_ub, rho_vecs of          */
/* lqr_example.cpp:12-50,169); ws [batch][N*s+n], ys, zs [batch][ny]: warm   */
/* start in, solution out (w^k, y^k, z^k of the last iteration).  After the */
/* call the handle is "updated and factored" (forward may follow).          */
int pdplqr_admm_solve(pdplqr_handle h, const pdplqr_admm_settings *s, const double *x0, const double *lb,
                      const double *ub, const double *rho, double *ws, double *ys, double *zs, int mem);

/* Per-problem outcome of the last admm_solve (host arrays of `batch`        */
/* entries, each may be NULL): iterations run, 1 if the termination test     */
/* passed, primal / dual residual at the last test; `rho` (batch * ny, may be */
/* NULL) the final rho vectors.  Returns the number of iterations of the     */
/* batch (>= 1) or an error code.                                             */
int pdplqr_admm_info(pdplqr_handle h, int32_t *iters, int32_t *converged, double *prim_res, double *dual_res,
                     double *rho);

/* ---------------------------------------------------------------------- */
/* Infeasibility detection of the ADMM loop (new; OSQP's certificates,     */
/* Stellato et al. 2020 section 3.4, in the coordinates of the dynamics'    */
/* affine set -- the x-update solves the dynamics exactly).  */
/* A problem whose feasible set {w : dynamics, lb <= D w <= ub} is empty,   */
/* or whose cost is unbounded below on it, is recognised at a termination   */
/* test, frozen like a converged one and reported by pdplqr_admm_status.    */
/* Limits: SERIAL and PARALLEL handles on one device (num_devices 0 or 1    */
/* without `devices`), nx + nu <= 64, any ncs, either keep_factors value;   */
/* PDPLQR_ERR_UNSUPPORTED otherwise (the KKT solver softens its dynamics by */
/* rho_dyn, so "infeasible" is not the same statement there).  A small rho  */
/* or a long unstable horizon (nu grows with |A^T|^N) certifies slowly.     */
/* ---------------------------------------------------------------------- */
#define PDPLQR_ADMM_UNSOLVED 0          /* ran to max_iter                       */
#define PDPLQR_ADMM_SOLVED 1            /* the termination test passed           */
#define PDPLQR_ADMM_PRIMAL_INFEASIBLE 2 /* no feasible point                     */
#define PDPLQR_ADMM_DUAL_INFEASIBLE 3   /* cost unbounded below                  */

/* Detection state of the handle (default: off; with it off admm_solve        */
/* launches and copies nothing new and its results are unchanged bit for bit). */
/* eps_prim_inf / eps_dual_inf: OSQP's defaults are 1e-4; a tolerance of 0     */
/* switches that one test off; negative or NaN with `enable` set is            */
/* PDPLQR_ERR_INVALID.  With dy = y^{k+1} - y^k, dw = w^{k+1} - w^k at a       */
/* termination test and |.| the max-norm, a bound with |value| >= 1e20 being   */
/* infinite:                                                                   */
/*   primal: nu_N = q_N, [g_k; nu_k] = q_k + E_k^T nu_{k+1} with q_k = D_k^T   */
/*     dy_k, beta = sum_k nu_{k+1}^T c_k + nu_0^T x0; certified when |dy| > 0, */
/*     max_k |g_k| <= eps |dy|, no row has dy_i > eps |dy| with ub_i infinite  */
/*     or dy_i < -eps |dy| with lb_i infinite, and                             */
/*     sum_i [ub_i (dy_i)+ + lb_i (dy_i)-] - beta < -eps |dy| (finite bounds); */
/*   dual: certified when |dw| > 0, |H_k dw_k| <= eps |dw| for all k (the      */
/*     model's H, without sigma), sum_k h_k^T dw_k < -eps |dw|, |dx_0| and     */
/*     |dx_{k+1} - E_k dw_k| <= eps |dw|, and for every row (D dw)_i <= eps    */
/*     |dw| where ub_i is finite, >= -eps |dw| where lb_i is finite.           */
/* A problem that passes the termination test in the same pass is SOLVED.     */
int pdplqr_admm_set_infeasibility_detection(pdplqr_handle h, int enable, double eps_prim_inf, double eps_dual_inf);

/* PDPLQR_ADMM_* of every problem after the last admm_solve (host array of    */
/* `batch` entries).  With detection off only 0 and 1 occur and the value     */
/* equals `converged` of pdplqr_admm_info.  PDPLQR_ERR_STATE before any       */
/* admm_solve.                                                                 */
int pdplqr_admm_status(pdplqr_handle h, int32_t *status);

/* The certificates of the last admm_solve: dy [batch][ny], dw [batch][N*s+n] */
/* (either may be NULL), both in `mem`.  A problem with status 2 or 3 gets    */
/* the dy / dw of the deciding test, every other problem zeros.               */
/* PDPLQR_ERR_STATE unless detection was on in the last admm_solve.           */
int pdplqr_admm_certificate(pdplqr_handle h, double *dy, double *dw, int mem);

/* The two certificate tests on given vectors, without the loop: needs only   */
/* set_model, same limits as above; changes no handle state.  x0 [batch][n],  */
/* lb, ub, dy [batch][ny], dw [batch][N*s+n], all pointers in `mem`.          */
/* measures [batch][8]:                                                        */
/*   [0] |dy|   [1] max_k |g_k|   [2] the support term (the sum minus beta)   */
/*   [3] 1 if a row with an infinite bound fails the sign test, else 0        */
/*   [4] |dw|   [5] max_k |H_k dw_k|   [6] h^T dw                             */
/*   [7] max of the dynamics residuals (dx_0 included) and the row violations */
/* verdict [batch]: bit 0 = primal certificate holds, bit 1 = dual.  dy or dw */
/* NULL skips that half (its measures are 0, its bit clear; lb, ub may then   */
/* be NULL only when no stage has rows).                                       */
int pdplqr_admm_check_certificates(pdplqr_handle h, const double *x0, const double *lb, const double *ub,
                                   const double *dy, const double *dw, double eps_prim_inf,
                                   double eps_dual_inf, double *measures, int32_t *verdict, int mem);

/* ---------------------------------------------------------------------- */
/* Polish of the ADMM solution (new; OSQP's polish, Stellato et al. 2020    */
/* section 4, with the dynamics kept as hard constraints).   */
/* admm_solve stops at first-order accuracy (eps); the polish guesses the   */
/* active rows from (y, z), solves the equality-constrained problem on them */
/* regularised by delta, and refines: refine_iter + 1 penalised x-updates   */
/* of the protocol with sigma = delta, rho = 1/delta on the active rows and */
/* 0 on the rest, zs = the active bounds, each followed by                  */
/*   y <- y + (D_a w - b_a) / delta.                                        */
/* Same limits as infeasibility detection (SERIAL and PARALLEL, one device, */
/* nx + nu <= 64, any ncs, either keep_factors value: with keep_factors = 0 */
/* every refinement step factorises); PDPLQR_ERR_UNSUPPORTED otherwise.     */
/* ---------------------------------------------------------------------- */
#define PDPLQR_POLISH_NOT_ATTEMPTED 0 /* the problem did not end SOLVED           */
#define PDPLQR_POLISH_ACCEPTED 1      /* the polished (w, y, z) were written back */
#define PDPLQR_POLISH_REJECTED 2      /* the ADMM iterate is kept, bit for bit    */

/* Polish state of the handle (default: off; with it off admm_solve launches  */
/* and copies nothing new and its results are unchanged bit for bit).  OSQP's */
/* defaults: delta = 1e-6, refine_iter = 3.  delta <= 0 or not finite, or      */
/* refine_iter < 0, with `enable` set is PDPLQR_ERR_INVALID.  With it on,      */
/* admm_solve, after its loop and on the handle's stream:                      */
/*   classifies every row: lower-active if lb == ub or z - lb < -y, else       */
/*     upper-active if ub - z < y (OSQP's rule);                               */
/*   runs the refinement from (w, y on the active rows, 0 elsewhere);          */
/*   takes the KKT measures (pdplqr_admm_kkt_residuals) of the ADMM (w, y) and */
/*     of the polished pair; with pri = max([0], [1]) and dua = [2] the        */
/*     polished pair is accepted when pri_pol < pri && dua_pol < dua, or       */
/*     pri_pol < pri && dua < 1e-10, or dua_pol < dua && pri < 1e-10;          */
/*   an accepted problem gets w, y and z = clamp(D w, lb, ub); a rejected one, */
/*     one that did not end SOLVED, or one whose polish factorisation failed   */
/*     keeps its ADMM w, y, z bit for bit.                                     */
/* pdplqr_admm_info and pdplqr_admm_status are unchanged.  After the call the  */
/* handle is "updated and factored" for the POLISHING system: a following      */
/* pdplqr_forward returns the last polish iterate of every problem.            */
int pdplqr_admm_set_polish(pdplqr_handle h, int enable, double delta, int32_t refine_iter);

/* The polish of the last admm_solve, host arrays, any of them NULL:          */
/* status [batch] (PDPLQR_POLISH_*), n_active [batch] (rows guessed active),  */
/* measures [batch][8]: the four KKT measures of the ADMM iterate, then of    */
/* the polished pair.  PDPLQR_ERR_STATE unless polish was on in that solve.   */
int pdplqr_admm_polish_info(pdplqr_handle h, int32_t *status, int32_t *n_active, double *measures);

/* The KKT measures of any (w, y), without the loop: needs only set_model,    */
/* same limits as above; changes no handle state.  x0 [batch][n], lb, ub, ys  */
/* [batch][ny], ws [batch][N*s+n], measures [batch][4], all pointers in `mem`.*/
/* With v = D w, |.| the max-norm and a bound with |value| >= 1e20 infinite:  */
/*   [0] the row residual max_i |v_i - clamp(v_i + y_i, lb_i, ub_i)| (the     */
/*       natural map: zero iff v is within the bounds and y in their normal   */
/*       cone -- bound violation, multiplier sign and complementarity in one) */
/*   [1] the dynamics residual max(|x_0 - x0|, max_k |x_{k+1} - E_k w_k - c_k|)*/
/*   [2] the reduced gradient max_k |g_k|: nu_N = q_N, [g_k; nu_k] = q_k +    */
/*       E_k^T nu_{k+1}, q_k = H_k w_k + h_k + D_k^T y_k (the model's H,      */
/*       without sigma)                                                       */
/*   [3] the objective sum_k 1/2 w_k^T H_k w_k + h_k^T w_k                    */
int pdplqr_admm_kkt_residuals(pdplqr_handle h, const double *x0, const double *lb, const double *ub,
                              const double *ws, const double *ys, double *measures, int mem);

/* ---------------------------------------------------------------------- */
/* Gradients of the box-constrained optimum of the last admm_solve (new;    */
/* DESIGN.md 5.9).  The polish left a guessed active set (rows D_a, targets */
/* b: lb on the lower-active rows, ub on the upper-active ones) and a       */
/* handle that factors the polishing system H + delta I + D_a^T D_a / delta. */
/* The adjoint of the equality-constrained KKT solve on that set is one     */
/* more solve with the same symmetric matrix, so the polish's iterative     */
/* refinement serves it with another right-hand side.  On the handle's      */
/* stream, with no host wait:                                                */
/*   1. the polishing x-update at the returned (w, y) is run again          */
/*      (update_problem_data, backward, forward): factor, lp and its        */
/*      solution w~ belong together whatever protocol calls ran in between; */
/*   2. g~ = gws + D^T gvs;                                                  */
/*   3. v = 0, eta = 0; refine_iter + 1 times: v <- the adjoint solve on    */
/*      the cached factor with h~ := g~ - delta v + D_a^T eta, c := 0,      */
/*      x0 := 0 (pdplqr_adjoint's); eta <- eta + (D_a v) / delta;           */
/*   4. gE, gc, gH, gh, gx by pdplqr_adjoint's formulas on (w~, v), and     */
/*      with y_a = y on the active rows, 0 elsewhere:                        */
/*        gD  = y_a,k v_k^T + (eta_k + gvs_k) w~_k^T   (D's layout)         */
/*        glb = -eta on the lower-active rows, gub = -eta on the upper-     */
/*        active rows, 0 elsewhere.  A row's side is the polish             */
/*        classification's: a row with lb == ub is lower-active, its whole  */
/*        gradient goes to glb.                                              */
/* gws = dl/dws [batch][N*s+n]; gvs = dl/d(D ws) [batch][ny] (NULL = 0);     */
/* gE, gc, gH, gh, gx, gD in the boundary layouts of pdplqr_adjoint_rows;    */
/* glb, gub [batch][ny].  Any output may be NULL: its work and stores are   */
/* skipped.  All non-NULL pointers live in `mem`.  delta and refine_iter    */
/* are the handle's (pdplqr_admm_set_polish).  Everything                   */
/* pdplqr_adjoint_rows requires (SERIAL, keep_factors = 1, one device,      */
/* nx + nu <= 64, every stage's rows within the rows kernel's LDS tile),    */
/* at least one constraint row, and the last pdplqr_admm_solve ran with     */
/* polish on; PDPLQR_ERR_UNSUPPORTED / PDPLQR_ERR_STATE otherwise.  A       */
/* refused call writes nothing.  The call reads only what that solve left   */
/* (w, y, x0, lb, ub, the classification).  Afterwards the handle is        */
/* "updated and factored" for the polishing system at the solution: a       */
/* following pdplqr_forward returns w~; admm_info, admm_status, polish_info */
/* and the solve's w, y, z are untouched.                                    */
/* ---------------------------------------------------------------------- */
#define PDPLQR_ADMM_ADJOINT_EXACT 1  /* the polish was accepted: the optimum's gradient if the guess was right */
#define PDPLQR_ADMM_ADJOINT_APPROX 2 /* polish rejected or not SOLVED: the guessed set at the ADMM iterate     */
#define PDPLQR_ADMM_ADJOINT_FAILED 3 /* the factorisation of step 1 failed: this problem's outputs are unspecified */

int pdplqr_admm_adjoint(pdplqr_handle h, const double *gws, const double *gvs, double *gE, double *gc, double *gH,
                        double *gh, double *gx, double *gD, double *glb, double *gub, int mem);

/* The last pdplqr_admm_adjoint, host arrays, either may be NULL: status     */
/* [batch] (PDPLQR_ADMM_ADJOINT_*); resid [batch][2]: max|D_a v| / max|v|    */
/* after the last step, and max|v_new - v_old| / max|v_new| of the last step. */
/* PDPLQR_ERR_STATE before any pdplqr_admm_adjoint.                           */
int pdplqr_admm_adjoint_info(pdplqr_handle h, int32_t *status, double *resid);

/* ---------------------------------------------------------------------- */
/* Second-order cone rows of the ADMM loop (new).  Some of   */
/* a stage's constraint rows form cones: the z-update of admm_solve then    */
/* projects onto the mixed set (box rows: clamp; the rows of a cone, with   */
/* p = v - lb: |x| <= t keeps p, |x| <= -t gives 0, otherwise (a |x|, a x)  */
/* with a = (1 + t / |x|) / 2; |x| is the square root of the squares summed */
/* in row order, without rescaling).  Everything else of the iteration --   */
/* the y and w updates, the termination test, the freezing of converged     */
/* problems, adaptive rho (a cone counts as an active row when its          */
/* projection's argument had |x| >= t), admm_info, admm_status -- is         */
/* unchanged, and a handle with no cones set launches what it launched      */
/* before.  Examples: |u_k| <= u_max is the rows [0; I_m 0] with             */
/* lb = (-u_max, 0, ..); a terminal ball |x_N| <= r the same on stage N.    */
/* ---------------------------------------------------------------------- */

/* cones of the handle's constraint rows, shared by the batch (host arrays, copied).
 * Cone i covers rows [cone_row[i], cone_row[i] + cone_dim[i]) of stage cone_stage[i]
 * (0..N; row indices are within the stage).  For those rows, with v = D_k w_k and b = lb:
 *     v - b  in  K_q = { (t, x) : |x|_2 <= t },  first row = t
 * ub of a cone row is not read (it still has to pass the existing lb <= ub check: pass ub = lb).
 * Rows in no cone stay box rows.  num_cones = 0 clears.
 * PDPLQR_ERR_INVALID: cone_dim < 2, a stage outside 0..N, a cone that leaves its stage's
 * rows, overlapping or unsorted cones (order: stage, then row).  PDPLQR_ERR_UNSUPPORTED: a
 * KKT handle (its softened dynamics make the split a different problem), num_devices > 1
 * or a non-NULL `devices`, nx + nu > 64, cone_dim > nx + nu + 1 (nx + 1 at the terminal
 * stage).  A refused call leaves the previous cones in place.
 * With cones set, pdplqr_admm_solve returns PDPLQR_ERR_UNSUPPORTED while infeasibility
 * detection or polish is on (hence pdplqr_admm_adjoint too), PDPLQR_ERR_INVALID when rho is
 * not constant within a cone (the projection is Euclidean only then; the adaptive rule
 * scales per problem and keeps it constant) or a cone row's lb is not finite (|lb| >= 1e20
 * included) -- a refused solve writes nothing to ws, ys, zs -- and
 * pdplqr_admm_kkt_residuals / pdplqr_admm_check_certificates return PDPLQR_ERR_UNSUPPORTED
 * (they would read cone rows as boxes). */
int pdplqr_admm_set_cones(pdplqr_handle h, int32_t num_cones, const int32_t *cone_stage,
                          const int32_t *cone_row, const int32_t *cone_dim);
/* out = the projection of v onto the handle's constraint set (box rows: clamp; cone rows:
 * b + P_K(v - b)); v, lb, ub, out [batch][ny] in `mem`; needs only create (+ set_cones). */
int pdplqr_admm_project(pdplqr_handle h, const double *v, const double *lb, const double *ub,
                        double *out, int mem);
/* The transposed Jacobian of that projection at v applied to gout, the cotangent of its
 * output: gv = J^T gout, and glb, gub the cotangents of the bounds; all [batch][ny] in
 * `mem`, any of the three outputs may be NULL.  Box rows: gv = gout where lb < v < ub, else
 * 0; glb = gout where v <= lb; gub = gout where v >= ub (a row with lb == ub gives both).
 * Cone rows, with p = v - lb = (t, x), r = |x| and g = (g_t, g_x): the case is the one
 * pdplqr_admm_project takes for the same bits; r <= t: J = I; r <= -t: J = 0; otherwise,
 * with xh = x / r and d = xh . g_x,
 *     (J g)_t = (g_t + d) / 2,   (J g)_x = (g_t xh + (1 + t / r) g_x - (t / r) d xh) / 2
 * (J is symmetric).  gv = J g, glb = g - J g, gub = 0.  Needs only create (+ set_cones),
 * changes no handle state; the limits and error codes of pdplqr_admm_project. */
int pdplqr_admm_project_vjp(pdplqr_handle h, const double *v, const double *lb, const double *ub,
                            const double *gout, double *gv, double *glb, double *gub, int mem);

/* ---------------------------------------------------------------------- */
/* The fixed-point adjoint of the ADMM loop on the device, box rows and     */
/* cone rows alike (new).  At a fixed point (w, y, z) of     */
/* the iteration the gradient of a loss on w is the limit of                 */
/*     a <- dl/ds + J_step^T a,   a = (a_w, a_y, a_z) from 0,                */
/* J_step the Jacobian of one ADMM step.  With tt = zs + ys / rho (the       */
/* projection's argument at the fixed point) and P^T the operator of         */
/* pdplqr_admm_project_vjp at tt, one iteration is                            */
/*     b_w = gws + a_w;  q = a_z - rho o a_y;  b_vr = rho o a_y + P^T q       */
/*     (dh, dg) = pdplqr_adjoint_rows' (gh, gg) for gws := alpha b_w,         */
/*                gvs := alpha b_vr (one solve on the cached factor)         */
/*     a_w <- (1 - alpha) b_w - sigma dh                                      */
/*     a_y <- a_y + P^T q / rho - dg / rho                                    */
/*     a_z <- (1 - alpha) b_vr + dg                                           */
/* Every check_every iterations (and at max_iter) a problem whose max-norm   */
/* change of a is <= tol times the max-norm of a is frozen; the loop ends    */
/* when none is active (one small device-to-host read per test) or at        */
/* max_iter.  One last adjoint pass at the final cotangents writes gE, gc,   */
/* gH, gh, gx, gD in pdplqr_adjoint_rows' layouts; glb, gub [batch][ny]      */
/* follow pdplqr_admm_project_vjp with gout := q (box rows: q where          */
/* tt <= lb / tt >= ub; cone rows: glb = q - P^T q, gub = 0).  Any output    */
/* may be NULL.                                                               */
/* On entry the preconditions of pdplqr_adjoint_rows hold: the handle last   */
/* factored the x-update at (w, y, z) with `rho`, and ws is the w~ its       */
/* forward returned.  ys, zs, lb, ub, rho [batch][ny]; gws [batch][N*s+n];   */
/* sigma, alpha the solve's.  Limits: those of pdplqr_adjoint_rows (SERIAL,  */
/* keep_factors = 1, one device, nx + nu <= 64, rows within the rows         */
/* kernel's LDS tile) and at least one constraint row, else                  */
/* PDPLQR_ERR_UNSUPPORTED; PDPLQR_ERR_STATE before backward;                 */
/* PDPLQR_ERR_INVALID for null inputs, bad settings (0 < alpha < 2, sigma,   */
/* tol >= 0, max_iter, check_every >= 1) or rho not constant within a cone.  */
/* A refused call writes nothing.  The handle's factor, record and lp are    */
/* unchanged.                                                                 */
/* ---------------------------------------------------------------------- */
int pdplqr_admm_adjoint_fixed_point(pdplqr_handle h, const double *ws, const double *ys, const double *zs,
                                    const double *lb, const double *ub, const double *rho, const double *gws,
                                    double sigma, double alpha, double tol, int32_t max_iter, int32_t check_every,
                                    double *gE, double *gc, double *gH, double *gh, double *gx, double *gD,
                                    double *glb, double *gub, int mem);

/* The last pdplqr_admm_adjoint_fixed_point, host arrays, any may be NULL: iters [batch]    */
/* (the iteration of the problem's last test), converged [batch], resid [batch][2]: the     */
/* max-norm change and the max-norm of a at that test.  PDPLQR_ERR_STATE before any call.   */
int pdplqr_admm_adjoint_fixed_point_info(pdplqr_handle h, int32_t *iters, int32_t *converged, double *resid);

/* Device info helpers (for hosts that do not link HIP). */
int pdplqr_device_count(int32_t *count);

#ifdef __cplusplus
}
#endif

#endif /* PDPLQR_H */
