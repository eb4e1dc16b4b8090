// adjoint.hpp -- the adjoint solve's gradient pass (kernels_adjoint.hip) and
// its per-handle scratch (adjoint.hip).
#pragma once
#include "internal.hpp"

namespace pdplqr {

struct AdjointArgs {
    Shape sh;
    const double *ws, *v;     // primal and adjoint solutions [b][N*s + n]
    const double *Lc;         // factor cache [b][N*ps + pn]
    const double *lpc, *lpa;  // lp_k = [lu'; p_k] of the primal and of the adjoint solve
    double *gE, *gc, *gH, *gh, *gx;  // outputs in the boundary layouts; NULL = not wanted
    int ts = 0;               // stages per block (set by the launcher)
};

// writes the requested gradients (device pointers)
int launch_adjoint_grad(const AdjointArgs &a, hipStream_t st);
// lu'_k of the rollout record KD to buf [b][N][m], or back
int launch_adjoint_lu(const Shape &sh, double *KD, double *buf, bool restore, hipStream_t st);
size_t adjoint_lds_bytes(const Shape &sh, int ts);
int adjoint_tile(const Shape &sh);

// pdplqr_adjoint_parallel (adjoint_parallel.hip, kernels_adjoint_parallel.hip): the
// per-stage costates of both solves on a PARALLEL handle, one wave per
// (problem, device segment), and the gradient pass reading them
struct SegCostateArgs {
    Shape sh;
    int S;                               // device segments per problem
    const int32_t *seg_start, *seg_len;  // [S]
    const double *E, *FR;                // model, rollout records [b][N][s m + m]
    const double *Lc;                    // the segment-local P_k, packed lower n x n at stage offset k ps
    const double *lpc, *lpa;             // lp_k = [lu'; p_k] of the primal and of the adjoint solve
    const double *ws, *v;                // primal and adjoint solutions [b][N*s + n]
    const double *sufp, *sufa;           // suffix scans of both solves [b][S][es]
    double *lam, *mu;                    // out: costates [b][N + 1][n] (entry 0: segment 0's lambda_0, mu_0)
    int need_lam;                        // 0: lam is not stored
};
int launch_seg_costate(const SegCostateArgs &a, hipStream_t st);
struct AdjointCostateArgs {
    Shape sh;
    const double *ws, *v;     // primal and adjoint solutions [b][N*s + n]
    const double *lam, *mu;   // costates [b][N + 1][n]
    double *gE, *gc, *gH, *gh, *gx;  // outputs in the boundary layouts; NULL = not wanted
    int ts = 0;               // stages per block (set by the launcher)
};
int launch_adjoint_grad_costate(const AdjointCostateArgs &a, hipStream_t st);

// pdplqr_adjoint_rows: the gradients of the constraint rows (kernels_adjoint_rows.hip)
struct AdjointRowsArgs {
    Shape sh;
    const double *ws, *v;             // primal and adjoint solutions [b][N*s + n]
    const double *D, *rho, *g, *gvs;  // [b][ndD], [b][ny] each; gvs NULL = zero
    const int32_t *d_off, *y_off;     // the handle's device tables (N + 2 entries)
    double *gD, *gg, *grho;           // outputs; NULL = not wanted
    int ts = 0, max_rows = 0;         // stages per block and the most rows of one tile (adjoint_rows_plan)
    int lanes = 1;                    // lanes sharing one row's products, a power of two (adjoint_rows_plan)
    int vecD = 0, vecY = 0;           // 16-byte stores allowed for gD / for gg and grho (set by the launcher)
};
// tile of the rows kernel from the host tables; false: one stage's rows do not fit the LDS tile
bool adjoint_rows_plan(const Shape &sh, const int32_t *y_off_h, const int32_t *d_off_h, AdjointRowsArgs &a);
int launch_adjoint_rows(const AdjointRowsArgs &a, const int32_t *y_off_h, const int32_t *d_off_h, hipStream_t st);
// rhs = gws + D^T gvs (rhs may alias gws)
int launch_adjoint_rhs(const Shape &sh, const double *gws, const double *gvs, const double *D, const int32_t *d_off,
                       const int32_t *y_off, double *rhs, hipStream_t st);

size_t adjoint_rows_lds_bytes(const Shape &sh, int ts, int max_rows);  // the rows kernels' tile

// pdplqr_admm_adjoint: the refinement step and the row gradients (kernels_asadj.hip)
struct AsadjStepArgs {
    Shape sh;
    const double *D, *act;         // act [b][ny]: != 0 on the active rows (the polish's rho)
    const int32_t *d_off, *y_off;
    int max_nc;
    double delta;
    const double *v, *gt;          // the new adjoint iterate and g~, [b][N*s + n]
    double *eta;                   // [b][ny], stepped in place on the active rows
    double *rhs;                   // out: g~ - delta v + D^T eta (NULL: not wanted, the last step)
    // the last step (resid non-NULL): the measures and the status of every problem
    const double *vprev;           // the iterate before (NULL: zero)
    double *resid;                 // [b][2]
    int32_t *stat;                 // [b] PDPLQR_ADMM_ADJOINT_*
    const int32_t *pstat, *fstat;  // the polish outcome and the factorisation status
};
int launch_asadj_step(const AsadjStepArgs &a, hipStream_t st);

struct AsadjRowsArgs {
    Shape sh;
    const double *ws, *v;                  // w~ and the adjoint solution [b][N*s + n]
    const double *y, *eta, *gvs;           // [b][ny]; gvs NULL = zero
    const double *act, *bt, *lb;           // the classification: active flag, target, lower bound
    const int32_t *d_off, *y_off;
    double *gD, *glb, *gub;                // outputs; NULL = not wanted
    int ts = 0, max_rows = 0;              // adjoint_rows_plan's tile
    int vecD = 0, vecY = 0;                // 16-byte stores allowed (set by the launcher)
};
int launch_asadj_rows(const AsadjRowsArgs &a, const int32_t *y_off_h, const int32_t *d_off_h, hipStream_t st);

// pdplqr_admm_adjoint_fixed_point: one iteration's elementwise work (kernels_fpadj.hip)
struct FpadjArgs {
    Shape sh;
    const double *D;
    const double *ys, *zs, *lb, *ub, *rho;  // the fixed point and the call's vectors, [b][ny]
    const double *gws;                      // dl/dw [b][N*s + n]
    const int32_t *d_off, *y_off;
    const int32_t *c_off, *c_row, *c_dim;   // the handle's cone table (c_off NULL: no cones)
    int max_nc;
    double alpha, sigma, tol;
    const double *v;            // this iteration's adjoint solution (NULL: no update, the cotangents only)
    double *aw, *ay, *az;       // the state, stepped in place
    double *jq;                 // [b][ny] P^T q at the state (read by the next update)
    double *rhs;                // out: the next solve's right-hand side alpha b_w + D^T (alpha b_vr)
    int test, it;               // a test iteration: the measures, done / conv / iters / active
    int32_t *done, *conv, *iters, *active;
    double *resid;              // [b][2]: the change and the norm of the problem's last test
    double *gvs, *glb, *gub;    // the final pass (NULL: not wanted): alpha b_vr and the bounds' gradients
};
int launch_fpadj_step(const FpadjArgs &a, hipStream_t st);

}  // namespace pdplqr
