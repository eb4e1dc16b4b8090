// admm.hpp -- the ADMM outer loop's device arguments and termination /
// adaptive-rho decision, shared by the stand-alone update kernel (admm.hip)
// and the update fused into the streamed backward (kernels_nofact.hip).
#pragma once
#include "internal.hpp"

namespace pdplqr {

struct AdmmArgs {
    Shape sh;
    const double *D, *hv, *wt, *lb, *ub, *rho, *irho;
    double *w, *y, *z, *hw, *gw;
    const int32_t *d_off, *y_off;
    int32_t *done, *iters, *conv, *active;
    double *prim, *dual, *rscale;
    double alpha, sigma, eps_abs, eps_rel, rho_tol;
    int max_nc, it, adaptive;
    int no_penalty = 0;  // fused next-update h~ without the penalty term (KKT: rho enters through g)
    int uni = 0;         // > 0: every stage k < N has exactly uni rows, the terminal none (offsets by arithmetic)
};

// Termination test of iteration a.it for problem b from the five maxima
// (r_prim, |Dw|, |z|, r_dual, |D^T y|), then OSQP's rho estimate when the
// test fails (admm.hip header).  One thread per problem.
// act > 0: some row's z sits at one of its bounds (an active constraint).
__device__ __forceinline__ void admm_decide(const AdmmArgs &a, int b, double rp, double dwm, double zm, double rd,
                                            double dty, double act) {
    a.iters[b] = a.it;
    a.prim[b] = rp;
    a.dual[b] = rd;
    double f = 1.0;
    if (rp <= a.eps_abs + a.eps_rel * fmax(dwm, zm) && rd <= a.eps_abs + a.eps_rel * dty) {
        a.done[b] = 1;
        a.conv[b] = 1;
    } else {
        atomicAdd(a.active, 1);
        // no rescale while no row is active (y is rounding noise there and the
        // dual normalisation undefined -- the estimate would collapse to ~1e-14
        // and pin rho at its lower clamp) or |D^T y| vanishes (OSQP's 1e-30 guard)
        if (a.adaptive && act > 0.0 && dty > 1e-30) {
            // OSQP's compute_rho_estimate: the ratio of the normalised
            // residuals, with its division guard 1e-30
            const double pn = rp / (fmax(dwm, zm) + 1e-30), dn = rd / (dty + 1e-30);
            const double e = sqrt(pn / (dn + 1e-30));
            if (e > a.rho_tol || e < 1.0 / a.rho_tol) {
                f = e;
                atomicOr(a.active + 1, 1);
            }
        }
    }
    a.rscale[b] = f;
}

// Second-order cone rows (kernels_cone.hip).  The
// handle's cone table on the device: the cones of stage k are entries
// c_off[k] .. c_off[k + 1] - 1 of (c_row, c_dim), in row order; cone i covers
// rows [c_row[i], c_row[i] + c_dim[i]) of its stage.
struct ConeArgs {
    AdmmArgs a;
    const int32_t *c_off, *c_row, *c_dim;
};
// k_admm_update with the cone projection on the cone rows (lps 16 / 32 / 64)
int launch_admm_update_cone(const ConeArgs &c, int lps, bool fuse, bool check, hipStream_t st);
// out = the projection of v onto the mixed set, all [batch][ny] (c_off null: every row a box row)
int launch_cone_project(const Shape &sh, const int32_t *y_off, const int32_t *c_off, const int32_t *c_row,
                        const int32_t *c_dim, const double *v, const double *lb, const double *ub, double *out,
                        hipStream_t st);
// gv = J^T gout, J the Jacobian of launch_cone_project at v; glb, gub the cotangents of the
// bounds (any of the three NULL: not wanted)
int launch_cone_project_vjp(const Shape &sh, const int32_t *y_off, const int32_t *c_off, const int32_t *c_row,
                            const int32_t *c_dim, const double *v, const double *lb, const double *ub,
                            const double *gout, double *gv, double *glb, double *gub, hipStream_t st);
// flag[0] += cones whose rho is not constant, flag[1] += cone rows whose e_lb is
// not finite; c_y0[i] is the first row of cone i within a problem's ny rows
int launch_cone_validate(int batch, int ny, int num_cones, const int32_t *c_y0, const int32_t *c_dim, const double *lb,
                         const double *rho, int32_t *flag, hipStream_t st);

// Infeasibility certificates (kernels_infeas.hip).  The
// vectors tested are y - yp and w - wp (the loop: differences of consecutive
// iterates) or y and w themselves (yp, wp null: the stand-alone evaluator).
struct InfeasArgs {
    Shape sh;
    const double *E, *c, *H, *hv, *D, *x0, *lb, *ub;
    const double *y, *yp, *w, *wp;
    const int32_t *d_off, *y_off;
    int uni, max_nc;
    double eps_p, eps_d;
    double *meas;      // [b][8]: |dy|, max|g|, support - beta, infinite-bound flag; |dw|, max|H dw|, h^T dw, violation
    int32_t *verdict;  // [b] bit 0 primal, bit 1 dual (nullable)
    // the loop (done non-null): problems with done[b] != 0 are skipped, a certified one is frozen
    int32_t *done, *status, *active;
    double *rscale;
};
bool infeas_shape_supported(const Shape &sh);  // n + m <= 64
int launch_infeas_primal(const InfeasArgs &a, hipStream_t st);
int launch_infeas_dual(const InfeasArgs &a, hipStream_t st);
int launch_infeas_snapshot(const Shape &sh, const int32_t *done, const double *y, const double *w, double *yp,
                           double *wp, hipStream_t st);
int launch_infeas_delta(long long total, long long per, const int32_t *status, const double *cur, const double *prev,
                        double *out, hipStream_t st);

// The polish and the KKT measures (kernels_polish.hip).
// measures of (w, y) into meas[b * mstride + 0..3]: row residual, dynamics
// residual, reduced gradient, objective
struct KktArgs {
    Shape sh;
    const double *E, *c, *H, *hv, *D, *x0, *lb, *ub, *w, *y;
    const int32_t *d_off, *y_off;
    int uni, max_nc;
    double *meas;
    int mstride;
};
struct PolishArgs {
    Shape sh;
    const double *D, *lb, *ub;
    const double *y, *z;           // the ADMM iterate (classify)
    const int32_t *d_off, *y_off;
    int uni, max_nc;
    double delta;
    double *rho_p, *irho_p, *bt;   // [b][ny] the polishing x-update's rho, inv_rho and row targets
    double *wp, *yp, *vp;          // the polish iterate (w, y) and v = D w
    int32_t *nact;                 // [b] rows guessed active
};
int launch_polish_classify(const PolishArgs &a, hipStream_t st);
int launch_polish_ystep(const PolishArgs &a, hipStream_t st);
int launch_kkt_residual(const KktArgs &a, hipStream_t st);  // two launches: the recursion, the stage-local half
int launch_polish_accept(int batch, const int32_t *conv, const double *meas, const int32_t *fst1, int S1,
                         const int32_t *fst2, int32_t *pstat, hipStream_t st);
int launch_polish_write(const Shape &sh, const int32_t *pstat, const double *wp, const double *yp, const double *vp,
                        const double *lb, const double *ub, double *w, double *y, double *z, hipStream_t st);

// What pdplqr_admm_adjoint (adjoint.hip) reads of the last admm_solve: the
// returned point, the call's vectors and the polish classification.
struct AdmmAdjointView {
    const double *w, *y, *x0, *lb;
    const double *prho, *pirho, *pb;  // 1/delta | 0, delta | 0 and the target of every row
    const int32_t *pstat;             // [b] PDPLQR_POLISH_*
};
// 0: filled; 1: no admm_solve has run; 2: the last one ran without polish
int admm_adjoint_view(pdplqr_handle h, AdmmAdjointView &v);

// Fused ADMM update + backward_without_factorization (kernels_nofact.hip):
// PDPLQR_ERR_UNSUPPORTED when the shape / constraint layout is not covered.
int launch_nofact_admm(const RiccatiArgs &r, const AdmmArgs &a, bool check, hipStream_t st);

// KKT (Riccati-ordered, C5 row layout): the rollout with the ADMM update of the
// iteration in the same pass (kkt_riccati.hip); ERR_UNSUPPORTED otherwise
int launch_kkt_ric_forward_admm(const Shape &sh, const double *E, const double *c, const double *rec,
                                const double *x0, double *x0acc, double rho_dyn, const AdmmArgs &q, bool fuse,
                                bool check, hipStream_t st);
int kkt_forward_admm(pdplqr_handle h, const double *x0, const AdmmArgs &q, bool fuse, bool check);

}  // namespace pdplqr
