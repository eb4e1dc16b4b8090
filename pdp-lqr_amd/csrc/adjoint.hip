// adjoint.hip -- pdplqr_adjoint: gradients of a scalar loss on the solution of
// the batched serial LQ solve with respect to E, c, H, h and x0 (new: the
// reference has no such call).
//
// The adjoint of a KKT solve is one more solve with the same matrix: with
// g = dl/dw*, the problem with h~ := g, c := 0, x0 := 0 and the handle's E, H~
// has the solution v = -K^{-1} [g; 0].  The factor is cached (keep_factors = 1),
// so v costs one backward_without_factorization and one forward on substituted
// pointers; one streamed pass (kernels_adjoint.hip) then forms the costates of
// both solves from the cached Lxx_k and writes the gradients.
//
// The handle is unchanged for the caller: the nofact kernels write lp_k to
// `lpc` and lu'_k into the rollout record, so the adjoint runs with an lpc of
// its own and saves / restores the record's lu' column (m doubles per stage).
#include <string>

#include "adjoint.hpp"
#include "admm.hpp"
#include "solvers.hpp"

namespace pdplqr {

struct AdjointState {
    double *zc = nullptr, *zx0 = nullptr;  // c = 0, x0 = 0
    double *rhs = nullptr;                 // dl/dw in the hw layout
    double *v = nullptr;                   // adjoint solution
    double *lpa = nullptr;                 // adjoint lp_k = [lu'; p^_k]
    double *lus = nullptr;                 // the primal lu'_k, [b][N][m]
    // host outputs' staging (gE, gc, gH, gh, gx, gD, gg, grho)
    double *out[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    double *rho = nullptr, *gvs = nullptr;  // host rho / gvs staging (pdplqr_adjoint_rows)
    // pdplqr_admm_adjoint (allocated by its first call)
    double *gt = nullptr, *eta = nullptr;   // g~ = gws + D^T gvs; the multiplier of the active rows
    double *wt = nullptr, *v2 = nullptr;    // w~ of the x-update at the solution; the other adjoint iterate
    double *resid = nullptr;                // [b][2]
    int32_t *stat = nullptr;                // [b] PDPLQR_ADMM_ADJOINT_*
    bool as_ran = false;                    // an admm_adjoint got as far as its launches
    // pdplqr_admm_adjoint_fixed_point (allocated by its first call)
    double *fa_w = nullptr, *fa_y = nullptr, *fa_z = nullptr;  // the state a
    double *fjq = nullptr, *fgvs = nullptr;  // P^T q; alpha b_vr of the final pass
    double *fresid = nullptr;                // [b][2]
    int32_t *fint = nullptr;                 // [4 + 3 b]: active, the validation's two counts | done | conv | iters
    int32_t *factive_h = nullptr;            // pinned copy of fint[0..2]
    double *fin[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // host ys, zs, lb, ub, rho, gws staged
    bool fp_ran = false;                     // an admm_adjoint_fixed_point got as far as its loop
};

void adjoint_release(pdplqr_handle h) {
    if (h->adj && h->adj->factive_h) (void)hipHostFree(h->adj->factive_h);
    delete h->adj;
    h->adj = nullptr;
}

static int adjoint_alloc(pdplqr_handle h) {
    if (h->adj) return PDPLQR_OK;
    const Shape &sh = h->sh;
    const long long B = sh.batch;
    AdjointState s;
    int rc;
    if ((rc = dev_alloc(h, &s.zc, B * sh.perc)) || (rc = dev_alloc(h, &s.zx0, B * sh.n)) ||
        (rc = dev_alloc(h, &s.rhs, B * sh.perh)) || (rc = dev_alloc(h, &s.v, B * sh.perh)) ||
        (rc = dev_alloc(h, &s.lpa, B * sh.perh)) || (rc = dev_alloc(h, &s.lus, B * sh.N * sh.m)))
        return rc;
    PDPLQR_HIP_TRY(hipMemsetAsync(s.zc, 0, (size_t)(B * sh.perc) * sizeof(double), h->stream));
    PDPLQR_HIP_TRY(hipMemsetAsync(s.zx0, 0, (size_t)(B * sh.n) * sizeof(double), h->stream));
    h->adj = new AdjointState(s);
    return PDPLQR_OK;
}

// the rows kernel's pointers on a block adjoint_rows_plan laid out: the
// handle's rows and the adjoint solution in the scratch, the call's vectors
static void adjoint_rows_args(pdplqr_handle h, AdjointRowsArgs &ra, const double *ws, const double *rho,
                              const double *gvs, double *gD, double *gg, double *grho) {
    ra.ws = ws;
    ra.v = h->adj->v;
    ra.D = h->D;
    ra.rho = rho;
    ra.g = h->gw;
    ra.gvs = gvs;
    ra.d_off = h->d_off;
    ra.y_off = h->y_off;
    ra.gD = gD;
    ra.gg = gg;
    ra.grho = grho;
}

// the gradient pass's arguments: the cached factor, both solves' lp and the adjoint solution
static AdjointArgs adjoint_args(pdplqr_handle h, const double *ws, double *gE, double *gc, double *gH, double *gh,
                                double *gx) {
    AdjointArgs g;
    g.sh = h->sh;
    g.ws = ws;
    g.v = h->adj->v;
    g.Lc = h->Lc;
    g.lpc = h->lpc;
    g.lpa = h->adj->lpa;
    g.gE = gE;
    g.gc = gc;
    g.gH = gH;
    g.gh = gh;
    g.gx = gx;
    return g;
}

// the adjoint solve on the cached factor: h~ := rhs, c := 0, x0 := 0, lp into the
// scratch's own lpa; the caller saves and restores the record's lu'
static int adjoint_solve(pdplqr_handle h, double *rhs, double *v) {
    AdjointState *s = h->adj;
    RiccatiArgs a = riccati_args(h);  // (xl_ws: null on these handles, n + m <= 64)
    a.c = s->zc;
    a.hw = rhs;
    a.lpc = s->lpa;
    const int rc = launch_riccati_backward_nofact(a, h->stream);
    return rc ? rc : launch_riccati_forward(h->sh, h->E, s->zc, h->KD, s->zx0, v, h->stream);
}

static int fail(int code, const char *msg) {
    set_error(msg);
    return code;
}

}  // namespace pdplqr

using namespace pdplqr;

// The body of pdplqr_adjoint and pdplqr_adjoint_rows (`what` names the call in
// messages).  The rows arguments (rho, gvs, gD, gg, grho) are all NULL for
// pdplqr_adjoint, whose handles have no rows.
static int adjoint_run(pdplqr_handle h, const char *what, const double *ws, const double *rho, const double *gws,
                       const double *gvs, double *const user[8], int mem) {
    if (int brc = bind_device(h)) return brc;
    const Shape &sh = h->sh;
    AdjointRowsArgs ra;
    if (sh.ny > 0 && !adjoint_rows_plan(sh, h->y_off_h.data(), h->d_off_h.data(), ra))
        return fail(PDPLQR_ERR_UNSUPPORTED,
                    (std::string(what) + ": the constraint rows of one stage exceed the kernel's LDS tile").c_str());
    int rc = adjoint_alloc(h);
    if (rc) return rc;
    AdjointState *s = h->adj;
    const long long B = sh.batch;
    const bool dev = mem == PDPLQR_MEM_DEVICE;
    hipStream_t st = h->stream;
    const hipMemcpyKind in = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;

    // inputs: ws is read in place on the device (host: staged as forward's output is);
    // the right-hand side is formed in the scratch buffer (a copy of dl/dw, or k_adjoint_rhs
    // reading it), so the recursion's kernel choice never depends on the caller's alignment
    const double *dws, *drho = rho, *dgvs = gvs;
    if ((rc = stage_in(h, ws, h->st_ws, B * sh.perh, mem, &dws))) return rc;
    if (!dev && sh.ny > 0) {
        if (!s->rho && (rc = dev_alloc(h, &s->rho, B * sh.ny))) return rc;
        if ((rc = stage_in(h, rho, s->rho, B * sh.ny, mem, &drho))) return rc;
        if (gvs) {
            if (!s->gvs && (rc = dev_alloc(h, &s->gvs, B * sh.ny))) return rc;
            if ((rc = stage_in(h, gvs, s->gvs, B * sh.ny, mem, &dgvs))) return rc;
        }
    }
    // the adjoint solve's right-hand side: dl/dw (+ D^T dl/d(D w))
    if (sh.ny > 0 && gvs && dev) {
        if ((rc = launch_adjoint_rhs(sh, gws, dgvs, h->D, h->d_off, h->y_off, s->rhs, st))) return rc;
    } else {
        PDPLQR_HIP_TRY(hipMemcpyAsync(s->rhs, gws, (size_t)(B * sh.perh) * sizeof(double), in, st));
        if (sh.ny > 0 && gvs && (rc = launch_adjoint_rhs(sh, s->rhs, dgvs, h->D, h->d_off, h->y_off, s->rhs, st)))
            return rc;
    }
    // outputs: the caller's device pointers, or staging allocated on first use
    const long long cnt[8] = {B * sh.perE, B * sh.perc, B * sh.perH, B * sh.perh, B * sh.n,
                              B * sh.ndD,  B * sh.ny,   B * sh.ny};
    double *out[8];
    for (int i = 0; i < 8; ++i) {
        out[i] = cnt[i] > 0 ? user[i] : nullptr;
        if (out[i] && !dev) {
            if (!s->out[i] && (rc = dev_alloc(h, &s->out[i], cnt[i]))) return rc;
            out[i] = s->out[i];
        }
    }

    // v: backward_without_factorization + forward of (E, H~) with h~ := g, c := 0, x0 := 0
    if ((rc = launch_adjoint_lu(sh, h->KD, s->lus, false, st))) return rc;
    rc = adjoint_solve(h, s->rhs, s->v);
    // the record's lu' goes back whatever the launches returned
    const int rc2 = launch_adjoint_lu(sh, h->KD, s->lus, true, st);
    if (rc || rc2) return rc ? rc : rc2;

    if ((rc = launch_adjoint_grad(adjoint_args(h, dws, out[0], out[1], out[2], out[3], out[4]), st))) return rc;
    if (out[5] || out[6] || out[7]) {
        adjoint_rows_args(h, ra, dws, drho, dgvs, out[5], out[6], out[7]);
        if ((rc = launch_adjoint_rows(ra, h->y_off_h.data(), h->d_off_h.data(), st))) return rc;
    }

    if (!dev) {
        for (int i = 0; i < 8; ++i)
            if (out[i])
                PDPLQR_HIP_TRY(hipMemcpyAsync(user[i], out[i], (size_t)cnt[i] * sizeof(double), hipMemcpyDeviceToHost, st));
        PDPLQR_HIP_TRY(hipStreamSynchronize(st));
    }
    h->host_staged = false;
    return PDPLQR_OK;
}

extern "C" int pdplqr_adjoint(pdplqr_handle h, const double *ws, const double *gws, double *gE, double *gc, double *gH,
                              double *gh, double *gx, int mem) {
    if (!h) return fail(PDPLQR_ERR_INVALID, "adjoint: null handle");
    if (!ws || !gws) return fail(PDPLQR_ERR_INVALID, "adjoint: null ws/gws");
    if (h->md) return fail(PDPLQR_ERR_UNSUPPORTED, "adjoint: multi-device handles are not supported");
    if (h->cfg.solver != PDPLQR_SOLVER_SERIAL)
        return fail(PDPLQR_ERR_UNSUPPORTED, "adjoint needs a SERIAL handle (PARALLEL and KKT are not supported)");
    if (h->sh.ny > 0) return fail(PDPLQR_ERR_UNSUPPORTED, "adjoint: constrained stages (ncs > 0) are not supported");
    if (h->sh.s > 64) return fail(PDPLQR_ERR_UNSUPPORTED, "adjoint: n + m > 64 is not supported");
    if (!h->cfg.keep_factors || !h->Lc || !h->lpc)
        return fail(PDPLQR_ERR_STATE, "adjoint requires keep_factors = 1");
    if (!h->factored) return fail(PDPLQR_ERR_STATE, "adjoint before backward");
    if (h->rec_gain) return fail(PDPLQR_ERR_STATE, "adjoint: the rollout record is not in factor form");
    double *const user[8] = {gE, gc, gH, gh, gx, nullptr, nullptr, nullptr};
    return adjoint_run(h, "adjoint", ws, nullptr, gws, nullptr, user, mem);
}

// The same with constraint rows: the handle last factored the penalised
// x-update H~ = H + sigma I + D^T R D, h~ = h - sigma w - D^T R g (R = diag(rho),
// g = h->gw from update_problem_data).  The penalty is inside the cached factor,
// so the adjoint solve is the one above with the right-hand side gws + D^T gvs;
// k_adjoint_rows (kernels_adjoint_rows.hip) adds the gradients of D, g and rho.
extern "C" int pdplqr_adjoint_rows(pdplqr_handle h, const double *ws, const double *rho, const double *gws,
                                   const double *gvs, double *gE, double *gc, double *gH, double *gh, double *gx,
                                   double *gD, double *gg, double *grho, int mem) {
    if (!h) return fail(PDPLQR_ERR_INVALID, "adjoint_rows: null handle");
    if (!ws || !gws) return fail(PDPLQR_ERR_INVALID, "adjoint_rows: null ws/gws");
    if (h->md) return fail(PDPLQR_ERR_UNSUPPORTED, "adjoint_rows: multi-device handles are not supported");
    if (h->cfg.solver != PDPLQR_SOLVER_SERIAL)
        return fail(PDPLQR_ERR_UNSUPPORTED, "adjoint_rows needs a SERIAL handle (PARALLEL and KKT are not supported)");
    if (h->sh.s > 64) return fail(PDPLQR_ERR_UNSUPPORTED, "adjoint_rows: n + m > 64 is not supported");
    if (!h->cfg.keep_factors || !h->Lc || !h->lpc)
        return fail(PDPLQR_ERR_STATE, "adjoint_rows requires keep_factors = 1");
    if (!h->factored) return fail(PDPLQR_ERR_STATE, "adjoint_rows before backward");
    if (h->rec_gain) return fail(PDPLQR_ERR_STATE, "adjoint_rows: the rollout record is not in factor form");
    if (h->sh.ny > 0 && !rho) return fail(PDPLQR_ERR_INVALID, "adjoint_rows: null rho with constraint rows");
    double *const user[8] = {gE, gc, gH, gh, gx, gD, gg, grho};
    return adjoint_run(h, "adjoint_rows", ws, rho, gws, gvs, user, mem);
}

// Internal diagnostic (not part of include/pdplqr.h; scripts/adjoint_rows_bench.py):
// the rows kernel alone, on the adjoint solution the last pdplqr_adjoint_rows
// left in the scratch.  Device pointers; gvs may be NULL.
extern "C" int pdplqr_debug_adjoint_rows(pdplqr_handle h, const double *ws, const double *rho, const double *gvs,
                                         double *gD, double *gg, double *grho) {
    if (!h || !ws || !rho || !h->adj || h->sh.ny == 0)
        return fail(PDPLQR_ERR_STATE, "debug_adjoint_rows before adjoint_rows");
    if (int brc = bind_device(h)) return brc;
    AdjointRowsArgs ra;
    if (!adjoint_rows_plan(h->sh, h->y_off_h.data(), h->d_off_h.data(), ra))
        return fail(PDPLQR_ERR_UNSUPPORTED, "debug_adjoint_rows: rows exceed the LDS tile");
    adjoint_rows_args(h, ra, ws, rho, gvs, gD, gg, grho);
    return launch_adjoint_rows(ra, h->y_off_h.data(), h->d_off_h.data(), h->stream);
}

// Internal diagnostic (not part of include/pdplqr.h; scripts/adjoint_bench.py):
// the gradient pass alone, on the adjoint solution the last pdplqr_adjoint
// left in the scratch.  Device pointers.
extern "C" int pdplqr_debug_adjoint_grad(pdplqr_handle h, const double *ws, double *gE, double *gc, double *gH,
                                         double *gh, double *gx) {
    if (!h || !ws || !h->adj || !h->Lc || !h->lpc) return fail(PDPLQR_ERR_STATE, "debug_adjoint_grad before adjoint");
    if (int brc = bind_device(h)) return brc;
    return launch_adjoint_grad(adjoint_args(h, ws, gE, gc, gH, gh, gx), h->stream);
}

// The gradient of the box-constrained optimum of the last admm_solve on the
// active set its polish guessed (include/pdplqr.h):
// the polishing x-update at the returned point, then refine_iter + 1 adjoint
// solves on its factor with k_asadj_step between them, the gradient pass of
// pdplqr_adjoint and k_asadj_rows.  Nothing here waits for the device (device
// buffers).
extern "C" int pdplqr_admm_adjoint(pdplqr_handle h, const double *gws, const double *gvs, double *gE, double *gc,
                                   double *gH, double *gh, double *gx, double *gD, double *glb, double *gub,
                                   int mem) {
    if (!h) return fail(PDPLQR_ERR_INVALID, "admm_adjoint: null handle");
    if (!gws) return fail(PDPLQR_ERR_INVALID, "admm_adjoint: null gws");
    if (h->md) return fail(PDPLQR_ERR_UNSUPPORTED, "admm_adjoint: multi-device handles are not supported");
    if (h->cfg.solver != PDPLQR_SOLVER_SERIAL)
        return fail(PDPLQR_ERR_UNSUPPORTED, "admm_adjoint needs a SERIAL handle (PARALLEL and KKT are not supported)");
    const Shape &sh = h->sh;
    if (sh.s > 64) return fail(PDPLQR_ERR_UNSUPPORTED, "admm_adjoint: n + m > 64 is not supported");
    if (h->num_cones > 0)
        return fail(PDPLQR_ERR_UNSUPPORTED,
                    "admm_adjoint: the active-set adjoint is a statement about box rows; the handle has cones");
    if (sh.ny == 0)
        return fail(PDPLQR_ERR_UNSUPPORTED, "admm_adjoint: the handle has no constraint rows (use pdplqr_adjoint)");
    if (!h->cfg.keep_factors || !h->Lc || !h->lpc)
        return fail(PDPLQR_ERR_STATE, "admm_adjoint requires keep_factors = 1");
    AdmmAdjointView V;
    const int vrc = h->model_set ? admm_adjoint_view(h, V) : 1;
    if (vrc == 1) return fail(PDPLQR_ERR_STATE, "admm_adjoint before admm_solve");
    if (vrc) return fail(PDPLQR_ERR_STATE, "admm_adjoint: the last admm_solve did not run with polish on");
    if (int brc = bind_device(h)) return brc;
    AdjointRowsArgs plan;
    if (!adjoint_rows_plan(sh, h->y_off_h.data(), h->d_off_h.data(), plan))
        return fail(PDPLQR_ERR_UNSUPPORTED, "admm_adjoint: the constraint rows of one stage exceed the kernel's LDS tile");
    int rc = adjoint_alloc(h);
    if (rc) return rc;
    AdjointState *s = h->adj;
    const long long B = sh.batch;
    if (!s->gt && ((rc = dev_alloc(h, &s->gt, B * sh.perh)) || (rc = dev_alloc(h, &s->eta, B * sh.ny)) ||
                   (rc = dev_alloc(h, &s->wt, B * sh.perh)) || (rc = dev_alloc(h, &s->v2, B * sh.perh)) ||
                   (rc = dev_alloc(h, &s->resid, 2 * B)) || (rc = dev_alloc(h, &s->stat, B)))) {
        s->gt = nullptr;  // (what was allocated is freed with the handle)
        return rc;
    }
    const bool dev = mem == PDPLQR_MEM_DEVICE;
    hipStream_t st = h->stream;
    const hipMemcpyKind in = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const double delta = h->polish_delta;
    const int refine = h->polish_refine;

    // g~ = gws (+ D^T gvs), in the scratch: the recursion never reads the caller's buffer
    const double *dgvs = gvs;
    if (!dev && gvs) {
        if (!s->gvs && (rc = dev_alloc(h, &s->gvs, B * sh.ny))) return rc;
        if ((rc = stage_in(h, gvs, s->gvs, B * sh.ny, mem, &dgvs))) return rc;
    }
    if (gvs && dev) {
        if ((rc = launch_adjoint_rhs(sh, gws, dgvs, h->D, h->d_off, h->y_off, s->gt, st))) return rc;
    } else {
        PDPLQR_HIP_TRY(hipMemcpyAsync(s->gt, gws, (size_t)(B * sh.perh) * sizeof(double), in, st));
        if (gvs && (rc = launch_adjoint_rhs(sh, s->gt, dgvs, h->D, h->d_off, h->y_off, s->gt, st))) return rc;
    }
    // outputs: the caller's device pointers, or staging allocated on first use
    // (glb, gub share the staging of pdplqr_adjoint_rows's gg, grho: [b][ny] each)
    double *const user[8] = {gE, gc, gH, gh, gx, gD, glb, gub};
    const long long cnt[8] = {B * sh.perE, B * sh.perc, B * sh.perH, B * sh.perh, B * sh.n,
                              B * sh.ndD,  B * sh.ny,   B * sh.ny};
    double *out[8];
    for (int i = 0; i < 8; ++i) {
        out[i] = cnt[i] > 0 ? user[i] : nullptr;
        if (out[i] && !dev) {
            if (!s->out[i] && (rc = dev_alloc(h, &s->out[i], cnt[i]))) return rc;
            out[i] = s->out[i];
        }
    }

    // 1. the polishing x-update at the returned point: factor, lp and w~ belong together
    //    (y enters through g = b - inv_rho o y only, and inv_rho is 0 off the active rows)
    if ((rc = solver_update(h, V.w, V.y, V.pb, V.pirho, delta))) return rc;
    h->updated = true;
    if ((rc = solver_backward(h, V.prho))) return rc;
    h->factored = true;
    if ((rc = solver_forward(h, V.x0, s->wt))) return rc;
    s->as_ran = true;

    // 3. v^0 = 0, eta^0 = 0: the first right-hand side is g~ itself; iterate j + 1 goes to vb[(j + 1) & 1]
    PDPLQR_HIP_TRY(hipMemsetAsync(s->eta, 0, (size_t)(B * sh.ny) * sizeof(double), st));
    double *const vb[2] = {s->v2, s->v};
    AsadjStepArgs q{};
    q.sh = sh;
    q.D = h->D;
    q.act = V.prho;
    q.d_off = h->d_off;
    q.y_off = h->y_off;
    q.max_nc = h->max_nc;
    q.delta = delta;
    q.gt = s->gt;
    q.eta = s->eta;
    q.pstat = V.pstat;
    q.fstat = h->status;
    if ((rc = launch_adjoint_lu(sh, h->KD, s->lus, false, st))) return rc;
    for (int j = 0; j <= refine && !rc; ++j) {
        const bool last = j == refine;
        q.v = vb[(j + 1) & 1];
        q.vprev = j > 0 ? vb[j & 1] : nullptr;
        q.rhs = last ? nullptr : s->rhs;
        q.resid = last ? s->resid : nullptr;
        q.stat = last ? s->stat : nullptr;
        rc = adjoint_solve(h, j == 0 ? s->gt : s->rhs, vb[(j + 1) & 1]);
        if (!rc) rc = launch_asadj_step(q, st);
    }
    // the record's lu' goes back whatever the launches returned
    const int rc2 = launch_adjoint_lu(sh, h->KD, s->lus, true, st);
    if (rc || rc2) return rc ? rc : rc2;
    const double *v = vb[(refine + 1) & 1];

    // 4. the gradients: pdplqr_adjoint's pass on (w~, v), then the rows
    AdjointArgs g = adjoint_args(h, s->wt, out[0], out[1], out[2], out[3], out[4]);
    g.v = v;
    if ((rc = launch_adjoint_grad(g, st))) return rc;
    if (out[5] || out[6] || out[7]) {
        AsadjRowsArgs ra;
        ra.sh = sh;
        ra.ws = s->wt;
        ra.v = v;
        ra.y = V.y;
        ra.eta = s->eta;
        ra.gvs = dgvs;
        ra.act = V.prho;
        ra.bt = V.pb;
        ra.lb = V.lb;
        ra.d_off = h->d_off;
        ra.y_off = h->y_off;
        ra.gD = out[5];
        ra.glb = out[6];
        ra.gub = out[7];
        ra.ts = plan.ts;
        ra.max_rows = plan.max_rows;
        if ((rc = launch_asadj_rows(ra, h->y_off_h.data(), h->d_off_h.data(), st))) return rc;
    }

    if (!dev) {
        for (int i = 0; i < 8; ++i)
            if (out[i])
                PDPLQR_HIP_TRY(hipMemcpyAsync(user[i], out[i], (size_t)cnt[i] * sizeof(double), hipMemcpyDeviceToHost, st));
        PDPLQR_HIP_TRY(hipStreamSynchronize(st));
    }
    h->host_staged = false;
    return PDPLQR_OK;
}

extern "C" int pdplqr_admm_adjoint_info(pdplqr_handle h, int32_t *status, double *resid) {
    if (!h) return fail(PDPLQR_ERR_INVALID, "admm_adjoint_info: null handle");
    if (!h->adj || !h->adj->as_ran) return fail(PDPLQR_ERR_STATE, "admm_adjoint_info before admm_adjoint");
    if (int brc = bind_device(h)) return brc;
    PDPLQR_HIP_TRY(hipStreamSynchronize(h->stream));
    const size_t B = (size_t)h->sh.batch;
    if (status) PDPLQR_HIP_TRY(hipMemcpy(status, h->adj->stat, B * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (resid) PDPLQR_HIP_TRY(hipMemcpy(resid, h->adj->resid, 2 * B * sizeof(double), hipMemcpyDeviceToHost));
    return PDPLQR_OK;
}

// Internal diagnostics (not part of include/pdplqr.h; scripts/admm_adjoint_bench.py):
// the two kernels of pdplqr_admm_adjoint alone, on what its last call left in
// the scratch.  Device pointers.  The step is a middle one (eta stepped, rhs
// written); eta is scratch: the next admm_adjoint starts it from zero.
extern "C" int pdplqr_debug_asadj_step(pdplqr_handle h) {
    AdmmAdjointView V;
    if (!h || !h->adj || !h->adj->as_ran || admm_adjoint_view(h, V))
        return fail(PDPLQR_ERR_STATE, "debug_asadj_step before admm_adjoint");
    if (int brc = bind_device(h)) return brc;
    AdjointState *s = h->adj;
    AsadjStepArgs q{};
    q.sh = h->sh;
    q.D = h->D;
    q.act = V.prho;
    q.d_off = h->d_off;
    q.y_off = h->y_off;
    q.max_nc = h->max_nc;
    q.delta = h->polish_delta;
    q.v = s->v;
    q.gt = s->gt;
    q.eta = s->eta;
    q.rhs = s->rhs;
    return launch_asadj_step(q, h->stream);
}

extern "C" int pdplqr_debug_asadj_rows(pdplqr_handle h, double *gD, double *glb, double *gub) {
    AdmmAdjointView V;
    if (!h || !h->adj || !h->adj->as_ran || admm_adjoint_view(h, V))
        return fail(PDPLQR_ERR_STATE, "debug_asadj_rows before admm_adjoint");
    if (int brc = bind_device(h)) return brc;
    AdjointRowsArgs plan;
    if (!adjoint_rows_plan(h->sh, h->y_off_h.data(), h->d_off_h.data(), plan))
        return fail(PDPLQR_ERR_UNSUPPORTED, "debug_asadj_rows: rows exceed the LDS tile");
    AdjointState *s = h->adj;
    AsadjRowsArgs ra;
    ra.sh = h->sh;
    ra.ws = s->wt;
    ra.v = s->v;
    ra.y = V.y;
    ra.eta = s->eta;
    ra.gvs = nullptr;
    ra.act = V.prho;
    ra.bt = V.pb;
    ra.lb = V.lb;
    ra.d_off = h->d_off;
    ra.y_off = h->y_off;
    ra.gD = gD;
    ra.glb = glb;
    ra.gub = gub;
    ra.ts = plan.ts;
    ra.max_rows = plan.max_rows;
    return launch_asadj_rows(ra, h->y_off_h.data(), h->d_off_h.data(), h->stream);
}

// k_fpadj_step's arguments: the handle's rows and cone table, the scratch's state and
// flags, the call's six vectors in[] = (ys, zs, lb, ub, rho, gws) on the device
static FpadjArgs fpadj_args(pdplqr_handle h, const double *const in[6], double sigma, double alpha, double tol) {
    AdjointState *s = h->adj;
    const long long B = h->sh.batch;
    FpadjArgs q{};
    q.sh = h->sh;
    q.D = h->D;
    q.ys = in[0];
    q.zs = in[1];
    q.lb = in[2];
    q.ub = in[3];
    q.rho = in[4];
    q.gws = in[5];
    q.d_off = h->d_off;
    q.y_off = h->y_off;
    q.c_off = h->num_cones > 0 ? h->cone_off : nullptr;
    q.c_row = h->cone_row;
    q.c_dim = h->cone_dim;
    q.max_nc = h->max_nc;
    q.alpha = alpha;
    q.sigma = sigma;
    q.tol = tol;
    q.aw = s->fa_w;
    q.ay = s->fa_y;
    q.az = s->fa_z;
    q.jq = s->fjq;
    q.rhs = s->rhs;
    q.active = s->fint;
    q.done = s->fint + 4;
    q.conv = q.done + B;
    q.iters = q.conv + B;
    q.resid = s->fresid;
    return q;
}

// The fixed-point adjoint of the ADMM loop at its solution, box rows and cone
// rows alike (include/pdplqr.h): per iteration one
// adjoint solve on the cached factor and one k_fpadj_step, which forms the
// next right-hand side itself; every check_every iterations one 4-byte read
// tells whether any problem is still active.  The last solve's gradients are
// pdplqr_adjoint_rows' passes at the final cotangents.
extern "C" int pdplqr_admm_adjoint_fixed_point(pdplqr_handle h, const double *ws, const double *ys, const double *zs,
                                               const double *lb, const double *ub, const double *rho,
                                               const double *gws, double sigma, double alpha, double tol,
                                               int32_t max_iter, int32_t check_every, double *gE, double *gc,
                                               double *gH, double *gh, double *gx, double *gD, double *glb,
                                               double *gub, int mem) {
    const char *nm = "admm_adjoint_fixed_point";
    auto bad = [&](int code, const char *why) { return fail(code, (std::string(nm) + ": " + why).c_str()); };
    if (!h) return bad(PDPLQR_ERR_INVALID, "null handle");
    if (h->md) return bad(PDPLQR_ERR_UNSUPPORTED, "multi-device handles are not supported");
    if (h->cfg.solver != PDPLQR_SOLVER_SERIAL)
        return bad(PDPLQR_ERR_UNSUPPORTED, "needs a SERIAL handle (PARALLEL and KKT are not supported)");
    const Shape &sh = h->sh;
    if (sh.s > 64) return bad(PDPLQR_ERR_UNSUPPORTED, "n + m > 64 is not supported");
    if (sh.ny == 0) return bad(PDPLQR_ERR_UNSUPPORTED, "the handle has no constraint rows (use pdplqr_adjoint)");
    if (!h->cfg.keep_factors) return bad(PDPLQR_ERR_UNSUPPORTED, "requires keep_factors = 1");
    if (!ws || !ys || !zs || !lb || !ub || !rho || !gws)
        return bad(PDPLQR_ERR_INVALID, "null ws / ys / zs / lb / ub / rho / gws");
    if (!(alpha > 0.0 && alpha < 2.0) || !(sigma >= 0.0) || !(tol >= 0.0) || max_iter < 1 || check_every < 1)
        return bad(PDPLQR_ERR_INVALID, "bad settings (0 < alpha < 2, sigma >= 0, tol >= 0, max_iter >= 1, check_every >= 1)");
    if (!h->Lc || !h->lpc || !h->factored) return bad(PDPLQR_ERR_STATE, "called before backward");
    if (h->rec_gain) return bad(PDPLQR_ERR_STATE, "the rollout record is not in factor form");
    if (int brc = bind_device(h)) return brc;
    AdjointRowsArgs ra;
    if (!adjoint_rows_plan(sh, h->y_off_h.data(), h->d_off_h.data(), ra))
        return bad(PDPLQR_ERR_UNSUPPORTED, "the constraint rows of one stage exceed the kernel's LDS tile");
    int rc = adjoint_alloc(h);
    if (rc) return rc;
    AdjointState *s = h->adj;
    const long long B = sh.batch, Y = B * sh.ny, W = B * sh.perh;
    // first use; every pointer is guarded on its own, so a call after a failed allocation takes up where that one stopped
    if ((!s->fa_w && (rc = dev_alloc(h, &s->fa_w, W))) || (!s->fa_y && (rc = dev_alloc(h, &s->fa_y, Y))) ||
        (!s->fa_z && (rc = dev_alloc(h, &s->fa_z, Y))) || (!s->fjq && (rc = dev_alloc(h, &s->fjq, Y))) ||
        (!s->fgvs && (rc = dev_alloc(h, &s->fgvs, Y))) || (!s->fresid && (rc = dev_alloc(h, &s->fresid, 2 * B))) ||
        (!s->fint && (rc = dev_alloc(h, &s->fint, 4 + 3 * B))))
        return rc;
    if (!s->factive_h) {
        int32_t *pin = nullptr;
        PDPLQR_HIP_TRY(hipHostMalloc((void **)&pin, 3 * sizeof(int32_t), hipHostMallocDefault));
        s->factive_h = pin;
    }
    const bool dev = mem == PDPLQR_MEM_DEVICE;
    hipStream_t st = h->stream;

    // inputs: read in place on the device, staged from the host
    const double *dws, *din[6];
    if ((rc = stage_in(h, ws, h->st_ws, W, mem, &dws))) return rc;
    const double *const hin[6] = {ys, zs, lb, ub, rho, gws};
    for (int i = 0; i < 6; ++i) {
        const long long cnt = i < 5 ? Y : W;
        if (!dev && !s->fin[i] && (rc = dev_alloc(h, &s->fin[i], cnt))) return rc;
        if ((rc = stage_in(h, hin[i], s->fin[i], cnt, mem, &din[i]))) return rc;
    }
    int32_t *active = s->fint;
    if (h->num_cones > 0) {
        // rho constant within a cone (the projection is Euclidean only then), before anything is written
        PDPLQR_HIP_TRY(hipMemsetAsync(active, 0, 3 * sizeof(int32_t), st));
        if ((rc = launch_cone_validate(sh.batch, sh.ny, h->num_cones, h->cone_y0, h->cone_dim, din[2], din[4],
                                       active + 1, st)))
            return rc;
        PDPLQR_HIP_TRY(hipMemcpyAsync(s->factive_h, active, 3 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        PDPLQR_HIP_TRY(hipStreamSynchronize(st));
        if (s->factive_h[1] != 0 || s->factive_h[2] != 0)
            return bad(PDPLQR_ERR_INVALID, (std::to_string(s->factive_h[1]) + " cones with rho not constant over their "
                       "rows, " + std::to_string(s->factive_h[2]) + " cone rows whose lb is not finite").c_str());
    }
    // outputs: the caller's device pointers, or staging allocated on first use
    double *const user[8] = {gE, gc, gH, gh, gx, gD, glb, gub};
    const long long cnt[8] = {B * sh.perE, B * sh.perc, B * sh.perH, W, B * sh.n, B * sh.ndD, Y, Y};
    double *out[8];
    for (int i = 0; i < 8; ++i) {
        out[i] = cnt[i] > 0 ? user[i] : nullptr;
        if (out[i] && !dev) {
            if (!s->out[i] && (rc = dev_alloc(h, &s->out[i], cnt[i]))) return rc;
            out[i] = s->out[i];
        }
    }

    // a = 0: the first cotangents are (gws, 0, 0)
    PDPLQR_HIP_TRY(hipMemsetAsync(s->fa_w, 0, (size_t)W * sizeof(double), st));
    PDPLQR_HIP_TRY(hipMemsetAsync(s->fa_y, 0, (size_t)Y * sizeof(double), st));
    PDPLQR_HIP_TRY(hipMemsetAsync(s->fa_z, 0, (size_t)Y * sizeof(double), st));
    PDPLQR_HIP_TRY(hipMemsetAsync(s->fresid, 0, (size_t)(2 * B) * sizeof(double), st));
    PDPLQR_HIP_TRY(hipMemsetAsync(s->fint, 0, (size_t)(4 + 3 * B) * sizeof(int32_t), st));
    s->fp_ran = true;
    FpadjArgs q = fpadj_args(h, din, sigma, alpha, tol);
    if ((rc = launch_fpadj_step(q, st))) return rc;

    if ((rc = launch_adjoint_lu(sh, h->KD, s->lus, false, st))) return rc;
    for (int it = 1; it <= max_iter && !rc; ++it) {
        const bool test = it % check_every == 0 || it == max_iter;
        if ((rc = adjoint_solve(h, s->rhs, s->v))) break;
        if (test && hipMemsetAsync(active, 0, sizeof(int32_t), st) != hipSuccess) rc = PDPLQR_ERR_HIP;
        q.v = s->v;
        q.test = test ? 1 : 0;
        q.it = it;
        if (!rc) rc = launch_fpadj_step(q, st);
        if (rc || !test) continue;
        if (hipMemcpyAsync(s->factive_h, active, sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess) {
            rc = fail(PDPLQR_ERR_HIP, "admm_adjoint_fixed_point: reading the active count failed");
            break;
        }
        if (s->factive_h[0] == 0) break;
    }
    // the final pass: the cotangents' row vectors, then the solve the gradients are read from
    const bool need_solve = out[0] || out[1] || out[2] || out[3] || out[4] || out[5];
    if (!rc && (need_solve || out[6] || out[7])) {
        q.v = nullptr;
        q.test = 0;
        q.gvs = s->fgvs;
        q.glb = out[6];
        q.gub = out[7];
        rc = launch_fpadj_step(q, st);
    }
    if (!rc && need_solve) rc = adjoint_solve(h, s->rhs, s->v);
    // the record's lu' goes back whatever the launches returned
    const int rc2 = launch_adjoint_lu(sh, h->KD, s->lus, true, st);
    if (rc || rc2) return rc ? rc : rc2;

    if (need_solve) {
        if ((rc = launch_adjoint_grad(adjoint_args(h, dws, out[0], out[1], out[2], out[3], out[4]), st))) return rc;
        if (out[5]) {
            adjoint_rows_args(h, ra, dws, din[4], s->fgvs, out[5], nullptr, nullptr);
            if ((rc = launch_adjoint_rows(ra, h->y_off_h.data(), h->d_off_h.data(), st))) return rc;
        }
    }
    if (!dev) {
        for (int i = 0; i < 8; ++i)
            if (out[i])
                PDPLQR_HIP_TRY(hipMemcpyAsync(user[i], out[i], (size_t)cnt[i] * sizeof(double), hipMemcpyDeviceToHost, st));
        PDPLQR_HIP_TRY(hipStreamSynchronize(st));
    }
    h->host_staged = false;
    return PDPLQR_OK;
}

extern "C" int pdplqr_admm_adjoint_fixed_point_info(pdplqr_handle h, int32_t *iters, int32_t *converged,
                                                    double *resid) {
    if (!h) return fail(PDPLQR_ERR_INVALID, "admm_adjoint_fixed_point_info: null handle");
    if (!h->adj || !h->adj->fp_ran)
        return fail(PDPLQR_ERR_STATE, "admm_adjoint_fixed_point_info before admm_adjoint_fixed_point");
    if (int brc = bind_device(h)) return brc;
    PDPLQR_HIP_TRY(hipStreamSynchronize(h->stream));
    const size_t B = (size_t)h->sh.batch;
    const int32_t *conv = h->adj->fint + 4 + B, *its = conv + B;
    if (iters) PDPLQR_HIP_TRY(hipMemcpy(iters, its, B * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (converged) PDPLQR_HIP_TRY(hipMemcpy(converged, conv, B * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (resid) PDPLQR_HIP_TRY(hipMemcpy(resid, h->adj->fresid, 2 * B * sizeof(double), hipMemcpyDeviceToHost));
    return PDPLQR_OK;
}

// Internal diagnostic (not part of include/pdplqr.h; scripts/cone_adjoint_bench.py):
// k_fpadj_step alone, a middle iteration (state stepped, right-hand side
// written, no test) on the state and the adjoint solution the last
// pdplqr_admm_adjoint_fixed_point left in the scratch, every problem unfrozen.
// The call's vectors are arguments (device pointers; nothing of an earlier
// call's is kept).  The state is scratch: the next call starts it from zero.
extern "C" int pdplqr_debug_fpadj_step(pdplqr_handle h, const double *ys, const double *zs, const double *lb,
                                       const double *ub, const double *rho, const double *gws, double sigma,
                                       double alpha) {
    if (!h || !h->adj || !h->adj->fp_ran) return fail(PDPLQR_ERR_STATE, "debug_fpadj_step before admm_adjoint_fixed_point");
    if (!ys || !zs || !lb || !ub || !rho || !gws) return fail(PDPLQR_ERR_INVALID, "debug_fpadj_step: null input");
    if (int brc = bind_device(h)) return brc;
    const double *const in[6] = {ys, zs, lb, ub, rho, gws};
    FpadjArgs q = fpadj_args(h, in, sigma, alpha, 0.0);
    PDPLQR_HIP_TRY(hipMemsetAsync(q.done, 0, (size_t)h->sh.batch * sizeof(int32_t), h->stream));
    q.v = h->adj->v;
    return launch_fpadj_step(q, h->stream);
}
