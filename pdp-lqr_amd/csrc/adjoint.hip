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
#include "solvers.hpp"

namespace pdplqr {

struct AdjointState {
    double *zc = nullptr, *zx0 = nullptr;  // c = 0, x0 = 0
    double *rhs = nullptr;                 // dl/dw in the hw layout
    double *v = nullptr;                   // adjoint solution
    double *lpa = nullptr;                 // adjoint lp_k = [lu'; p^_k]
    double *lus = nullptr;                 // the primal lu'_k, [b][N][m]
    double *out[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // host outputs' staging (gE, gc, gH, gh, gx)
};

void adjoint_release(pdplqr_handle h) {
    delete h->adj;
    h->adj = nullptr;
}

static int jalloc(pdplqr_handle h, double **p, long long count) {
    *p = nullptr;
    void *q = nullptr;
    const hipError_t e = hipMalloc(&q, (size_t)(count > 0 ? count : 1) * sizeof(double));
    if (e != hipSuccess) {
        set_error(std::string("adjoint: hipMalloc: ") + hipGetErrorString(e));
        return PDPLQR_ERR_ALLOC;
    }
    h->allocs.push_back(q);
    *p = reinterpret_cast<double *>(q);
    return PDPLQR_OK;
}

static int adjoint_alloc(pdplqr_handle h) {
    if (h->adj) return PDPLQR_OK;
    const Shape &sh = h->sh;
    const long long B = sh.batch;
    AdjointState s;
    int rc;
    if ((rc = jalloc(h, &s.zc, B * sh.perc)) || (rc = jalloc(h, &s.zx0, B * sh.n)) ||
        (rc = jalloc(h, &s.rhs, B * sh.perh)) || (rc = jalloc(h, &s.v, B * sh.perh)) ||
        (rc = jalloc(h, &s.lpa, B * sh.perh)) || (rc = jalloc(h, &s.lus, B * sh.N * sh.m)))
        return rc;
    PDPLQR_HIP_TRY(hipMemsetAsync(s.zc, 0, (size_t)(B * sh.perc) * sizeof(double), h->stream));
    PDPLQR_HIP_TRY(hipMemsetAsync(s.zx0, 0, (size_t)(B * sh.n) * sizeof(double), h->stream));
    h->adj = new AdjointState(s);
    return PDPLQR_OK;
}

static int fail(int code, const char *msg) {
    set_error(msg);
    return code;
}

}  // namespace pdplqr

using namespace pdplqr;

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

    PDPLQR_HIP_TRY(hipSetDevice(h->cfg.device));
    int rc = adjoint_alloc(h);
    if (rc) return rc;
    AdjointState *s = h->adj;
    const Shape &sh = h->sh;
    const long long B = sh.batch;
    const bool dev = mem == PDPLQR_MEM_DEVICE;
    hipStream_t st = h->stream;

    // inputs: ws is read in place on the device (host: staged as forward's output is);
    // dl/dw is copied, so the recursion's kernel choice never depends on the caller's alignment
    const double *dws = ws;
    if (!dev) {
        PDPLQR_HIP_TRY(hipMemcpyAsync(h->st_ws, ws, (size_t)(B * sh.perh) * sizeof(double), hipMemcpyHostToDevice, st));
        dws = h->st_ws;
    }
    PDPLQR_HIP_TRY(hipMemcpyAsync(s->rhs, gws, (size_t)(B * sh.perh) * sizeof(double),
                                  dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    // outputs: the caller's device pointers, or staging allocated on first use
    double *user[5] = {gE, gc, gH, gh, gx};
    const long long cnt[5] = {B * sh.perE, B * sh.perc, B * sh.perH, B * sh.perh, B * sh.n};
    double *out[5];
    for (int i = 0; i < 5; ++i) {
        out[i] = user[i];
        if (user[i] && !dev) {
            if (!s->out[i] && (rc = jalloc(h, &s->out[i], cnt[i]))) return rc;
            out[i] = s->out[i];
        }
    }

    // v: backward_without_factorization + forward of (E, H~) with h~ := g, c := 0, x0 := 0
    if ((rc = launch_adjoint_lu(sh, h->KD, s->lus, false, st))) return rc;
    RiccatiArgs a;
    a.sh = sh;
    a.E = h->E;
    a.c = s->zc;
    a.Hw = h->Hw;
    a.hw = s->rhs;
    a.KD = h->KD;
    a.Lc = h->Lc;
    a.lpc = s->lpa;
    a.status = h->status;
    a.tab_s = h->tab_s;
    a.tab_n = h->tab_n;
    rc = launch_riccati_backward_nofact(a, st);
    if (!rc) rc = launch_riccati_forward(sh, h->E, s->zc, h->KD, s->zx0, s->v, st);
    // the record's lu' goes back whatever the launches returned
    const int rc2 = launch_adjoint_lu(sh, h->KD, s->lus, true, st);
    if (rc || rc2) return rc ? rc : rc2;

    AdjointArgs g;
    g.sh = sh;
    g.ws = dws;
    g.v = s->v;
    g.Lc = h->Lc;
    g.lpc = h->lpc;
    g.lpa = s->lpa;
    g.gE = out[0];
    g.gc = out[1];
    g.gH = out[2];
    g.gh = out[3];
    g.gx = out[4];
    if ((rc = launch_adjoint_grad(g, st))) return rc;

    if (!dev) {
        for (int i = 0; i < 5; ++i)
            if (user[i])
                PDPLQR_HIP_TRY(hipMemcpyAsync(user[i], out[i], (size_t)cnt[i] * sizeof(double), hipMemcpyDeviceToHost, st));
        PDPLQR_HIP_TRY(hipStreamSynchronize(st));
    }
    h->host_staged = false;
    return PDPLQR_OK;
}

// Internal diagnostic (not part of include/pdplqr.h; scripts/adjoint_bench.py):
// the gradient pass alone, on the adjoint solution the last pdplqr_adjoint
// left in the scratch.  Device pointers.
extern "C" int pdplqr_debug_adjoint_grad(pdplqr_handle h, const double *ws, double *gE, double *gc, double *gH,
                                         double *gh, double *gx) {
    if (!h || !ws || !h->adj || !h->Lc || !h->lpc) return fail(PDPLQR_ERR_STATE, "debug_adjoint_grad before adjoint");
    PDPLQR_HIP_TRY(hipSetDevice(h->cfg.device));
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
    return launch_adjoint_grad(g, h->stream);
}
