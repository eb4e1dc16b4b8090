// adjoint_parallel.hip -- pdplqr_adjoint_parallel: pdplqr_adjoint's gradients
// for a PARALLEL (segmented) handle (new: the reference has no such call).
//
// The adjoint solve is backward_without_factorization + forward of the same
// segmented factorisation with h~ := dl/dw, c := 0, x0 := 0 (log depth in the
// horizon).  The per-stage costates, which the serial path forms from its
// cached Lxx_k, come from k_seg_costate (kernels_adjoint_parallel.hip): every
// device segment walks back from the boundary costate the suffix scans give.
//
// Handle state.  The adjoint solve runs on an element array, a scan ping-pong,
// a failure flag and an lpc of its own; the elements' F, C, P are copied in
// (device to device) per call, so the primal elements and the primal suffix
// scan -- which the costates read and a later forward needs -- are never
// written.  The boundary maps, vfun, xhat and lam are shared with the handle:
// every forward rebuilds them from the elements, the scan and x0 before it
// reads them.  The one thing the nofact recursion overwrites in place is the
// lu' column of the rollout records, saved and restored as pdplqr_adjoint does
// (m doubles per stage each way, against a second copy of the whole record).
#include "adjoint.hpp"
#include "parallel.hpp"
#include "solvers.hpp"

namespace pdplqr {

struct ParAdjointState {
    double *zc = nullptr, *zx0 = nullptr;  // c = 0, x0 = 0
    double *rhs = nullptr, *v = nullptr;   // dl/dw in the hw layout; the adjoint solution
    double *lpa = nullptr, *lus = nullptr; // the adjoint lp_k; the primal lu'_k [b][N][m]
    double *elem = nullptr, *bufA = nullptr, *bufB = nullptr;  // the adjoint solve's elements and scan
    int *flag = nullptr;
    double *lam = nullptr, *mu = nullptr;  // costates [b][N + 1][n]
    double *out[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // host outputs' staging
};

void adjoint_parallel_release(pdplqr_handle h) {
    delete h->padj;
    h->padj = nullptr;
}

static int par_adjoint_alloc(pdplqr_handle h, int S) {
    if (h->padj) return PDPLQR_OK;
    const Shape &sh = h->sh;
    const long long B = sh.batch, es = elem_doubles(sh.n), cs = B * (sh.N + 1) * sh.n;
    ParAdjointState s;
    int rc;
    if ((rc = dev_alloc(h, &s.zc, B * sh.perc)) || (rc = dev_alloc(h, &s.zx0, B * sh.n)) ||
        (rc = dev_alloc(h, &s.rhs, B * sh.perh)) || (rc = dev_alloc(h, &s.v, B * sh.perh)) ||
        (rc = dev_alloc(h, &s.lpa, B * sh.perh)) || (rc = dev_alloc(h, &s.lus, B * sh.N * sh.m)) ||
        (rc = dev_alloc(h, &s.elem, B * S * es)) || (rc = dev_alloc(h, &s.bufA, B * S * es)) ||
        (rc = dev_alloc(h, &s.bufB, B * S * es)) || (rc = dev_alloc(h, &s.flag, B)) ||
        (rc = dev_alloc(h, &s.lam, cs)) || (rc = dev_alloc(h, &s.mu, cs)))
        return rc;
    PDPLQR_HIP_TRY(hipMemsetAsync(s.zc, 0, (size_t)(B * sh.perc) * sizeof(double), h->stream));
    PDPLQR_HIP_TRY(hipMemsetAsync(s.zx0, 0, (size_t)(B * sh.n) * sizeof(double), h->stream));
    h->padj = new ParAdjointState(s);
    return PDPLQR_OK;
}

static int pfail(int code, const char *msg) {
    set_error(msg);
    return code;
}

}  // namespace pdplqr

using namespace pdplqr;

extern "C" int pdplqr_adjoint_parallel(pdplqr_handle h, const double *ws, const double *gws, double *gE, double *gc,
                                       double *gH, double *gh, double *gx, int mem) {
    if (!h) return pfail(PDPLQR_ERR_INVALID, "adjoint_parallel: null handle");
    if (!ws || !gws) return pfail(PDPLQR_ERR_INVALID, "adjoint_parallel: null ws/gws");
    if (h->md) return pfail(PDPLQR_ERR_UNSUPPORTED, "adjoint_parallel: multi-device handles are not supported");
    if (h->cfg.solver != PDPLQR_SOLVER_PARALLEL || !h->par)
        return pfail(PDPLQR_ERR_UNSUPPORTED, "adjoint_parallel needs a PARALLEL handle (SERIAL: pdplqr_adjoint)");
    if (h->sh.ny > 0)
        return pfail(PDPLQR_ERR_UNSUPPORTED, "adjoint_parallel: constrained stages (ncs > 0) are not supported");
    if (h->sh.s > 64) return pfail(PDPLQR_ERR_UNSUPPORTED, "adjoint_parallel: n + m > 64 is not supported");
    if (!h->cfg.keep_factors || !h->Lc || !h->lpc)
        return pfail(PDPLQR_ERR_STATE, "adjoint_parallel requires keep_factors = 1");
    if (!h->factored) return pfail(PDPLQR_ERR_STATE, "adjoint_parallel before backward");
    if (!h->shard_last)
        return pfail(PDPLQR_ERR_STATE, "adjoint_parallel: the handle holds a horizon shard that is not the last");
    if (int brc = bind_device(h)) return brc;
    const Shape &sh = h->sh;
    ParallelView pv;
    parallel_view(h, pv);
    int rc = par_adjoint_alloc(h, pv.S);
    if (rc) return rc;
    ParAdjointState *s = h->padj;
    const long long B = sh.batch;
    const bool dev = mem == PDPLQR_MEM_DEVICE;
    hipStream_t st = h->stream;

    // inputs: ws is read in place on the device (host: staged as forward's output is); the
    // right-hand side is copied, so the recursion never reads the caller's buffer
    const double *dws;
    if ((rc = stage_in(h, ws, h->st_ws, B * sh.perh, mem, &dws))) return rc;
    PDPLQR_HIP_TRY(hipMemcpyAsync(s->rhs, gws, (size_t)(B * sh.perh) * sizeof(double),
                                  dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    // outputs: the caller's device pointers, or staging allocated on first use
    double *const user[5] = {gE, gc, gH, gh, gx};
    const long long cnt[5] = {B * sh.perE, B * sh.perc, B * sh.perH, B * sh.perh, B * sh.n};
    double *out[5];
    for (int i = 0; i < 5; ++i) {
        out[i] = user[i];
        if (out[i] && !dev) {
            if (!s->out[i] && (rc = dev_alloc(h, &s->out[i], cnt[i]))) return rc;
            out[i] = s->out[i];
        }
    }

    // v: the segment nofact recursion and the suffix scan on the adjoint's own elements
    // (F, C, P of the factorisation copied in), then maps, composition and segment rollout
    PDPLQR_HIP_TRY(hipMemcpyAsync(s->elem, pv.elem, (size_t)(B * pv.S * elem_doubles(sh.n)) * sizeof(double),
                                  hipMemcpyDeviceToDevice, st));
    ParallelSub sub;
    sub.c = s->zc;
    sub.hw = s->rhs;
    sub.lpc = s->lpa;
    sub.elem = s->elem;
    sub.bufA = s->bufA;
    sub.bufB = s->bufB;
    sub.flag = s->flag;
    if ((rc = launch_adjoint_lu(sh, h->KD, s->lus, false, st))) return rc;
    rc = parallel_backward(h, 1, false, &sub);
    if (!rc) rc = parallel_forward(h, s->zx0, s->v, nullptr, nullptr, 1, 0, &sub);
    // the record's lu' goes back whatever the launches returned
    const int rc2 = launch_adjoint_lu(sh, h->KD, s->lus, true, st);
    if (rc || rc2) return rc ? rc : rc2;

    if (out[0] || out[1] || out[4]) {  // the costates: lambda for grad E only, mu for grad E, c, x0
        SegCostateArgs ca;
        ca.sh = sh;
        ca.S = pv.S;
        ca.seg_start = pv.seg_start;
        ca.seg_len = pv.seg_len;
        ca.E = h->E;
        ca.FR = h->KD;
        ca.Lc = h->Lc;
        ca.lpc = h->lpc;
        ca.lpa = s->lpa;
        ca.ws = dws;
        ca.v = s->v;
        ca.sufp = pv.suf_final;
        ca.sufa = sub.suf_final;
        ca.lam = s->lam;
        ca.mu = s->mu;
        ca.need_lam = out[0] ? 1 : 0;
        if ((rc = launch_seg_costate(ca, st))) return rc;
    }
    AdjointCostateArgs g;
    g.sh = sh;
    g.ws = dws;
    g.v = s->v;
    g.lam = s->lam;
    g.mu = s->mu;
    g.gE = out[0];
    g.gc = out[1];
    g.gH = out[2];
    g.gh = out[3];
    g.gx = out[4];
    if ((rc = launch_adjoint_grad_costate(g, st))) return rc;

    if (!dev) {
        for (int i = 0; i < 5; ++i)
            if (out[i])
                PDPLQR_HIP_TRY(hipMemcpyAsync(user[i], out[i], (size_t)cnt[i] * sizeof(double), hipMemcpyDeviceToHost, st));
        PDPLQR_HIP_TRY(hipStreamSynchronize(st));
    }
    h->host_staged = false;
    return PDPLQR_OK;
}
