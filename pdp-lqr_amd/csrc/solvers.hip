// solvers.hip -- dispatch of the protocol calls to the three solver kinds
// (the PARALLEL solver's host side: parallel_host.hip) and the graph capture.
#include <cstdlib>

#include "admm.hpp"
#include "parallel.hpp"
#include "solvers.hpp"

namespace pdplqr {

static int unsupported(const char *what) {
    set_error(std::string(what) + ": not implemented in this build");
    return PDPLQR_ERR_UNSUPPORTED;
}

void graph_release(pdplqr_handle h);

// ---------------------------------------------------------------------------
int solver_init(pdplqr_handle h) {
    switch (h->cfg.solver) {
        case PDPLQR_SOLVER_SERIAL:
            if (h->sh.s > 256) return unsupported("SERIAL solver with n + m > 256");
            if (xl_shape(h->sh)) return dev_alloc(h, &h->xl_ws, (size_t)h->sh.batch * xl_ws_doubles(h->sh));
            return PDPLQR_OK;
        case PDPLQR_SOLVER_PARALLEL:
            return parallel_init(h);
        default:
            return kkt_init(h);
    }
}

void solver_release(pdplqr_handle h) {
    graph_release(h);
    admm_release(h);
    adjoint_release(h);
    adjoint_parallel_release(h);
    parallel_release(h);
    kkt_release(h);
}

int solver_on_model(pdplqr_handle h) {
    return h->cfg.solver == PDPLQR_SOLVER_KKT ? kkt_on_model(h) : PDPLQR_OK;
}

int solver_update(pdplqr_handle h, const double *ws, const double *ys, const double *zs, const double *irho,
                  double sigma) {
    if (h->cfg.solver == PDPLQR_SOLVER_KKT) return kkt_update(h, ws, ys, zs, irho, sigma);
    const bool cacheable = h->max_nc <= 0;
    const bool skipH = cacheable && h->hw_cached && h->hw_sigma == sigma;
    const int rc = launch_update_problem_data(h->sh, h->H, h->h, ws, ys, zs, irho, sigma, h->Hw, h->hw, h->gw,
                                              h->tab_s, h->tab_n, h->stream, skipH);
    h->hw_cached = rc == PDPLQR_OK && cacheable;
    h->hw_sigma = sigma;
    return rc;
}

// ---------------------------------------------------------------------------
// HIP graphs.  A protocol call issues a fixed sequence of launches whose
// arguments depend only on the handle and on the call's device pointers (the
// parallel solver: ~20 short kernels, launch-rate bound from the host).  The
// sequence is captured once per (pointer set, stream) and replayed with one
// hipGraphLaunch.  Host-side state the sequence sets is set outside the
// captured part.  Opt-in (PDPLQR_GRAPH=1): measured on MI355X the replay is
// not faster -- C2 (N = 1024 single problem, ~20 kernels) 0.169 ms issued
// directly vs 0.176 ms replayed; the GPU-side dispatch gap, not the host
// launch rate, separates the kernels.  A stream that cannot capture (the
// legacy null stream) falls back to direct issue.
// ---------------------------------------------------------------------------
void graph_release(pdplqr_handle h) {
    for (auto &g : h->graphs) {
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
        g = pdplqr_handle_s::Graph{};
    }
}

template <class Issue>
static int run_graphed(pdplqr_handle h, int slot, const void *k1, const void *k2, Issue &&issue) {
    static const bool off = getenv("PDPLQR_GRAPH") == nullptr;
    if (off || !h->stream) return issue();
    auto &g = h->graphs[slot];
    if (g.exec && g.k1 == k1 && g.k2 == k2 && g.stream == h->stream) {
        PDPLQR_HIP_TRY(hipGraphLaunch(g.exec, h->stream));
        return PDPLQR_OK;
    }
    if (g.exec) {
        (void)hipGraphExecDestroy(g.exec);
        g = pdplqr_handle_s::Graph{};
    }
    if (hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        (void)hipGetLastError();
        return issue();
    }
    const int rc = issue();
    hipGraph_t graph = nullptr;
    const hipError_t e = hipStreamEndCapture(h->stream, &graph);
    if (rc || e != hipSuccess || !graph) {
        if (graph) (void)hipGraphDestroy(graph);
        (void)hipGetLastError();
        return rc ? rc : issue();  // capture failed: run the sequence directly
    }
    hipGraphExec_t exec = nullptr;
    const hipError_t ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ei != hipSuccess) {
        (void)hipGetLastError();
        return issue();
    }
    g.exec = exec;
    g.k1 = k1;
    g.k2 = k2;
    g.stream = h->stream;
    PDPLQR_HIP_TRY(hipGraphLaunch(g.exec, h->stream));
    return PDPLQR_OK;
}

// the constraint row count shared by every stage k < N, or 0
static int uniform_nc(pdplqr_handle h) {
    const int N = h->sh.N;
    if (N < 1) return 0;
    const int nc = h->ncs[0];
    for (int k = 1; k < N; ++k)
        if (h->ncs[k] != nc) return 0;
    return nc;
}

int solver_backward(pdplqr_handle h, const double *rho) {
    if (h->cfg.solver == PDPLQR_SOLVER_PARALLEL) h->shard_last = 1;
    // the record form is host state: set outside the (replayable) launch sequence
    h->rec_gain = (h->cfg.solver == PDPLQR_SOLVER_SERIAL && schur_gain_record(riccati_args(h))) ||
                  (h->cfg.solver == PDPLQR_SOLVER_KKT && kkt_plain_rec_ehat(h));
    // the record form selects the backward kernel: it is part of the graph key
    // (a replay of the other form's capture would leave the record in the
    // layout the forward does not read)
    return run_graphed(h, 0, rho, reinterpret_cast<const void *>((intptr_t)(h->rec_gain ? 2 : 1)), [&]() -> int {
        if (h->cfg.solver == PDPLQR_SOLVER_KKT) return kkt_backward(h, rho);  // rho = inv_rho (qdldl_solver.hpp:88)
        if (h->cfg.solver == PDPLQR_SOLVER_SERIAL && h->max_nc > 0) {
            // the penalty inside the streamed backward (one pass, H~ / h~ penalised in place)
            const int nc = uniform_nc(h);
            if (nc > 0 && h->rec_gain) {
                RiccatiArgs a = riccati_args(h);
                a.D = h->D;
                a.rho = rho;
                a.gw = h->gw;
                a.d_off = h->d_off;
                a.y_off = h->y_off;
                a.nc_last = h->ncs[h->sh.N];
                const int rc = launch_riccati_backward_pen(a, nc, h->stream);
                if (rc != PDPLQR_ERR_UNSUPPORTED) return rc;
            }
        }
        int rc = launch_penalty(h->sh, h->D, rho, h->gw, h->Hw, h->hw, h->d_off, h->y_off, h->tab_s, h->tab_n, 1,
                                h->max_nc, h->stream);
        if (rc) return rc;
        if (h->cfg.solver == PDPLQR_SOLVER_PARALLEL) return parallel_backward(h, 1);
        return launch_riccati_backward(riccati_args(h), h->stream);
    });
}

int solver_backward_nofact(pdplqr_handle h, const double *rho) {
    const int last = h->shard_last;
    h->rec_gain = false;  // the nofact kernels write lu' into the L-form record
    return run_graphed(h, 1, rho, reinterpret_cast<const void *>((intptr_t)(last + 1)), [&]() -> int {
        int rc = launch_penalty(h->sh, h->D, rho, h->gw, h->Hw, h->hw, h->d_off, h->y_off, h->tab_s, h->tab_n, 0,
                                h->max_nc, h->stream);
        if (rc) return rc;
        // LQRParallelSolver::backward_without_factorization (lqr_solver_parallel.hpp:148-154)
        if (h->cfg.solver == PDPLQR_SOLVER_PARALLEL) return parallel_backward(h, last, false);
        return launch_riccati_backward_nofact(riccati_args(h), h->stream);
    });
}

int solver_backward_prepared(pdplqr_handle h) {
    const bool fact = h->Lc == nullptr || h->lpc == nullptr;
    if (h->cfg.solver == PDPLQR_SOLVER_PARALLEL) return parallel_backward(h, 1, fact);
    const RiccatiArgs a = riccati_args(h);
    h->rec_gain = fact && schur_gain_record(a);
    return fact ? launch_riccati_backward(a, h->stream) : launch_riccati_backward_nofact(a, h->stream);
}

// ADMM: the update of iteration it fused into the backward of it + 1
// (serial solver with cached factors; ERR_UNSUPPORTED otherwise)
int solver_nofact_admm(pdplqr_handle h, const AdmmArgs &a, bool check) {
    if (h->cfg.solver != PDPLQR_SOLVER_SERIAL) return PDPLQR_ERR_UNSUPPORTED;
    for (int k = 0; k < h->sh.N; ++k)
        if (h->ncs[k] != 4) return PDPLQR_ERR_UNSUPPORTED;
    if (h->ncs[h->sh.N] != 0) return PDPLQR_ERR_UNSUPPORTED;
    h->rec_gain = false;
    return launch_nofact_admm(riccati_args(h), a, check, h->stream);
}

int solver_forward(pdplqr_handle h, const double *x0, double *ws) {
    // a forward sequence captured for the other record form is stale
    auto &g = h->graphs[2];
    if (g.exec && h->graph_rec_gain != h->rec_gain) {
        (void)hipGraphExecDestroy(g.exec);
        g = pdplqr_handle_s::Graph{};
    }
    h->graph_rec_gain = h->rec_gain;
    return run_graphed(h, 2, x0, ws, [&]() -> int {
        if (h->cfg.solver == PDPLQR_SOLVER_KKT) return kkt_forward(h, x0, ws);
        if (h->cfg.solver == PDPLQR_SOLVER_PARALLEL) return parallel_forward(h, x0, ws, nullptr, nullptr, 1);
        if (h->rec_gain) {
            const int rc = launch_rollout_dma(h->sh, h->E, h->c, h->KD, x0, ws, h->stream, true);
            if (rc == PDPLQR_ERR_UNSUPPORTED) set_error("forward: the model changed layout since backward");
            return rc;
        }
        return launch_riccati_forward(h->sh, h->E, h->c, h->KD, x0, ws, h->stream);
    });
}

int solver_clear(pdplqr_handle) { return PDPLQR_OK; }

int solver_status(pdplqr_handle h, int32_t *flags) {
    if (h->cfg.solver != PDPLQR_SOLVER_PARALLEL) {
        PDPLQR_HIP_TRY(hipMemcpy(flags, h->status, (size_t)h->sh.batch * sizeof(int32_t), hipMemcpyDeviceToHost));
        return PDPLQR_OK;
    }
    return parallel_status(h, flags);
}

}  // namespace pdplqr
