// admm_adjoint_args_check.cpp -- host-side drive of the argument and state
// checks of pdplqr_admm_adjoint / pdplqr_admm_adjoint_info: create -> the checks
// -> destroy, no device solve.  Meant to be linked against the library's sources
// built with -Xarch_host -fsanitize=address,undefined (see DESIGN.md section
// 5.9).  Without a HIP device pdplqr_create fails and only the null-handle checks
// run; the exit code is 0 when every check that could run gave the documented code.
#include <cstdio>

#include "pdplqr.h"

static int fails = 0;
#define EXPECT(call, want)                                                          \
    do {                                                                            \
        const int got_ = (call);                                                    \
        if (got_ != (want)) {                                                       \
            std::printf("FAIL %s = %d, expected %d\n", #call, got_, (int)(want));   \
            ++fails;                                                                \
        }                                                                           \
    } while (0)

static int adjoint(pdplqr_handle h, const double *gws, double *out) {
    return pdplqr_admm_adjoint(h, gws, nullptr, nullptr, nullptr, nullptr, out, nullptr, nullptr, nullptr, nullptr,
                               PDPLQR_MEM_HOST);
}

static pdplqr_handle make(int solver, int keep, const int32_t *ncs) {
    pdplqr_config cfg;
    pdplqr_config_init(&cfg);
    cfg.nx = 4;
    cfg.nu = 2;
    cfg.N = 6;
    cfg.batch = 1;
    cfg.solver = solver;
    cfg.keep_factors = keep;
    cfg.num_segments = solver == PDPLQR_SOLVER_PARALLEL ? 2 : 1;
    cfg.ncs = ncs;
    pdplqr_handle h = nullptr;
    const int rc = pdplqr_create(&cfg, &h);
    if (rc != PDPLQR_OK) std::printf("pdplqr_create: %d (%s)\n", rc, pdplqr_last_error());
    return rc == PDPLQR_OK ? h : nullptr;
}

int main() {
    double gws[40] = {0}, gh[40], resid[2] = {0};
    for (double &x : gh) x = 7.0;
    int32_t st[1] = {0};
    EXPECT(adjoint(nullptr, gws, gh), PDPLQR_ERR_INVALID);
    EXPECT(pdplqr_admm_adjoint_info(nullptr, st, resid), PDPLQR_ERR_INVALID);

    const int32_t ncs[7] = {2, 2, 2, 2, 2, 2, 0};
    pdplqr_handle h = make(PDPLQR_SOLVER_SERIAL, 1, ncs);
    if (!h) {
        std::printf("no device, handle checks skipped\n");
        std::printf(fails ? "FAILED\n" : "OK (null-handle checks only)\n");
        return fails ? 1 : 0;
    }
    EXPECT(adjoint(h, nullptr, gh), PDPLQR_ERR_INVALID);
    EXPECT(adjoint(h, gws, gh), PDPLQR_ERR_STATE);  // no admm_solve yet
    EXPECT(pdplqr_admm_adjoint_info(h, st, resid), PDPLQR_ERR_STATE);
    EXPECT(pdplqr_destroy(h), PDPLQR_OK);
    if ((h = make(PDPLQR_SOLVER_SERIAL, 0, ncs))) {
        EXPECT(adjoint(h, gws, gh), PDPLQR_ERR_STATE);  // keep_factors = 0
        EXPECT(pdplqr_destroy(h), PDPLQR_OK);
    }
    if ((h = make(PDPLQR_SOLVER_SERIAL, 1, nullptr))) {
        EXPECT(adjoint(h, gws, gh), PDPLQR_ERR_UNSUPPORTED);  // no rows
        EXPECT(pdplqr_destroy(h), PDPLQR_OK);
    }
    if ((h = make(PDPLQR_SOLVER_PARALLEL, 1, ncs))) {
        EXPECT(adjoint(h, gws, gh), PDPLQR_ERR_UNSUPPORTED);
        EXPECT(pdplqr_destroy(h), PDPLQR_OK);
    }
    if ((h = make(PDPLQR_SOLVER_KKT, 0, ncs))) {
        EXPECT(adjoint(h, gws, gh), PDPLQR_ERR_UNSUPPORTED);
        EXPECT(pdplqr_destroy(h), PDPLQR_OK);
    }
    for (double x : gh)
        if (x != 7.0) {
            std::printf("FAIL a refused call wrote its output\n");
            ++fails;
            break;
        }
    std::printf(fails ? "FAILED\n" : "OK\n");
    return fails ? 1 : 0;
}
