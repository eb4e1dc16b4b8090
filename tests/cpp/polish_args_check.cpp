// polish_args_check.cpp -- host-side drive of the polish entry points' argument
// and state checks: create -> pdplqr_admm_set_polish / polish_info /
// kkt_residuals checks -> destroy, no device solve.  Meant to be linked against
// the library's sources built with -Xarch_host -fsanitize=address,undefined
// (see DESIGN.md section 5.8).  Without a HIP device pdplqr_create fails and
// only the null-handle checks run; the exit code is 0 when every check that
// could run gave the documented code.
#include <cmath>
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

int main() {
    double meas[8] = {0};
    int32_t st[1] = {0};
    EXPECT(pdplqr_admm_set_polish(nullptr, 1, 1e-6, 3), PDPLQR_ERR_INVALID);
    EXPECT(pdplqr_admm_polish_info(nullptr, st, st, meas), PDPLQR_ERR_INVALID);
    EXPECT(pdplqr_admm_kkt_residuals(nullptr, meas, meas, meas, meas, meas, meas, PDPLQR_MEM_HOST), PDPLQR_ERR_INVALID);

    pdplqr_config cfg;
    pdplqr_config_init(&cfg);
    int32_t ncs[7] = {2, 2, 2, 2, 2, 2, 0};
    cfg.nx = 4;
    cfg.nu = 2;
    cfg.N = 6;
    cfg.batch = 1;
    cfg.ncs = ncs;
    pdplqr_handle h = nullptr;
    const int rc = pdplqr_create(&cfg, &h);
    if (rc != PDPLQR_OK) {
        std::printf("pdplqr_create: %d (%s): no device, handle checks skipped\n", rc, pdplqr_last_error());
        std::printf(fails ? "FAILED\n" : "OK (null-handle checks only)\n");
        return fails ? 1 : 0;
    }
    EXPECT(pdplqr_admm_set_polish(h, 1, 0.0, 3), PDPLQR_ERR_INVALID);
    EXPECT(pdplqr_admm_set_polish(h, 1, -1e-6, 3), PDPLQR_ERR_INVALID);
    EXPECT(pdplqr_admm_set_polish(h, 1, std::nan(""), 3), PDPLQR_ERR_INVALID);
    EXPECT(pdplqr_admm_set_polish(h, 1, 1e-6, -1), PDPLQR_ERR_INVALID);
    EXPECT(pdplqr_admm_set_polish(h, 0, -1.0, -1), PDPLQR_OK);  // off: the values are not looked at
    EXPECT(pdplqr_admm_set_polish(h, 1, 1e-6, 0), PDPLQR_OK);
    EXPECT(pdplqr_admm_polish_info(h, st, nullptr, nullptr), PDPLQR_ERR_STATE);  // no admm_solve yet
    EXPECT(pdplqr_admm_kkt_residuals(h, meas, meas, meas, meas, meas, nullptr, PDPLQR_MEM_HOST), PDPLQR_ERR_INVALID);
    EXPECT(pdplqr_admm_kkt_residuals(h, meas, meas, meas, meas, meas, meas, PDPLQR_MEM_HOST), PDPLQR_ERR_STATE);  // no model
    EXPECT(pdplqr_destroy(h), PDPLQR_OK);
    std::printf(fails ? "FAILED\n" : "OK\n");
    return fails ? 1 : 0;
}
