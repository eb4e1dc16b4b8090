// adjoint_store.hpp -- the flat output runs of the adjoint gradient kernels
// (kernels_adjoint.hip, kernels_adjoint_parallel.hip): a 256-thread block
// writes `cnt` consecutive doubles at `dst`, lane t storing elements
// [2 t, 2 t + 1] as one 16-byte store (VEC: cnt even, dst 16-byte aligned) or
// element t as an 8-byte store.
#pragma once
#include "device_common.hpp"

namespace pdplqr {

template <bool VEC, class F>
__device__ __forceinline__ void store_run(double *dst, int cnt, F &&val) {
    const int tid = threadIdx.x;
    if (VEC) {
        for (int e = 2 * tid; e < cnt; e += 512) {
            d2v x;
            x.x = val(e);
            x.y = val(e + 1);
            gstore2(dst + e, x);
        }
    } else {
        for (int e = tid; e < cnt; e += 256) gstore(dst + e, val(e));
    }
}

}  // namespace pdplqr
