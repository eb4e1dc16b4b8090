// kernels_asadj.hip -- the device side of pdplqr_admm_adjoint (adjoint.hip;
// DESIGN.md section 5.9): the gradient of the box-constrained optimum on the
// active set the polish guessed.  New: the reference has no such call.
//
// The adjoint of the equality-constrained KKT solve on the active rows D_a is
//     H v + g~ + D_a^T eta + (dynamics) = 0,   D_a v = 0,
// solved by the polish's refinement on the factor of H + delta I + D_a^T D_a /
// delta: v <- solve(h~ := g~ - delta v + D_a^T eta), eta <- eta + D_a v / delta.
//
//   k_asadj_step   between two solves, one pass: r = D v, eta += act o r /
//                  delta, rhs = g~ - delta v + D^T eta (k_polish_ystep's
//                  layout: a block per problem, LPS lanes per stage, a
//                  butterfly per row, ragged nc_k, terminal rows of width n).
//                  D, act, v, g~ and eta of a stage are read once.  After the
//                  last solve rhs is not written; the block reduces max|D_a v|,
//                  max|v| and max|v - v_prev| in a fixed order instead and
//                  thread 0 writes the two measures and the problem's status.
//   k_asadj_rows   grad D_k = y_a,k v_k^T + (eta_k + gvs_k) w~_k^T, grad lb =
//                  -eta on the lower-active rows (target == lb, which takes
//                  lb == ub), grad ub = -eta on the other active rows, zeros
//                  elsewhere.  k_adjoint_rows's tiling: up to 16 stages per
//                  block within 40 KB of LDS, the tile's slices of the offset
//                  tables in LDS, every output's tile one flat run, 16 bytes
//                  per lane where the run is aligned, 8 otherwise.  D itself is
//                  not read: the gradient is two outer products.
// Contraction is off: a value does not depend on which outputs were requested.
// No atomics, plain vector stores.
#include <algorithm>

#include "adjoint.hpp"
#include "device_common.hpp"

namespace pdplqr {

namespace {

__device__ __forceinline__ double as_wave_max(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
    return v;
}

template <int LPS>
__device__ __forceinline__ double as_stage_sum(double v) {
#pragma unroll
    for (int m = 1; m < LPS; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// dst[0 .. cnt) = val(e), e ascending per lane (k_adjoint_rows's store_run_rows)
template <class F>
__device__ __forceinline__ void as_store_run(double *dst, int cnt, bool vec, F &&val) {
    const int tid = threadIdx.x;
    if (vec) {
        for (int e = 2 * tid; e < cnt; e += 512) {
            const double x0 = val(e);
            if (e + 1 < cnt) {
                d2v x;
                x.x = x0;
                x.y = val(e + 1);
                gstore2(dst + e, x);
            } else {
                gstore(dst + e, x0);
            }
        }
    } else {
        for (int e = tid; e < cnt; e += 256) gstore(dst + e, val(e));
    }
}

}  // namespace

template <int LPS>
__global__ __launch_bounds__(256) void k_asadj_step(AsadjStepArgs a) {
#pragma clang fp contract(off)
    const Shape &sh = a.sh;
    const int b = blockIdx.x;
    constexpr int SPW = 64 / LPS;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, sub = lane / LPS, j = lane % LPS;
    const int N = sh.N, s = sh.s;
    const bool last = a.resid != nullptr;  // kernel-uniform
    const long long wb = (long long)b * sh.perh;
    double mdv = 0.0, mv = 0.0, mch = 0.0;
    for (int kb = wv * SPW; kb <= N; kb += 4 * SPW) {
        // wave-uniform trip count: lanes past the horizon idle in the loop
        const int k = kb + sub;
        const bool stg = k <= N;
        const int kk = stg ? k : N;
        const int dim = kk < N ? s : sh.n;
        const bool col = stg && j < dim;
        const long long wo = wb + (long long)kk * s + (j < dim ? j : 0);
        const double vj = col ? a.v[wo] : 0.0;
        const int yo0 = a.y_off[kk];
        const int nc = stg ? a.y_off[kk + 1] - yo0 : 0;
        const long long yo = (long long)b * sh.ny + yo0;
        const double *Dk = a.D + (long long)b * sh.ndD + a.d_off[kk];
        double acc = 0.0;
        for (int r = 0; r < a.max_nc; ++r) {  // uniform
            const bool row = r < nc;
            const double d = (row && col) ? Dk[r + j * nc] : 0.0;
            const double rv = as_stage_sum<LPS>(d * vj);
            if (row) {
                const bool on = a.act[yo + r] != 0.0;
                double e = a.eta[yo + r];  // (every lane of the stage reads it before lane 0 stores)
                if (on) {
                    e = e + rv / a.delta;
                    mdv = fmax(mdv, fabs(rv));
                    if (j == 0) a.eta[yo + r] = e;
                }
                acc += d * e;
            }
        }
        if (col) {
            if (a.rhs) a.rhs[wo] = (a.gt[wo] - a.delta * vj) + acc;
            if (last) {
                mv = fmax(mv, fabs(vj));
                mch = fmax(mch, fabs(vj - (a.vprev ? a.vprev[wo] : 0.0)));
            }
        }
    }
    if (last) {
        __shared__ double red[4][3];
        mdv = as_wave_max(mdv);
        mv = as_wave_max(mv);
        mch = as_wave_max(mch);
        if (lane == 0) {
            red[wv][0] = mdv;
            red[wv][1] = mv;
            red[wv][2] = mch;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
#pragma unroll
            for (int q = 1; q < 4; ++q) {
                mdv = fmax(mdv, red[q][0]);
                mv = fmax(mv, red[q][1]);
                mch = fmax(mch, red[q][2]);
            }
            a.resid[2 * (long long)b] = mv > 0.0 ? mdv / mv : 0.0;
            a.resid[2 * (long long)b + 1] = mv > 0.0 ? mch / mv : 0.0;
            a.stat[b] = a.fstat[b] != 0 ? PDPLQR_ADMM_ADJOINT_FAILED
                                        : (a.pstat[b] == PDPLQR_POLISH_ACCEPTED ? PDPLQR_ADMM_ADJOINT_EXACT
                                                                                : PDPLQR_ADMM_ADJOINT_APPROX);
        }
    }
}

__global__ __launch_bounds__(256) void k_asadj_rows(AsadjRowsArgs A) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const Shape &sh = A.sh;
    const int n = sh.n, s = sh.s, N = sh.N;
    const int ts = A.ts, tiles = (N + ts) / ts;  // stages 0 .. N
    const long long b = blockIdx.x / tiles;
    const int k0 = (int)(blockIdx.x - b * tiles) * ts;
    const int T = min(ts, N + 1 - k0);
    const int tid = threadIdx.x;

    double *sw = lds, *sv = sw + ts * s;                   // w~, v of stages k0 .. k0 + T - 1
    double *a1 = sv + ts * s, *a2 = a1 + A.max_rows;       // y_a, eta + gvs
    double *sl = a2 + A.max_rows, *su = sl + A.max_rows;   // grad lb, grad ub
    int *yo = reinterpret_cast<int *>(su + A.max_rows);    // y_off[k0 + i] - y_off[k0], i = 0 .. T
    int *dofs = yo + ts + 1;                               // d_off likewise

    const int y0 = A.y_off[k0], d0 = A.d_off[k0];
    if (tid <= T) {
        yo[tid] = A.y_off[k0 + tid] - y0;
        dofs[tid] = A.d_off[k0 + tid] - d0;
    }
    if (A.gD) {
        const double *wb = A.ws + b * sh.perh + (long long)k0 * s, *vb = A.v + b * sh.perh + (long long)k0 * s;
        const int cnt = min((k0 + T) * s, N * s + n) - k0 * s;  // the terminal has no u part
        for (int e = tid; e < cnt; e += 256) {
            sv[e] = vb[e];
            sw[e] = wb[e];
        }
    }
    __syncthreads();
    const int rows = yo[T], dcnt = dofs[T];
    for (int row = tid; row < rows; row += 256) {
        const long long q = b * sh.ny + y0 + row;
        const bool on = A.act[q] != 0.0;
        const bool lower = on && A.bt[q] == A.lb[q];
        const double e = A.eta[q];  // (zero off the active rows)
        a1[row] = on ? A.y[q] : 0.0;
        a2[row] = A.gvs ? e + A.gvs[q] : e;
        sl[row] = lower ? -e : 0.0;
        su[row] = (on && !lower) ? -e : 0.0;
    }
    __syncthreads();

    if (A.gD) {
        int kk = 0;
        as_store_run(A.gD + b * sh.ndD + d0, dcnt, A.vecD != 0, [&](int e) {
            while (e >= dofs[kk + 1]) ++kk;  // e < dofs[T]: kk < T, and the stage has rows
            const int nc = yo[kk + 1] - yo[kk], le = e - dofs[kk], j = le / nc, row = yo[kk] + (le - j * nc);
            return a1[row] * sv[kk * s + j] + a2[row] * sw[kk * s + j];
        });
    }
    if (A.glb) as_store_run(A.glb + b * sh.ny + y0, rows, A.vecY != 0, [&](int e) { return sl[e]; });
    if (A.gub) as_store_run(A.gub + b * sh.ny + y0, rows, A.vecY != 0, [&](int e) { return su[e]; });
}

int launch_asadj_step(const AsadjStepArgs &a, hipStream_t st) {
    const Shape &sh = a.sh;
    if (sh.s > 64) return PDPLQR_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)sh.batch), blk(256);
    if (sh.s <= 16) hipLaunchKernelGGL((k_asadj_step<16>), grid, blk, 0, st, a);
    else if (sh.s <= 32) hipLaunchKernelGGL((k_asadj_step<32>), grid, blk, 0, st, a);
    else hipLaunchKernelGGL((k_asadj_step<64>), grid, blk, 0, st, a);
    PDPLQR_HIP_TRY(hipGetLastError());
    return PDPLQR_OK;
}

int launch_asadj_rows(const AsadjRowsArgs &a0, const int32_t *y_off_h, const int32_t *d_off_h, hipStream_t st) {
    AsadjRowsArgs a = a0;
    const Shape &sh = a.sh;
    if (sh.ny == 0 || (!a.gD && !a.glb && !a.gub)) return PDPLQR_OK;
    const long long tiles = (sh.N + a.ts) / a.ts, blocks = tiles * sh.batch;
    if (blocks > 0x7fffffffLL) {
        set_error("admm_adjoint: batch * stage tiles exceeds the grid limit");
        return PDPLQR_ERR_UNSUPPORTED;
    }
    // a tile's run starts at (b * per + off[k0]) doubles: 16-byte aligned for every block?
    auto al = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    bool evD = sh.batch == 1 || sh.ndD % 2 == 0, evY = sh.batch == 1 || sh.ny % 2 == 0;
    for (int k0 = 0; k0 <= sh.N; k0 += a.ts) {
        evD = evD && d_off_h[k0] % 2 == 0;
        evY = evY && y_off_h[k0] % 2 == 0;
    }
    a.vecD = evD && al(a.gD);
    a.vecY = evY && al(a.glb) && al(a.gub);
    const size_t lds = adjoint_rows_lds_bytes(sh, a.ts, a.max_rows);
    hipLaunchKernelGGL(k_asadj_rows, dim3((unsigned)blocks), dim3(256), lds, st, a);
    PDPLQR_HIP_TRY(hipGetLastError());
    return PDPLQR_OK;
}

}  // namespace pdplqr
