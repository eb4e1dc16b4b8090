// kernels_adjoint.hip -- parameter gradients of the batched serial LQ solve
// (pdplqr_adjoint, adjoint.hip).  New: the reference has no such call.
//
// Given the primal solution w, the adjoint solution v (a second solve on the
// cached factor with h~ := dl/dw, c := 0, x0 := 0) and the value-function
// vectors p_k, p^_k of both solves, every (problem, stage k) is independent:
//     lambda_{k+1} = Lxx_{k+1} (Lxx_{k+1}^T x_{k+1})   + p_{k+1}
//     mu_{k+1}     = Lxx_{k+1} (Lxx_{k+1}^T v_{x,k+1}) + p^_{k+1}
//     grad h_k = v_k                       grad H_k = (v_k w_k^T + w_k v_k^T) / 2
//     grad c_k = mu_{k+1}                  grad E_k = mu_{k+1} w_k^T + lambda_{k+1} v_k^T
// plus grad H_N, grad h_N at the terminal and grad x0 = p^_0.
//
// The kernel is a store stream: per stage it writes s^2 + n s + n + s doubles
// and reads 2 s + 2 n + n (n + 1) / 2 (3.8 KB against 1.1 KB at 12/4).  The
// outputs of consecutive stages of one problem are contiguous in every
// gradient array, so a 256-thread block takes a tile of `ts` stages, stages
// its inputs and the costates in LDS, and then writes each array's tile as ONE
// flat run: lane t stores elements [2 t, 2 t + 1] (one 16-byte store, 1 KiB
// contiguous per wave instruction) and derives (stage, row, column) from the
// flat index.  VEC needs n and m even (no pair straddles a column or a stage,
// every per-problem block starts 16-byte aligned) and aligned output
// pointers; otherwise the same runs go out as 8-byte stores, still contiguous
// across the wave.  NN, MM > 0 fix the shape at compile time (the index
// divisions become multiplies); NN = 0 reads it from Shape.
#include <algorithm>

#include "adjoint.hpp"
#include "adjoint_store.hpp"
#include "device_common.hpp"

namespace pdplqr {

template <int NN, int MM, bool VEC>
__global__ __launch_bounds__(256) void k_adjoint_grad(AdjointArgs A) {
#pragma clang fp contract(off)  // v_i w_j + w_i v_j rounds the same way as its transpose: grad H is exactly symmetric
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const Shape &sh = A.sh;
    const int n = NN ? NN : sh.n, m = NN ? MM : sh.m, s = n + m, N = sh.N;
    const int pn = n * (n + 1) / 2, ps = s * (s + 1) / 2;
    const int ts = A.ts, tiles = (N + ts - 1) / ts;
    const long long b = blockIdx.x / tiles;
    const int k0 = (int)(blockIdx.x - b * tiles) * ts;
    const int T = min(ts, N - k0);
    const bool last = k0 + T == N;
    const int tid = threadIdx.x;
    const bool need_mu = A.gE || A.gc, need_lam = A.gE != nullptr;

    double *sw = lds, *sv = sw + (ts + 1) * s;  // w, v of stages k0 .. k0 + T
    double *sL = sv + (ts + 1) * s;             // packed Lxx of stages k0 + 1 .. k0 + T
    double *sp = sL + ts * pn, *sq = sp + ts * n;        // p, p^
    double *stx = sq + ts * n, *stv = stx + ts * n;      // Lxx^T x, Lxx^T v_x
    double *slam = stv + ts * n, *smu = slam + ts * n;   // costates

    // offset of x_kk (and of p_kk in lp) in a [N*s + n] vector; the terminal has no u part
    auto xoff = [&](int kk) { return kk * s + (kk < N ? m : 0); };

    const double *wb = A.ws + b * sh.perh, *vb = A.v + b * sh.perh;
    {
        const int cnt = T * s + (last ? n : s);
        for (int e = tid; e < cnt; e += 256) {
            sw[e] = wb[(long long)k0 * s + e];
            sv[e] = vb[(long long)k0 * s + e];
        }
    }
    if (need_mu) {
        const double *Lb = A.Lc + b * sh.perHw;
        // Lxx_kk: the last pn entries of stage kk's packed block (columns m .. s - 1
        // of a packed-lower s x s are a packed-lower n x n); the whole block at kk = N
        for (int e = tid; e < T * pn; e += 256) {
            const int j = e / pn, q = e - j * pn, kk = k0 + 1 + j;
            sL[e] = Lb[(long long)kk * ps + (kk < N ? ps - pn : 0) + q];
        }
        const double *pb = A.lpc + b * sh.perh, *qb = A.lpa + b * sh.perh;
        for (int e = tid; e < T * n; e += 256) {
            const int j = e / n, i = e - j * n, o = xoff(k0 + 1 + j) + i;
            sq[e] = qb[o];
            if (need_lam) sp[e] = pb[o];
        }
    }
    __syncthreads();
    if (need_mu) {
        for (int e = tid; e < T * n; e += 256) {  // t = Lxx^T x: t_c = sum_{i >= c} L[i][c] x_i
            const int j = e / n, c = e - j * n, kk = k0 + 1 + j;
            const double *L = sL + j * pn + pidx(c, c, n) - c;  // L[i] = Lxx[i][c]
            const int xo = xoff(kk) - k0 * s;
            double ax = 0.0, av = 0.0;
            for (int i = c; i < n; ++i) {
                av += L[i] * sv[xo + i];
                if (need_lam) ax += L[i] * sw[xo + i];
            }
            stv[e] = av;
            stx[e] = ax;
        }
        __syncthreads();
        for (int e = tid; e < T * n; e += 256) {  // Lxx t: sum_{c <= i} L[i][c] t_c
            const int j = e / n, i = e - j * n;
            const double *L = sL + j * pn;
            double ax = 0.0, av = 0.0;
            for (int c = 0; c <= i; ++c) {
                const double l = L[pidx(i, c, n)];
                av += l * stv[j * n + c];
                if (need_lam) ax += l * stx[j * n + c];
            }
            smu[e] = av + sq[e];
            if (need_lam) slam[e] = ax + sp[e];
        }
        __syncthreads();
    }

    if (A.gH) {
        const int ss = s * s;
        store_run<VEC>(A.gH + b * sh.perH + (long long)k0 * ss, T * ss + (last ? n * n : 0), [&](int e) {
            const int kk = e / ss, r = e - kk * ss, d = kk < T ? s : n;  // kk == T: the terminal's n x n
            const int j = kk < T ? r / s : r / n, i = r - j * d, o = kk * s;
            return 0.5 * (sv[o + i] * sw[o + j] + sw[o + i] * sv[o + j]);
        });
    }
    if (A.gE) {
        const int ns = n * s;
        store_run<VEC>(A.gE + b * sh.perE + (long long)k0 * ns, T * ns, [&](int e) {
            const int kk = e / ns, r = e - kk * ns, j = r / n, i = r - j * n;
            return smu[kk * n + i] * sw[kk * s + j] + slam[kk * n + i] * sv[kk * s + j];
        });
    }
    if (A.gc) store_run<VEC>(A.gc + b * sh.perc + (long long)k0 * n, T * n, [&](int e) { return smu[e]; });
    if (A.gh)
        store_run<VEC>(A.gh + b * sh.perh + (long long)k0 * s, T * s + (last ? n : 0), [&](int e) { return sv[e]; });
    if (A.gx && k0 == 0 && tid < n) A.gx[b * n + tid] = A.lpa[b * sh.perh + m + tid];  // mu_0 = p^_0
}

// lu'_k of the rollout record (m doubles per stage) to `buf` (save) or back
__global__ __launch_bounds__(256) void k_adjoint_lu(Shape sh, double *KD, double *buf, int restore) {
    const long long per = (long long)sh.N * sh.m, total = per * sh.batch;
    const long long frs = (long long)sh.s * sh.m + sh.m;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long b = e / per, r = e - b * per, k = r / sh.m, i = r - k * sh.m;
        double *rec = KD + b * sh.perKD + k * frs + (long long)sh.s * sh.m + i;
        if (restore) *rec = buf[e];
        else buf[e] = *rec;
    }
}

size_t adjoint_lds_bytes(const Shape &sh, int ts) {
    return sizeof(double) * (2ull * (ts + 1) * sh.s + (size_t)ts * (sh.pn + 6 * sh.n));
}

// stages per block: up to 16, halved until the tile fits 40 KB of LDS (n + m <= 64: one stage always does)
int adjoint_tile(const Shape &sh) {
    int ts = 16;
    while (ts > 1 && (adjoint_lds_bytes(sh, ts) > 40 * 1024 || ts >= 2 * sh.N)) ts >>= 1;
    return ts;
}

int launch_adjoint_grad(const AdjointArgs &a0, hipStream_t st) {
    AdjointArgs a = a0;
    const Shape &sh = a.sh;
    if (!a.gE && !a.gc && !a.gH && !a.gh && !a.gx) return PDPLQR_OK;
    a.ts = adjoint_tile(sh);
    const long long tiles = (sh.N + a.ts - 1) / a.ts, blocks = tiles * sh.batch;
    if (blocks > 0x7fffffffLL) {
        set_error("adjoint: batch * stage tiles exceeds the grid limit");
        return PDPLQR_ERR_UNSUPPORTED;
    }
    auto al = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    const bool vec = sh.n % 2 == 0 && sh.m % 2 == 0 && al(a.gE) && al(a.gc) && al(a.gH) && al(a.gh);
    const dim3 grid((unsigned)blocks), blk(256);
    const size_t lds = adjoint_lds_bytes(sh, a.ts);
    if (vec && sh.n == 12 && sh.m == 4) hipLaunchKernelGGL((k_adjoint_grad<12, 4, true>), grid, blk, lds, st, a);
    else if (vec) hipLaunchKernelGGL((k_adjoint_grad<0, 0, true>), grid, blk, lds, st, a);
    else hipLaunchKernelGGL((k_adjoint_grad<0, 0, false>), grid, blk, lds, st, a);
    PDPLQR_HIP_TRY(hipGetLastError());
    return PDPLQR_OK;
}

int launch_adjoint_lu(const Shape &sh, double *KD, double *buf, bool restore, hipStream_t st) {
    const long long total = (long long)sh.batch * sh.N * sh.m;
    const unsigned blocks = (unsigned)std::min<long long>((total + 255) / 256, 1 << 16);
    hipLaunchKernelGGL(k_adjoint_lu, dim3(blocks), dim3(256), 0, st, sh, KD, buf, restore ? 1 : 0);
    PDPLQR_HIP_TRY(hipGetLastError());
    return PDPLQR_OK;
}

}  // namespace pdplqr
