// kernels_adjoint_rows.hip -- gradients of the constraint rows of the penalised
// x-update (pdplqr_adjoint_rows, adjoint.hip).  New: the reference has no such
// call.
//
// The handle factored H~_k = H_k + sigma I + D_k^T R D_k, h~_k = h_k - sigma w_k
// - D_k^T R g_k (R = diag(rho)).  With the primal solution w, the adjoint
// solution v (right-hand side gws + D^T gvs) and, per row of stage k,
//     r = D_k v_k,   e = D_k w_k - g_k
// the chain rule through H~ (grad H~ = sym(v w^T)) and h~ (grad h~ = v) gives
//     grad D_k = (rho o e) v_k^T + (rho o r + gvs_k) w_k^T      (nc_k x dim_k)
//     grad g   = -rho o r          grad rho = r o e  (g held fixed)
// Every (problem, stage) is independent.  Like k_adjoint_grad this is a store
// stream: D is read once (the two row products), grad D written once.  The
// blocks of consecutive stages are contiguous in D, g and rho, so a 256-thread
// block takes a tile of `ts` stages (the terminal is stage N, of width n),
// keeps w, v and the row results in LDS and writes each output's tile as ONE
// flat run, 16 bytes per lane where the run starts 16-byte aligned, 8 bytes
// otherwise.  Rows are ragged (any nc_k, 0 included): the tile's slices of the
// handle's d_off / y_off tables sit in LDS and every lane walks them forwards
// as its flat index grows.  No atomics; contraction is off, so a value does
// not depend on which outputs were requested.
#include <algorithm>

#include "adjoint.hpp"
#include "device_common.hpp"

namespace pdplqr {

// dst[0 .. cnt) = val(e), e ascending per lane
template <class F>
__device__ __forceinline__ void store_run_rows(double *dst, int cnt, bool vec, F &&val) {
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

__global__ __launch_bounds__(256) void k_adjoint_rows(AdjointRowsArgs A) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const Shape &sh = A.sh;
    const int n = sh.n, s = sh.s, N = sh.N;
    const int ts = A.ts, tiles = (N + ts) / ts;  // stages 0 .. N
    const long long b = blockIdx.x / tiles;
    const int k0 = (int)(blockIdx.x - b * tiles) * ts;
    const int T = min(ts, N + 1 - k0);
    const int tid = threadIdx.x;
    const bool need_e = A.gD || A.grho;

    double *sw = lds, *sv = sw + ts * s;                   // w, v of stages k0 .. k0 + T - 1
    double *a1 = sv + ts * s, *a2 = a1 + A.max_rows;       // rho o e, rho o r + gvs
    double *sg = a2 + A.max_rows, *sr = sg + A.max_rows;   // grad g, grad rho
    int *yo = reinterpret_cast<int *>(sr + A.max_rows);    // y_off[k0 + i] - y_off[k0], i = 0 .. T
    int *dofs = yo + ts + 1;                               // d_off likewise

    const int y0 = A.y_off[k0], d0 = A.d_off[k0];
    if (tid <= T) {
        yo[tid] = A.y_off[k0 + tid] - y0;
        dofs[tid] = A.d_off[k0 + tid] - d0;
    }
    {
        const double *wb = A.ws + b * sh.perh + (long long)k0 * s, *vb = A.v + b * sh.perh + (long long)k0 * s;
        const int cnt = min((k0 + T) * s, N * s + n) - k0 * s;  // the terminal has no u part
        for (int e = tid; e < cnt; e += 256) {
            sv[e] = vb[e];
            if (need_e) sw[e] = wb[e];
        }
    }
    __syncthreads();
    const int rows = yo[T], dcnt = dofs[T];
    const double *Db = A.D + b * sh.ndD + d0;
    // G = A.lanes adjacent lanes share a row: lane c of the group takes columns
    // c, c + G, ... and an xor butterfly leaves the same sum in all of them
    // (a wave's loads of one column step then cover whole runs of D)
    const int G = A.lanes, lg = tid & (G - 1), gsh = __builtin_ctz(G);
    for (int base = 0; base < rows * G; base += 256) {  // block-uniform trip count
        const int row = (base + tid) >> gsh;
        const bool on = row < rows;
        int kk = 0;
        double ar = 0.0, aw = 0.0;
        if (on) {
            while (row >= yo[kk + 1]) ++kk;  // row < yo[T]: kk < T
            const int nc = yo[kk + 1] - yo[kk], r = row - yo[kk], dim = k0 + kk < N ? s : n;
            const double *Dk = Db + dofs[kk] + r, *vk = sv + kk * s, *wk = sw + kk * s;
            for (int j = lg; j < dim; j += G) {
                const double d = Dk[(long long)j * nc];
                ar += d * vk[j];
                if (need_e) aw += d * wk[j];
            }
        }
        for (int mask = 1; mask < G; mask <<= 1) {
            ar += __shfl_xor(ar, mask, 64);
            aw += __shfl_xor(aw, mask, 64);
        }
        if (!on || lg) continue;
        const long long q = b * sh.ny + y0 + row;
        const double rho = A.rho[q], e = need_e ? aw - A.g[q] : 0.0, gv = A.gvs ? A.gvs[q] : 0.0;
        const double pr = rho * ar;
        a1[row] = rho * e;
        a2[row] = pr + gv;
        sg[row] = -pr;
        sr[row] = ar * e;
    }
    __syncthreads();

    if (A.gD) {
        int kk = 0;
        store_run_rows(A.gD + b * sh.ndD + d0, dcnt, A.vecD != 0, [&](int e) {
            while (e >= dofs[kk + 1]) ++kk;  // e < dofs[T]: kk < T, and the stage has rows
            const int nc = yo[kk + 1] - yo[kk], le = e - dofs[kk], j = le / nc, row = yo[kk] + (le - j * nc);
            return a1[row] * sv[kk * s + j] + a2[row] * sw[kk * s + j];
        });
    }
    if (A.gg) store_run_rows(A.gg + b * sh.ny + y0, rows, A.vecY != 0, [&](int e) { return sg[e]; });
    if (A.grho) store_run_rows(A.grho + b * sh.ny + y0, rows, A.vecY != 0, [&](int e) { return sr[e]; });
}

// rhs = gws + D^T gvs: one thread per entry of the [N*s + n] vectors
__global__ __launch_bounds__(256) void k_adjoint_rhs(Shape sh, const double *gws, const double *gvs, const double *D,
                                                     const int32_t *d_off, const int32_t *y_off, double *rhs) {
#pragma clang fp contract(off)
    const long long total = sh.perh * sh.batch;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long b = e / sh.perh;
        const int r = (int)(e - b * sh.perh), k = min(r / sh.s, sh.N), j = r - k * sh.s;
        const int yo = y_off[k], nc = y_off[k + 1] - yo;
        const double *Dc = D + b * sh.ndD + d_off[k] + (long long)j * nc, *gv = gvs + b * sh.ny + yo;
        double acc = 0.0;
        for (int i = 0; i < nc; ++i) acc += Dc[i] * gv[i];
        rhs[e] = gws[e] + acc;
    }
}

size_t adjoint_rows_lds_bytes(const Shape &sh, int ts, int max_rows) {
    return sizeof(double) * (2ull * ts * sh.s + 4ull * max_rows) + sizeof(int) * 2ull * (ts + 1);
}

// the most rows of one tile of ts stages (stages 0 .. N)
static int rows_of_tile(const Shape &sh, const int32_t *y_off_h, int ts) {
    int mx = 0;
    for (int k0 = 0; k0 <= sh.N; k0 += ts) mx = std::max(mx, y_off_h[std::min(k0 + ts, sh.N + 1)] - y_off_h[k0]);
    return mx;
}

// stages per block: up to 16, halved until the tile fits 40 KB of LDS; false when
// one stage alone does not (about 1,270 rows on a stage at n + m = 6)
bool adjoint_rows_plan(const Shape &sh, const int32_t *y_off_h, const int32_t *, AdjointRowsArgs &a) {
    int ts = 16;
    auto bytes = [&](int t) { return adjoint_rows_lds_bytes(sh, t, rows_of_tile(sh, y_off_h, t)); };
    while (ts > 1 && (bytes(ts) > 40 * 1024 || ts >= 2 * (sh.N + 1))) ts >>= 1;
    a.sh = sh;
    a.ts = ts;
    a.max_rows = rows_of_tile(sh, y_off_h, ts);
    // lanes per row of the two row products: as many as keep the fullest tile within one pass of the block
    a.lanes = 1;
    while (a.lanes < 16 && a.max_rows * a.lanes * 2 <= 256) a.lanes <<= 1;
    return adjoint_rows_lds_bytes(sh, ts, a.max_rows) <= 40 * 1024;
}

int launch_adjoint_rows(const AdjointRowsArgs &a0, const int32_t *y_off_h, const int32_t *d_off_h, hipStream_t st) {
    AdjointRowsArgs a = a0;
    const Shape &sh = a.sh;
    if (sh.ny == 0 || (!a.gD && !a.gg && !a.grho)) return PDPLQR_OK;
    const long long tiles = (sh.N + a.ts) / a.ts, blocks = tiles * sh.batch;
    if (blocks > 0x7fffffffLL) {
        set_error("adjoint_rows: batch * stage tiles exceeds the grid limit");
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
    a.vecY = evY && al(a.gg) && al(a.grho);
    const size_t lds = adjoint_rows_lds_bytes(sh, a.ts, a.max_rows);
    hipLaunchKernelGGL(k_adjoint_rows, dim3((unsigned)blocks), dim3(256), lds, st, a);
    PDPLQR_HIP_TRY(hipGetLastError());
    return PDPLQR_OK;
}

int launch_adjoint_rhs(const Shape &sh, const double *gws, const double *gvs, const double *D, const int32_t *d_off,
                       const int32_t *y_off, double *rhs, hipStream_t st) {
    const long long total = sh.perh * sh.batch;
    const unsigned blocks = (unsigned)std::min<long long>((total + 255) / 256, 1 << 16);
    hipLaunchKernelGGL(k_adjoint_rhs, dim3(blocks), dim3(256), 0, st, sh, gws, gvs, D, d_off, y_off, rhs);
    PDPLQR_HIP_TRY(hipGetLastError());
    return PDPLQR_OK;
}

}  // namespace pdplqr
