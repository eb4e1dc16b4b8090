// kernels_polish.hip -- the polish of the ADMM outer loop (DESIGN.md section
// 5.8; OSQP: Stellato et al. 2020 section 4) and the KKT measures it is judged
// by, in the coordinates of the dynamics' affine set (the x-update solves the
// dynamics exactly, so only the rows lb <= D w <= ub carry multipliers).
//
//   k_polish_classify  the active-set guess from the ADMM (y, z): per row the
//                      penalty of the polishing x-update (1/delta or 0), its
//                      inverse, the bound b the row is held at, y^0; the count
//                      of active rows per problem.
//   k_polish_ystep     y <- y + (D_a w - b) / delta after each polishing solve
//                      (k_admm_update's layout); also leaves v = D w.
//   k_kkt_grad         the reduced gradient: one wave per problem runs the
//                      costate recursion nu_N = q_N, [g_k ; nu_k] = q_k +
//                      E_k^T nu_{k+1} with q_k = H_k w_k + h_k + D_k^T y_k
//                      (k_infeas_primal's recursion with another q).
//   k_kkt_local        the stage-local measures: the row residual (the natural
//                      map |v - clamp(v + y, lb, ub)|), the dynamics residual
//                      and the objective (k_infeas_dual's layout).
//   k_polish_accept    OSQP's acceptance rule, one thread per problem;
//   k_polish_write     w, y, z = clamp(D w, lb, ub) of the accepted problems.
// The two halves of the measures are separate launches for the reason
// kernels_infeas.hip gives: N dependent steps of one wave against a
// stage-parallel sweep of a block.  Contraction is off: a measure does not
// depend on the kernel instance.  No atomics on measures.  A bound with
// |value| >= 1e20 is infinite.
#include "admm.hpp"
#include "device_common.hpp"

namespace pdplqr {

namespace {

constexpr double kInfBound = 1e20;

__device__ __forceinline__ double pw_max(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
    return v;
}

__device__ __forceinline__ double pw_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

template <int LPS>
__device__ __forceinline__ double pst_sum(double v) {
#pragma unroll
    for (int m = 1; m < LPS; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

}  // namespace

// One 256-thread block per problem striding its rows (coalesced loads and
// stores); the active count reduces over the block (lane butterflies, then
// waves 0..3).  OSQP's rule: lower-active if lb == ub or z - lb < -y, else
// upper-active if ub - z < y.
__global__ __launch_bounds__(256) void k_polish_classify(PolishArgs a) {
#pragma clang fp contract(off)
    const int b = blockIdx.x, ny = a.sh.ny;
    const long long o = (long long)b * ny;
    const double rho_act = 1.0 / a.delta;
    int cnt = 0;
    for (int i = threadIdx.x; i < ny; i += 256) {
        const double l = a.lb[o + i], u = a.ub[o + i], y = a.y[o + i], z = a.z[o + i];
        const bool lower = l == u || z - l < -y;
        const bool upper = !lower && u - z < y;
        const bool act = lower || upper;
        a.rho_p[o + i] = act ? rho_act : 0.0;
        a.irho_p[o + i] = act ? a.delta : 0.0;
        a.bt[o + i] = lower ? l : (upper ? u : 0.0);
        a.yp[o + i] = act ? y : 0.0;
        cnt += act ? 1 : 0;
    }
    __shared__ int red[4];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) a.nact[b] = red[0] + red[1] + red[2] + red[3];
}

// One 256-thread block per problem, LPS lanes per stage (k_admm_update's
// layout): row r of D_k w_k is a butterfly over the stage's lanes; lane 0 of
// the stage stores v and steps y on the active rows (rho_p != 0).
template <int LPS>
__global__ __launch_bounds__(256) void k_polish_ystep(PolishArgs a) {
#pragma clang fp contract(off)
    const Shape &sh = a.sh;
    const int b = blockIdx.x;
    constexpr int SPW = 64 / LPS;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, sub = lane / LPS, j = lane % LPS;
    const int N = sh.N, s = sh.s;
    const double *wb = a.wp + (long long)b * sh.perh;
    for (int kb = wv * SPW; kb <= N; kb += 4 * SPW) {
        // wave-uniform trip count: lanes past the horizon idle in the loop
        const int k = kb + sub;
        const bool stg = k <= N;
        const int kk = stg ? k : N;
        const int dim = kk < N ? s : sh.n;
        const bool col = stg && j < dim;
        const double wj = col ? wb[(long long)kk * s + j] : 0.0;
        const int yo0 = a.uni ? kk * a.uni : a.y_off[kk];
        const int nc = !stg ? 0 : (a.uni ? (kk < N ? a.uni : 0) : a.y_off[kk + 1] - yo0);
        const long long yo = (long long)b * sh.ny + yo0;
        const double *Dk = a.D + (long long)b * sh.ndD + (a.uni ? (long long)kk * a.uni * s : a.d_off[kk]);
        for (int r = 0; r < a.max_nc; ++r) {  // uniform
            const bool row = r < nc;
            const double d = (row && col) ? Dk[r + j * nc] : 0.0;
            const double v = pst_sum<LPS>(d * wj);
            if (row && j == 0) {
                a.vp[yo + r] = v;
                if (a.rho_p[yo + r] != 0.0) a.yp[yo + r] = a.yp[yo + r] + (v - a.bt[yo + r]) / a.delta;
            }
        }
    }
}

// One wave per problem; lane j owns entry j of [g_k ; nu_k] (s <= SB <= 64).
// The loads of a stage -- the lane's column of H (H is symmetric: the column
// is the row, contiguous) and of E, its h and w entries, the first four rows
// of D and y -- go into one of DEPTH + 1 register sets DEPTH stages before
// the stage is processed; the stage loop is unrolled DEPTH + 1 times so that
// every set has a fixed name (k_infeas_primal's scheme).  w_k and nu_{k+1} are
// broadcast through 2 x 64 LDS buffers, one barrier per stage.  SB >= s and
// NB >= n bound the two columns.  DEPTH = 2 for s <= 16, 1 for s <= 32; past
// that two columns are up to 128 doubles and DEPTH = 0 keeps no column: the
// stage's two dot products read theirs in runs of 8 (same order of additions).
template <int SB, int NB, int DEPTH>
__global__ __launch_bounds__(64) void k_kkt_grad(KktArgs a) {
#pragma clang fp contract(off)
    __shared__ double snu[2][64], sw[2][64];
    const Shape &sh = a.sh;
    const int b = blockIdx.x, j = threadIdx.x;
    const int n = sh.n, m = sh.m, s = sh.s, N = sh.N, ny = sh.ny;
    const double *wb = a.w + (long long)b * sh.perh, *hb = a.hv + (long long)b * sh.perh;
    const double *yb = a.y + (long long)b * ny;  // (never read when ny = 0)
    const double *Hb = a.H + (long long)b * sh.perH, *Eb = a.E + (long long)b * sh.perE;
    const double *Db = a.D + (long long)b * sh.ndD;
    snu[0][j] = snu[1][j] = 0.0;
    sw[0][j] = sw[1][j] = 0.0;
    __syncthreads();

    const bool xl = j >= m && j < s;  // the lane holds nu[j - m]
    const int xi = xl ? j - m : 0;
    // terminal: nu_N = q_N = H_N w_N + h_N + D_N^T y_N (H_N is n x n, D_N nc_N x n)
    double v = 0.0;
    if (N == 0) {  // no input stage: nothing to reduce over
        if (j == 0) a.meas[(long long)b * a.mstride + 2] = 0.0;
        return;
    }
    {
        const int yo = a.uni ? N * a.uni : a.y_off[N];
        const int nc = a.uni ? 0 : a.y_off[N + 1] - yo;
        const double *Dk = Db + (a.uni ? (long long)N * a.uni * s : a.d_off[N]);
        if (xl) {
            const double *HN = Hb + (long long)N * s * s + (long long)xi * n, *wN = wb + (long long)N * s;
            double acc = 0.0, q = 0.0;
            for (int i = 0; i < n; ++i) acc += HN[i] * wN[i];
            for (int r = 0; r < nc; ++r) q += Dk[r + xi * nc] * yb[yo + r];
            v = (acc + hb[(long long)N * s + xi]) + q;
        }
    }

    struct Stage {
        double h, w, d[4], y[4];
        int nc, yo;
        const double *Dk;
    };
    const bool col = j < s;
    auto load_cols = [&](int k, double *Hc, double *Ec) {
        const double *Hk = Hb + (long long)k * s * s + (col ? j * s : 0);
        const double *Ek = Eb + (long long)k * n * s + (col ? j * n : 0);
#pragma unroll
        for (int i = 0; i < SB; ++i) Hc[i] = (col && i < s) ? Hk[i] : 0.0;
#pragma unroll
        for (int i = 0; i < NB; ++i) Ec[i] = (col && i < n) ? Ek[i] : 0.0;
    };
    auto load = [&](int k, Stage &st) {
        st.h = col ? hb[(long long)k * s + j] : 0.0;
        st.w = col ? wb[(long long)k * s + j] : 0.0;
        st.yo = a.uni ? k * a.uni : a.y_off[k];
        st.nc = a.uni ? a.uni : a.y_off[k + 1] - st.yo;
        st.Dk = Db + (a.uni ? (long long)k * a.uni * s : a.d_off[k]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool row = r < st.nc;
            st.d[r] = (row && col) ? st.Dk[r + j * st.nc] : 0.0;
            st.y[r] = row ? yb[st.yo + r] : 0.0;
        }
    };

    double gm = 0.0;
    constexpr int SETS = DEPTH + 1;
    Stage st[SETS];
    double Hc[SETS][DEPTH ? SB : 1], Ec[SETS][DEPTH ? NB : 1];
#pragma unroll
    for (int d = 0; d < DEPTH; ++d)
        if (N - 1 - d >= 0) {
            load(N - 1 - d, st[d]);
            load_cols(N - 1 - d, Hc[d], Ec[d]);
        }
    int buf = 0;
    for (int k0 = N - 1; k0 >= 0; k0 -= SETS) {
#pragma unroll
        for (int u = 0; u < SETS; ++u) {
            const int k = k0 - u;
            if (k < 0) break;  // wave-uniform
            const int f = (u + DEPTH) % SETS;  // the set stage k - DEPTH goes to (DEPTH = 0: this stage's own)
            if (k - DEPTH >= 0) {  // independent of the recursion: in flight during DEPTH stages
                load(k - DEPTH, st[f]);
                if constexpr (DEPTH > 0) load_cols(k - DEPTH, Hc[f], Ec[f]);
            }
            const Stage &cur = st[u];
            if (xl) snu[buf][xi] = v;
            sw[buf][j] = cur.w;  // (0 past s)
            __syncthreads();
            double acc = 0.0, ace = 0.0;
            if constexpr (DEPTH > 0) {
#pragma unroll
                for (int i = 0; i < SB; ++i) acc += Hc[u][i] * sw[buf][i];  // entries past s are 0 * 0
#pragma unroll
                for (int i = 0; i < NB; ++i) ace += Ec[u][i] * snu[buf][i];  // entries past n are 0 * 0
            } else {
                const double *Hk = Hb + (long long)k * s * s + (col ? j * s : 0);
                const double *Ek = Eb + (long long)k * n * s + (col ? j * n : 0);
                for (int i0 = 0; i0 < s; i0 += 8) {  // uniform; i0 + 7 <= 63
                    double t[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) t[e] = (col && i0 + e < s) ? Hk[i0 + e] : 0.0;
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc += t[e] * sw[buf][i0 + e];
                }
                for (int i0 = 0; i0 < n; i0 += 8) {
                    double t[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) t[e] = (col && i0 + e < n) ? Ek[i0 + e] : 0.0;
#pragma unroll
                    for (int e = 0; e < 8; ++e) ace += t[e] * snu[buf][i0 + e];
                }
            }
            double q = 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) q += cur.d[r] * cur.y[r];
            if (col)
                for (int r = 4; r < cur.nc; ++r) q += cur.Dk[r + j * cur.nc] * yb[cur.yo + r];
            v = col ? ((acc + cur.h) + q) + ace : 0.0;
            if (j < m) gm = fmax(gm, fabs(v));
            buf ^= 1;
        }
    }
    gm = pw_max(gm);
    if (j == 0) a.meas[(long long)b * a.mstride + 2] = gm;
}

// One 256-thread block per problem, LPS lanes per stage (k_infeas_dual's
// layout).  Lane j of stage k holds w_k[j]; row j of H_k w_k and of E_k w_k are
// sums over i of column i (coalesced over j) times w_k[i], broadcast by a
// shuffle; a row of D_k w_k is a butterfly over the stage's lanes.  The maxima
// and the two sums of the objective reduce over the block in a fixed order
// (lane butterflies, then waves 0..3).
template <int LPS>
__global__ __launch_bounds__(256) void k_kkt_local(KktArgs a) {
#pragma clang fp contract(off)
    const Shape &sh = a.sh;
    const int b = blockIdx.x;
    constexpr int SPW = 64 / LPS;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, sub = lane / LPS, j = lane % LPS;
    const int n = sh.n, m = sh.m, s = sh.s, N = sh.N;
    const double *wb = a.w + (long long)b * sh.perh, *hb = a.hv + (long long)b * sh.perh;
    const double *cb = a.c + (long long)b * sh.perc;
    double rowm = 0.0, dyn = 0.0, qs = 0.0, ls = 0.0;
    for (int kb = wv * SPW; kb <= N; kb += 4 * SPW) {
        // wave-uniform trip count: lanes past the horizon idle in the loop
        const int k = kb + sub;
        const bool stg = k <= N;
        const int kk = stg ? k : N;
        const int dim = kk < N ? s : n;
        const bool col = stg && j < dim;
        const long long wo = (long long)kk * s + (j < dim ? j : 0);
        const double wj = col ? wb[wo] : 0.0;
        if (col) ls += hb[wo] * wj;
        const double *Hk = a.H + (long long)b * sh.perH + (long long)kk * s * s;
        const bool dy = stg && kk < N && j < n;
        const double *Ek = a.E + (long long)b * sh.perE + (long long)(dy ? kk : 0) * n * s;
        double hacc = 0.0, eacc = 0.0;
        for (int i = 0; i < s; ++i) {  // uniform; s <= LPS
            const double wi = __shfl(wj, sub * LPS + i, 64);
            if (col && i < dim) hacc += Hk[j + i * dim] * wi;
            if (dy) eacc += Ek[j + i * n] * wi;
        }
        qs += wj * hacc;
        if (dy) {
            const long long xo = kk + 1 < N ? (long long)(kk + 1) * s + m + j : (long long)N * s + j;
            dyn = fmax(dyn, fabs((wb[xo] - eacc) - cb[(long long)kk * n + j]));  // x_{k+1} - E_k w_k - c_k
        }
        {  // x_0 - x0 (x_0 sits behind u_0; a horizon of 0 has only x_0)
            const int xj = N > 0 ? j - m : j;
            if (stg && kk == 0 && xj >= 0 && xj < n) dyn = fmax(dyn, fabs(wj - a.x0[(long long)b * n + xj]));
        }
        const int yo0 = a.uni ? kk * a.uni : a.y_off[kk];
        const int nc = !stg ? 0 : (a.uni ? (kk < N ? a.uni : 0) : a.y_off[kk + 1] - yo0);
        const long long yo = (long long)b * sh.ny + yo0;
        const double *Dk = a.D + (long long)b * sh.ndD + (a.uni ? (long long)kk * a.uni * s : a.d_off[kk]);
        for (int r = 0; r < a.max_nc; ++r) {  // uniform
            const bool row = r < nc;
            const double d = (row && col) ? Dk[r + j * nc] : 0.0;
            const double v = pst_sum<LPS>(d * wj);
            if (row) {
                const double l = a.lb[yo + r], u = a.ub[yo + r];
                const double lo = l <= -kInfBound ? -__builtin_inf() : l, hi = u >= kInfBound ? __builtin_inf() : u;
                rowm = fmax(rowm, fabs(v - fmin(fmax(v + a.y[yo + r], lo), hi)));
            }
        }
    }
    __shared__ double red[4][4];
    rowm = pw_max(rowm);
    dyn = pw_max(dyn);
    qs = pw_sum(qs);
    ls = pw_sum(ls);
    if (lane == 0) {
        red[wv][0] = rowm;
        red[wv][1] = dyn;
        red[wv][2] = qs;
        red[wv][3] = ls;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 1; q < 4; ++q) {
            rowm = fmax(rowm, red[q][0]);
            dyn = fmax(dyn, red[q][1]);
            qs += red[q][2];
            ls += red[q][3];
        }
        double *ms = a.meas + (long long)b * a.mstride;
        ms[0] = rowm;
        ms[1] = dyn;
        ms[3] = 0.5 * qs + ls;
    }
}

// OSQP's acceptance rule with its constants, one thread per problem, on the
// measures of the ADMM iterate (meas[0..3]) and of the polished pair
// (meas[4..7]): pri = max(row, dynamics), dua = reduced gradient.  A problem
// that did not end SOLVED is not attempted (0).  Rejected (2) without looking:
// a failed polish factorisation (fst1: S1 flags per problem, fst2: one; both
// nullable), or a non-finite polished objective (fmax drops a NaN, a sum keeps it).
__global__ void k_polish_accept(int batch, const int32_t *__restrict__ conv, const double *__restrict__ meas,
                                const int32_t *__restrict__ fst1, int S1, const int32_t *__restrict__ fst2,
                                int32_t *__restrict__ pstat) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    int st = 0;
    if (conv[b] == 1) {
        const double *ms = meas + (long long)b * 8;
        const double pri = fmax(ms[0], ms[1]), dua = ms[2], pri_p = fmax(ms[4], ms[5]), dua_p = ms[6];
        bool ok = ms[7] - ms[7] == 0.0;  // finite
        if (fst1)
            for (int i = 0; i < S1; ++i) ok = ok && fst1[(long long)b * S1 + i] == 0;
        if (fst2) ok = ok && fst2[b] == 0;
        const bool acc = (pri_p < pri && dua_p < dua) || (pri_p < pri && dua < 1e-10) || (dua_p < dua && pri < 1e-10);
        st = ok && acc ? 1 : 2;
    }
    pstat[b] = st;
}

// w, y and z = clamp(D w, lb, ub) of the accepted problems; the rest keep
// their ADMM iterate bit for bit
__global__ void k_polish_write(long long w_total, long long perh, long long ny_total, int ny,
                               const int32_t *__restrict__ pstat, const double *__restrict__ wp,
                               const double *__restrict__ yp, const double *__restrict__ vp,
                               const double *__restrict__ lb, const double *__restrict__ ub, double *__restrict__ w,
                               double *__restrict__ y, double *__restrict__ z) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < w_total) {
        if (pstat[t / perh] == 1) w[t] = wp[t];
    } else if (t - w_total < ny_total) {
        const long long q = t - w_total;
        if (pstat[q / ny] == 1) {
            y[q] = yp[q];
            z[q] = fmin(fmax(vp[q], lb[q]), ub[q]);
        }
    }
}

int launch_polish_classify(const PolishArgs &a, hipStream_t st) {
    if (a.sh.ny <= 0) return PDPLQR_OK;
    hipLaunchKernelGGL(k_polish_classify, dim3((unsigned)a.sh.batch), dim3(256), 0, st, a);
    PDPLQR_HIP_TRY(hipGetLastError());
    return PDPLQR_OK;
}

int launch_polish_ystep(const PolishArgs &a, hipStream_t st) {
    const Shape &sh = a.sh;
    if (!infeas_shape_supported(sh)) return PDPLQR_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)sh.batch), blk(256);
    if (sh.s <= 16) hipLaunchKernelGGL((k_polish_ystep<16>), grid, blk, 0, st, a);
    else if (sh.s <= 32) hipLaunchKernelGGL((k_polish_ystep<32>), grid, blk, 0, st, a);
    else hipLaunchKernelGGL((k_polish_ystep<64>), grid, blk, 0, st, a);
    PDPLQR_HIP_TRY(hipGetLastError());
    return PDPLQR_OK;
}

int launch_kkt_residual(const KktArgs &a, hipStream_t st) {
    const Shape &sh = a.sh;
    if (!infeas_shape_supported(sh)) return PDPLQR_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)sh.batch);
    if (sh.s <= 16) hipLaunchKernelGGL((k_kkt_grad<16, 16, 2>), grid, dim3(64), 0, st, a);
    else if (sh.s <= 32 && sh.n <= 16) hipLaunchKernelGGL((k_kkt_grad<32, 16, 1>), grid, dim3(64), 0, st, a);
    else if (sh.s <= 32) hipLaunchKernelGGL((k_kkt_grad<32, 32, 1>), grid, dim3(64), 0, st, a);
    else hipLaunchKernelGGL((k_kkt_grad<64, 64, 0>), grid, dim3(64), 0, st, a);
    if (sh.s <= 16) hipLaunchKernelGGL((k_kkt_local<16>), grid, dim3(256), 0, st, a);
    else if (sh.s <= 32) hipLaunchKernelGGL((k_kkt_local<32>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_kkt_local<64>), grid, dim3(256), 0, st, a);
    PDPLQR_HIP_TRY(hipGetLastError());
    return PDPLQR_OK;
}

int launch_polish_accept(int batch, const int32_t *conv, const double *meas, const int32_t *fst1, int S1,
                         const int32_t *fst2, int32_t *pstat, hipStream_t st) {
    hipLaunchKernelGGL(k_polish_accept, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, st, batch, conv, meas,
                       fst1, S1, fst2, pstat);
    PDPLQR_HIP_TRY(hipGetLastError());
    return PDPLQR_OK;
}

int launch_polish_write(const Shape &sh, const int32_t *pstat, const double *wp, const double *yp, const double *vp,
                        const double *lb, const double *ub, double *w, double *y, double *z, hipStream_t st) {
    const long long W = (long long)sh.batch * sh.perh, Y = (long long)sh.batch * sh.ny;
    hipLaunchKernelGGL(k_polish_write, dim3((unsigned)((W + Y + 255) / 256)), dim3(256), 0, st, W, sh.perh, Y,
                       sh.ny > 0 ? sh.ny : 1, pstat, wp, yp, vp, lb, ub, w, y, z);
    PDPLQR_HIP_TRY(hipGetLastError());
    return PDPLQR_OK;
}

}  // namespace pdplqr
