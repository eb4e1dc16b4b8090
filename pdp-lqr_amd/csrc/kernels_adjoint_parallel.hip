// kernels_adjoint_parallel.hip -- the costates of a segmented (PARALLEL) solve
// and the gradient pass on them (pdplqr_adjoint_parallel, adjoint_parallel.hip).
// New: the reference has no such call.
//
// A PARALLEL handle caches, per stage, the value function of the stage's own
// device segment under a free segment end (kernels_segment.hip: P_k packed in
// Lc, p_k in lpc), not the global one.  With y the costate at the segment's
// end, the cost-to-go of stage k inside the segment is
//     1/2 x^T P_k x + p_k^T x + y^T (F_k x + f_k) - 1/2 y^T C_k y,
// so the stage costate is
//     lambda_k = P_k x_k + p_k + t_k,   t_k = F_k^T y = Acl_k^T t_{k+1},  t_end = y,
// with Acl_k = A_k + B_k K_k the segment's closed loop.  F_k is not stored;
// t is carried down the segment from the rollout record [L(:, 0:m) | lu']:
//     r = E_k^T t_{k+1},   z = Luu^{-1} r_u,   t_k = r_x - Lxu z
// (K = -Luu^{-T} Lxu^T: this is k_seg_bwd_nofact's p recursion with h~ = 0,
// c = 0 and P = 0).  P_k x_k + p_k is formed afresh at every stage and t only
// passes through closed-loop maps, so rounding does not grow along a segment
// as it does in lambda_k = [H~ w + h~]_x + A_k^T lambda_{k+1} (norm(A^T)^L).
// y comes from the suffix scan: y = P_j x + p_j at the start of segment j; the
// last segment ends at the terminal (lambda_N = H~_N x_N + h~_N, t = 0).
// The adjoint solve's mu follows the same recursion with (v, lpa, its scan).
//
// k_seg_costate: one wave per (problem, device segment), all segments at once.
// Per stage it reads E_k (n s), L_k (s m), P_k (pn) and 4 n vector entries and
// writes 2 n.  The three blocks are contiguous in their arrays: the wave loads
// them flat (lane + 64 r, each block padded to whole rounds of 64 so that a
// register belongs to one block) one stage ahead, so the loads fly during the
// stage before, and drops them into LDS in the same order at the top of their
// stage.  Lane j < s owns entry j of r = E^T t and reads column j of E; with
// an even n the lanes start their column at different rows (i + j mod n), which
// spreads the column pitch over the LDS banks.  The m steps of the forward
// substitution broadcast r_i with readlane and update the lanes below, which
// leaves t_k on lanes m .. s - 1.  Lane i < n then forms row i of P_k x_k from
// the packed triangle.
#include "adjoint.hpp"
#include "adjoint_store.hpp"
#include "device_common.hpp"

namespace pdplqr {

// rounds of 64 of the stage's E, L and P blocks
struct CostateRounds {
    int e, l, p;
};
__host__ __device__ static inline CostateRounds costate_rounds(const Shape &sh) {
    return {(sh.n * sh.s + 63) >> 6, (sh.s * sh.m + 63) >> 6, (sh.pn + 63) >> 6};
}

static size_t seg_costate_lds_doubles(const Shape &sh) {
    const CostateRounds r = costate_rounds(sh);
    return 64 * (size_t)(r.e + r.l + r.p + 4);
}

template <int SB>  // SB >= n + m: 16, 32 or 64
__global__ __launch_bounds__(64) void k_seg_costate(SegCostateArgs A) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double lds[];
    // registers of one stage: s^2 + pn doubles in rounds of 64, each block rounded up
    constexpr int C = (SB * SB + SB * (SB + 1) / 2 + 63) / 64 + 2;
    const int lane = wave_lane();
    const Shape &sh = A.sh;
    const int n = sh.n, m = sh.m, s = sh.s, S = A.S, N = sh.N, pn = sh.pn;
    const int nE = n * s, nL = s * m;
    const CostateRounds rd = costate_rounds(sh);
    const int rE = rd.e, rEL = rd.e + rd.l, rELP = rEL + rd.p;
    double *sE = lds, *sL = sE + 64 * rE, *sP = sE + 64 * rEL;
    double *sx = sE + 64 * rELP, *sv = sx + 64, *stl = sv + 64, *stm = stl + 64;
    const long long b = blockIdx.x / S;
    const int seg = blockIdx.x % S;
    const int N0 = A.seg_start[seg], N1 = N0 + A.seg_len[seg];
    const bool last = seg == S - 1;  // ends at the terminal
    const long long frs = (long long)s * m + m;
    const double *__restrict__ Eb = A.E + b * sh.perE;
    const double *__restrict__ FRb = A.FR + b * sh.perKD;
    const double *__restrict__ Lcb = A.Lc + b * sh.perHw;
    const double *__restrict__ pb = A.lpc + b * sh.perh, *__restrict__ qb = A.lpa + b * sh.perh;
    const double *__restrict__ wb = A.ws + b * sh.perh, *__restrict__ vb = A.v + b * sh.perh;
    double *lamb = A.lam + b * (long long)(N + 1) * n, *mub = A.mu + b * (long long)(N + 1) * n;

    // the boundary costates at k = N1 (direct reads, once per segment)
    if (lane < n) {
        double al = 0.0, am = 0.0, p0, q0;
        if (last) {  // lambda_N = H~_N x_N + h~_N, mu_N = H~_N v_N + g_N: Lc holds H~_N at stage N
            const double *PN = Lcb + (long long)N * sh.ps;
            const long long xo = (long long)N * s;
            for (int j = 0; j < n; ++j) {
                const double p = PN[lane >= j ? pidx(lane, j, n) : pidx(j, lane, n)];
                al += p * wb[xo + j];
                am += p * vb[xo + j];
            }
            p0 = pb[xo + lane];
            q0 = qb[xo + lane];
        } else {  // entry seg + 1 of the scans: the value function at the start of the next segment
            const long long es = elem_doubles(n), eo = (b * S + seg + 1) * es;
            const double *Ps = A.sufp + eo + 2 * n * n + n;
            const long long xo = (long long)N1 * s + m;
            for (int j = 0; j < n; ++j) {
                const double p = Ps[lane + j * n];
                al += p * wb[xo + j];
                am += p * vb[xo + j];
            }
            p0 = A.sufp[eo + 3 * n * n + n + lane];
            q0 = A.sufa[eo + 3 * n * n + n + lane];
        }
        const double l = al + p0, u = am + q0;
        if (A.need_lam) gstore(lamb + (long long)N1 * n + lane, l);
        gstore(mub + (long long)N1 * n + lane, u);
        stl[lane] = last ? 0.0 : l;
        stm[lane] = last ? 0.0 : u;
    }

    const int klo = seg == 0 ? N0 : N0 + 1;  // segment 0 also forms the costates of stage 0 (mu_0 = grad x0)
    double R[C], xr = 0.0, vr = 0.0, pr = 0.0, qr = 0.0;
    auto load = [&](int k) {
        const double *Ek = Eb + (long long)k * nE, *Lk = FRb + (long long)k * frs, *Pk = Lcb + (long long)k * sh.ps;
#pragma unroll
        for (int r = 0; r < C; ++r) {  // (the round's block is wave-uniform)
            double x = 0.0;
            if (r < rE) {
                const int e = lane + 64 * r;
                if (e < nE) x = Ek[e];
            } else if (r < rEL) {
                const int e = lane + 64 * (r - rE);
                if (e < nL) x = Lk[e];
            } else if (r < rELP) {
                const int e = lane + 64 * (r - rEL);
                if (e < pn) x = Pk[e];
            }
            R[r] = x;
        }
        if (lane < n) {
            const long long xo = (long long)k * s + m + lane;
            xr = wb[xo];
            vr = vb[xo];
            pr = pb[xo];
            qr = qb[xo];
        }
    };
    const int rot = (n & 1) ? 0 : lane % n;  // the lane's first row of its E column
    const int ci = lane < n ? pidx(lane, lane, n) - lane : 0;  // packed P: entry (j, lane), j >= lane, is sP[ci + j]
    if (N1 - 1 >= klo) load(N1 - 1);
    for (int k = N1 - 1; k >= klo; --k) {
        wave_sync();  // the stage before is done with the LDS blocks
#pragma unroll
        for (int r = 0; r < C; ++r)
            if (r < rELP) sE[lane + 64 * r] = R[r];
        sx[lane] = xr;
        sv[lane] = vr;
        const double pk = pr, qk = qr;
        wave_sync();
        if (k - 1 >= klo) load(k - 1);  // in flight during this stage

        // r = E_k^T t_{k+1}
        double rl = 0.0, rm = 0.0;
        if (lane < s) {
            const double *Ec = sE + lane * n;
            int i = rot;
#pragma unroll 4  // (the LDS reads of four rows in flight)
            for (int q = 0; q < n; ++q) {
                const double e = Ec[i];
                rl += e * stl[i];
                rm += e * stm[i];
                i = i + 1 == n ? 0 : i + 1;
            }
        }
        // z = Luu^{-1} r_u, and r_x - Lxu z on the lanes below: L(j, i) = sL[i s + j];
        // the m pivots are inverted at once, off the chain of the substitution
        const double dinv = lane < m ? 1.0 / sL[lane * s + lane] : 0.0;
        double ln = sL[lane];  // column i + 1 is read while column i is applied (lanes >= s: unused slots of the block)
        for (int i = 0; i < m; ++i) {
            const double l = ln;
            if (i + 1 < m) ln = sL[(i + 1) * s + lane];
            const double di = readlane_f64(dinv, i);
            const double zl = readlane_f64(rl, i) * di, zm = readlane_f64(rm, i) * di;
            if (lane > i && lane < s) {
                rl -= l * zl;
                rm -= l * zm;
            }
        }
        wave_sync();
        if (lane >= m && lane < s) {
            stl[lane - m] = rl;
            stm[lane - m] = rm;
        }
        wave_sync();
        if (lane < n) {  // lambda_k = P_k x_k + p_k + t_k
            double al = 0.0, am = 0.0;
            int cj = 0;  // pidx(j, j, n) - j
#pragma unroll 4
            for (int j = 0; j < n; ++j) {
                const double p = sP[j <= lane ? cj + lane : ci + j];
                al += p * sx[j];
                am += p * sv[j];
                cj += n - j - 1;
            }
            if (A.need_lam) gstore(lamb + (long long)k * n + lane, (al + pk) + stl[lane]);
            gstore(mub + (long long)k * n + lane, (am + qk) + stm[lane]);
        }
    }
}

int launch_seg_costate(const SegCostateArgs &a, hipStream_t st) {
    const Shape &sh = a.sh;
    const long long blocks = (long long)sh.batch * a.S;
    if (sh.s > 64 || blocks > 0x7fffffffLL) {
        set_error("adjoint_parallel: n + m > 64 or batch * segments exceeds the grid limit");
        return PDPLQR_ERR_UNSUPPORTED;
    }
    const size_t lds = seg_costate_lds_doubles(sh) * sizeof(double);
    const dim3 grid((unsigned)blocks), blk(64);
    if (sh.s <= 16) {
        hipLaunchKernelGGL(k_seg_costate<16>, grid, blk, lds, st, a);
    } else if (sh.s <= 32) {
        hipLaunchKernelGGL(k_seg_costate<32>, grid, blk, lds, st, a);
    } else {  // (at most 64 (64 + 32 + 2 + 4) doubles: 52 KB)
        hipLaunchKernelGGL(k_seg_costate<64>, grid, blk, lds, st, a);
    }
    PDPLQR_HIP_TRY(hipGetLastError());
    return PDPLQR_OK;
}

// k_adjoint_grad (kernels_adjoint.hip) with the costates read from [b][N + 1][n]
// arrays instead of formed from a cached Lxx: the same stage tiles, the same
// flat runs, the same products.
template <int NN, int MM, bool VEC>
__global__ __launch_bounds__(256) void k_adjoint_grad_costate(AdjointCostateArgs A) {
#pragma clang fp contract(off)  // v_i w_j + w_i v_j rounds the same way as its transpose: grad H is exactly symmetric
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const Shape &sh = A.sh;
    const int n = NN ? NN : sh.n, m = NN ? MM : sh.m, s = n + m, N = sh.N;
    const int ts = A.ts, tiles = (N + ts - 1) / ts;
    const long long b = blockIdx.x / tiles;
    const int k0 = (int)(blockIdx.x - b * tiles) * ts;
    const int T = min(ts, N - k0);
    const bool last = k0 + T == N;
    const int tid = threadIdx.x;
    const bool need_mu = A.gE || A.gc, need_lam = A.gE != nullptr;

    double *sw = lds, *sv = sw + (ts + 1) * s;          // w, v of stages k0 .. k0 + T
    double *slam = sv + (ts + 1) * s, *smu = slam + ts * n;  // costates of stages k0 + 1 .. k0 + T

    const double *wb = A.ws + b * sh.perh, *vb = A.v + b * sh.perh;
    {
        const int cnt = T * s + (last ? n : s);
        for (int e = tid; e < cnt; e += 256) {
            sw[e] = wb[(long long)k0 * s + e];
            sv[e] = vb[(long long)k0 * s + e];
        }
    }
    if (need_mu) {
        const long long o = (b * (N + 1) + k0 + 1) * n;
        for (int e = tid; e < T * n; e += 256) {
            smu[e] = A.mu[o + e];
            if (need_lam) slam[e] = A.lam[o + e];
        }
    }
    __syncthreads();

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
    if (A.gx && k0 == 0 && tid < n) A.gx[b * n + tid] = A.mu[b * (long long)(N + 1) * n + tid];  // mu_0
}

int launch_adjoint_grad_costate(const AdjointCostateArgs &a0, hipStream_t st) {
    AdjointCostateArgs a = a0;
    const Shape &sh = a.sh;
    if (!a.gE && !a.gc && !a.gH && !a.gh && !a.gx) return PDPLQR_OK;
    a.ts = adjoint_tile(sh);
    const long long tiles = (sh.N + a.ts - 1) / a.ts, blocks = tiles * sh.batch;
    if (blocks > 0x7fffffffLL) {
        set_error("adjoint_parallel: batch * stage tiles exceeds the grid limit");
        return PDPLQR_ERR_UNSUPPORTED;
    }
    auto al = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    const bool vec = sh.n % 2 == 0 && sh.m % 2 == 0 && al(a.gE) && al(a.gc) && al(a.gH) && al(a.gh);
    const dim3 grid((unsigned)blocks), blk(256);
    const size_t lds = sizeof(double) * (2ull * (a.ts + 1) * sh.s + 2ull * a.ts * sh.n);
    if (vec && sh.n == 12 && sh.m == 4) hipLaunchKernelGGL((k_adjoint_grad_costate<12, 4, true>), grid, blk, lds, st, a);
    else if (vec) hipLaunchKernelGGL((k_adjoint_grad_costate<0, 0, true>), grid, blk, lds, st, a);
    else hipLaunchKernelGGL((k_adjoint_grad_costate<0, 0, false>), grid, blk, lds, st, a);
    PDPLQR_HIP_TRY(hipGetLastError());
    return PDPLQR_OK;
}

}  // namespace pdplqr
