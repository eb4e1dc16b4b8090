// kernels_infeas.hip -- infeasibility certificates of the ADMM outer loop
// (OSQP: Stellato et al. 2020 section 3.4, Banjac et al.
// 2019), in the coordinates of the dynamics' affine set: the x-update solves
// the dynamics exactly, so only the rows lb <= D w <= ub are split.
//
//   k_infeas_primal   dy = y^{k+1} - y^k certifies an empty feasible set.  One
//                     wave per problem runs the costate recursion backwards,
//                     nu_N = q_N, [g_k ; nu_k] = q_k + E_k^T nu_{k+1}, q_k =
//                     D_k^T dy_k: g is the reduced gradient Z^T D^T dy over the
//                     inputs, beta = sum nu_{k+1}^T c_k + nu_0^T x0 the value
//                     (D w_p)^T dy of the zero-input rollout w_p (no rollout).
//   k_infeas_dual     dw = w^{k+1} - w^k certifies a cost unbounded below; every
//                     term is stage-local, so it is laid out like k_admm_update
//                     (a block per problem, LPS lanes per stage).
//   k_infeas_snapshot keeps (y^k, w^k) of the problems still iterating;
//   k_infeas_delta    writes the certificate of a certified problem.
// The two tests are separate launches: the recursion is N dependent steps of
// one wave, the dual test a stage-parallel sweep of a 256-thread block -- one
// grid cannot serve both shapes, and either half may be switched off.
// Contraction is off: a measure does not depend on which half was asked for
// or on the kernel instance.  A bound with |value| >= 1e20 is infinite.
#include "admm.hpp"
#include "device_common.hpp"

namespace pdplqr {

namespace {

constexpr double kInfBound = 1e20;

__device__ __forceinline__ double iw_max(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
    return v;
}

__device__ __forceinline__ double iw_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

template <int LPS>
__device__ __forceinline__ double ist_sum(double v) {
#pragma unroll
    for (int m = 1; m < LPS; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// the difference of consecutive iterates (loop) or the given vector (evaluator)
__device__ __forceinline__ double delta(const double *cur, const double *prev, long long i) {
    return prev ? cur[i] - prev[i] : cur[i];
}

// a certified problem leaves the iteration: frozen like a converged one, its
// rho kept by a batch rescale, one fewer active problem
__device__ __forceinline__ void infeas_freeze(const InfeasArgs &a, int b, int status) {
    a.done[b] = 1;
    a.status[b] = status;
    a.rscale[b] = 1.0;
    atomicSub(a.active, 1);
}

}  // namespace

// One wave per problem; lane j owns entry j of [g_k ; nu_k] (s <= 64), NB >= n.
// Two flat passes over the problem's rows give |dy|, then the support sum and
// the infinite-bound flag (they need no recursion).  In the recursion the
// loads of a stage -- the lane's column of E (contiguous, n doubles), c, and
// the first four rows of D and dy -- go into one of DEPTH + 1 register sets,
// DEPTH stages before the stage is processed; the stage loop is unrolled
// DEPTH + 1 times so that every set has a fixed name and nothing is copied (a
// copy would wait for the loads it moves).  Rows past the fourth are loaded in
// their stage.  DEPTH = 2 for n <= 16, 1 for n <= 32; past that one column
// is 64 doubles and DEPTH = 0 loads each stage at its top.  nu_{k+1} is
// broadcast through a 2 x 64 LDS buffer (one barrier per stage).
template <int NB, int DEPTH>
__global__ __launch_bounds__(64) void k_infeas_primal(InfeasArgs a) {
#pragma clang fp contract(off)
    __shared__ double snu[2][64];
    const Shape &sh = a.sh;
    const int b = blockIdx.x, j = threadIdx.x;
    if (a.done && a.done[b]) return;  // wave-uniform
    const int n = sh.n, m = sh.m, s = sh.s, N = sh.N, ny = sh.ny;
    const double *yb = a.y + (long long)b * ny, *ypb = a.yp ? a.yp + (long long)b * ny : nullptr;
    const double *lbb = a.lb + (long long)b * ny, *ubb = a.ub + (long long)b * ny;
    const double *Eb = a.E + (long long)b * sh.perE, *cb = a.c + (long long)b * sh.perc;
    const double *Db = a.D + (long long)b * sh.ndD;
    snu[0][j] = 0.0;
    snu[1][j] = 0.0;

    double nrm = 0.0;
    for (int i = j; i < ny; i += 64) nrm = fmax(nrm, fabs(delta(yb, ypb, i)));
    nrm = iw_max(nrm);
    const double thr = a.eps_p * nrm;
    double sup = 0.0, flag = 0.0;
    for (int i = j; i < ny; i += 64) {
        const double d = delta(yb, ypb, i), u = ubb[i], l = lbb[i];
        const bool uinf = u >= kInfBound, linf = l <= -kInfBound;
        if ((d > thr && uinf) || (d < -thr && linf)) flag = 1.0;
        sup += (uinf ? 0.0 : u) * fmax(d, 0.0) + (linf ? 0.0 : l) * fmin(d, 0.0);
    }
    sup = iw_sum(sup);
    flag = iw_max(flag);

    const bool xl = j >= m && j < s;  // the lane holds nu[j - m]
    const int xi = xl ? j - m : 0;
    // terminal: nu_N = q_N = D_N^T dy_N (D_N is nc_N x n)
    double v = 0.0;
    {
        const int yo = a.uni ? N * a.uni : a.y_off[N];
        const int nc = a.uni ? 0 : a.y_off[N + 1] - yo;
        const double *Dk = Db + (a.uni ? (long long)N * a.uni * s : a.d_off[N]);
        if (xl)
            for (int r = 0; r < nc; ++r) v += Dk[r + xi * nc] * delta(yb, ypb, yo + r);
    }

    // registers of one stage: the lane's column of E; its c entry, rows 0..3
    struct Stage {
        double c, d[4], y[4];
        int nc, yo;
        const double *Dk;
    };
    const bool col = j < s;
    auto load_E = [&](int k, double *Ec) {
        const double *Ek = Eb + (long long)k * n * s + (col ? j * n : 0);
#pragma unroll
        for (int i = 0; i < NB; ++i) Ec[i] = (col && i < n) ? Ek[i] : 0.0;
    };
    auto load = [&](int k, Stage &st) {
        st.c = xl ? cb[(long long)k * n + xi] : 0.0;
        st.yo = a.uni ? k * a.uni : a.y_off[k];
        st.nc = a.uni ? a.uni : a.y_off[k + 1] - st.yo;
        st.Dk = Db + (a.uni ? (long long)k * a.uni * s : a.d_off[k]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool row = r < st.nc;
            st.d[r] = (row && col) ? st.Dk[r + j * st.nc] : 0.0;
            st.y[r] = row ? delta(yb, ypb, st.yo + r) : 0.0;
        }
    };

    double gm = 0.0, bacc = 0.0;
    constexpr int SETS = DEPTH + 1;
    Stage st[SETS];
    double Ec[SETS][NB];
#pragma unroll
    for (int d = 0; d < DEPTH; ++d)
        if (N - 1 - d >= 0) {
            load(N - 1 - d, st[d]);
            load_E(N - 1 - d, Ec[d]);
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
                load_E(k - DEPTH, Ec[f]);
            }
            const Stage &cur = st[u];
            if (xl) {
                snu[buf][xi] = v;
                bacc += v * cur.c;  // nu_{k+1}^T c_k
            }
            __syncthreads();
            double acc = 0.0;
#pragma unroll
            for (int i = 0; i < NB; ++i) acc += Ec[u][i] * snu[buf][i];  // entries past n are 0 * 0
            double q = 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) q += cur.d[r] * cur.y[r];
            if (j < s)
                for (int r = 4; r < cur.nc; ++r) q += cur.Dk[r + j * cur.nc] * delta(yb, ypb, cur.yo + r);
            v = j < s ? q + acc : 0.0;
            if (j < m) gm = fmax(gm, fabs(v));
            buf ^= 1;
        }
    }
    if (xl) bacc += v * a.x0[(long long)b * n + xi];  // nu_0^T x0
    const double beta = iw_sum(bacc);
    gm = iw_max(gm);
    if (j == 0) {
        const double support = sup - beta;
        const bool cert = a.eps_p > 0.0 && nrm > 0.0 && gm <= thr && flag == 0.0 && support < -thr;
        double *ms = a.meas + (long long)b * 8;
        ms[0] = nrm;
        ms[1] = gm;
        ms[2] = support;
        ms[3] = flag;
        if (a.verdict) a.verdict[b] = cert ? 1 : 0;
        if (a.done && cert) infeas_freeze(a, b, PDPLQR_ADMM_PRIMAL_INFEASIBLE);
    }
}

// One 256-thread block per problem, LPS lanes per stage (k_admm_update's
// layout).  Lane j of stage k holds dw_k[j]; row j of H_k dw_k and row j of
// E_k dw_k are sums over i of column i (coalesced over j) times dw_k[i],
// broadcast by a shuffle; a row of D_k dw_k is a butterfly over the stage's
// lanes.  The maxima and h^T dw reduce over the block (fixed order: lane
// butterflies, then waves 0..3) and thread 0 decides.
template <int LPS>
__global__ __launch_bounds__(256) void k_infeas_dual(InfeasArgs a) {
#pragma clang fp contract(off)
    const Shape &sh = a.sh;
    const int b = blockIdx.x;
    if (a.done && a.done[b]) return;  // block-uniform (also: certified primal infeasible in this pass)
    constexpr int SPW = 64 / LPS;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, sub = lane / LPS, j = lane % LPS;
    const int n = sh.n, m = sh.m, s = sh.s, N = sh.N;
    const double *wb = a.w + (long long)b * sh.perh, *wpb = a.wp ? a.wp + (long long)b * sh.perh : nullptr;
    const double *hb = a.hv + (long long)b * sh.perh;
    double nrm = 0.0, hm = 0.0, ht = 0.0, vi = 0.0;
    for (int kb = wv * SPW; kb <= N; kb += 4 * SPW) {
        // wave-uniform trip count: lanes past the horizon idle in the loop
        const int k = kb + sub;
        const bool stg = k <= N;
        const int kk = stg ? k : N;
        const int dim = kk < N ? s : n;
        const bool col = stg && j < dim;
        const long long wo = (long long)kk * s + (j < dim ? j : 0);
        const double dwj = col ? delta(wb, wpb, wo) : 0.0;
        nrm = fmax(nrm, fabs(dwj));
        if (col) ht += hb[wo] * dwj;
        const double *Hk = a.H + (long long)b * sh.perH + (long long)kk * s * s;
        const bool dyn = stg && kk < N && j < n;
        const double *Ek = a.E + (long long)b * sh.perE + (long long)(dyn ? kk : 0) * n * s;
        double hacc = 0.0, eacc = 0.0;
        for (int i = 0; i < s; ++i) {  // uniform; s <= LPS
            const double di = __shfl(dwj, sub * LPS + i, 64);
            if (col && i < dim) hacc += Hk[j + i * dim] * di;
            if (dyn) eacc += Ek[j + i * n] * di;
        }
        hm = fmax(hm, fabs(hacc));
        if (dyn) {
            const long long xo = kk + 1 < N ? (long long)(kk + 1) * s + m + j : (long long)N * s + j;
            vi = fmax(vi, fabs(delta(wb, wpb, xo) - eacc));  // dx_{k+1} - E_k dw_k
        }
        if (stg && kk == 0 && j >= m && j < s) vi = fmax(vi, fabs(dwj));  // dx_0
        const int yo0 = a.uni ? kk * a.uni : a.y_off[kk];
        const int nc = !stg ? 0 : (a.uni ? (kk < N ? a.uni : 0) : a.y_off[kk + 1] - yo0);
        const long long yo = (long long)b * sh.ny + yo0;
        const double *Dk = a.D + (long long)b * sh.ndD + (a.uni ? (long long)kk * a.uni * s : a.d_off[kk]);
        for (int r = 0; r < a.max_nc; ++r) {  // uniform
            const bool row = r < nc;
            const double d = (row && col) ? Dk[r + j * nc] : 0.0;
            const double rv = ist_sum<LPS>(d * dwj);
            if (row) {
                if (a.ub[yo + r] < kInfBound) vi = fmax(vi, rv);
                if (a.lb[yo + r] > -kInfBound) vi = fmax(vi, -rv);
            }
        }
    }
    __shared__ double red[4][4];
    nrm = iw_max(nrm);
    hm = iw_max(hm);
    vi = iw_max(vi);
    ht = iw_sum(ht);
    if (lane == 0) {
        red[wv][0] = nrm;
        red[wv][1] = hm;
        red[wv][2] = ht;
        red[wv][3] = vi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 1; q < 4; ++q) {
            nrm = fmax(nrm, red[q][0]);
            hm = fmax(hm, red[q][1]);
            ht += red[q][2];
            vi = fmax(vi, red[q][3]);
        }
        const double thr = a.eps_d * nrm;
        const bool cert = a.eps_d > 0.0 && nrm > 0.0 && hm <= thr && ht < -thr && vi <= thr;
        double *ms = a.meas + (long long)b * 8 + 4;
        ms[0] = nrm;
        ms[1] = hm;
        ms[2] = ht;
        ms[3] = vi;
        if (a.verdict && cert) a.verdict[b] |= 2;  // (after k_infeas_primal on the stream)
        if (a.done && cert) infeas_freeze(a, b, PDPLQR_ADMM_DUAL_INFEASIBLE);
    }
}

// (y, w) -> (yp, wp) for the problems still iterating: a frozen problem keeps
// the pair its certificate was decided on
__global__ void k_infeas_snapshot(long long ny_total, int ny, long long w_total, long long perh,
                                  const int32_t *__restrict__ done, const double *__restrict__ y,
                                  const double *__restrict__ w, double *__restrict__ yp, double *__restrict__ wp) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < ny_total) {
        if (!done[t / ny]) yp[t] = y[t];
    } else if (t - ny_total < w_total) {
        const long long q = t - ny_total;
        if (!done[q / perh]) wp[q] = w[q];
    }
}

// out = cur - prev for the problems with status 2 or 3, zeros for the rest
__global__ void k_infeas_delta(long long total, long long per, const int32_t *__restrict__ status,
                               const double *__restrict__ cur, const double *__restrict__ prev,
                               double *__restrict__ out) {
#pragma clang fp contract(off)
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int st = status[t / per];
    out[t] = (st == PDPLQR_ADMM_PRIMAL_INFEASIBLE || st == PDPLQR_ADMM_DUAL_INFEASIBLE) ? cur[t] - prev[t] : 0.0;
}

bool infeas_shape_supported(const Shape &sh) { return sh.s <= 64; }

int launch_infeas_primal(const InfeasArgs &a, hipStream_t st) {
    const Shape &sh = a.sh;
    if (!infeas_shape_supported(sh)) return PDPLQR_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)sh.batch), blk(64);
    if (sh.n <= 16) hipLaunchKernelGGL((k_infeas_primal<16, 2>), grid, blk, 0, st, a);
    else if (sh.n <= 32) hipLaunchKernelGGL((k_infeas_primal<32, 1>), grid, blk, 0, st, a);
    else hipLaunchKernelGGL((k_infeas_primal<64, 0>), grid, blk, 0, st, a);
    PDPLQR_HIP_TRY(hipGetLastError());
    return PDPLQR_OK;
}

int launch_infeas_dual(const InfeasArgs &a, hipStream_t st) {
    const Shape &sh = a.sh;
    if (!infeas_shape_supported(sh)) return PDPLQR_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)sh.batch), blk(256);
    if (sh.s <= 16) hipLaunchKernelGGL((k_infeas_dual<16>), grid, blk, 0, st, a);
    else if (sh.s <= 32) hipLaunchKernelGGL((k_infeas_dual<32>), grid, blk, 0, st, a);
    else hipLaunchKernelGGL((k_infeas_dual<64>), grid, blk, 0, st, a);
    PDPLQR_HIP_TRY(hipGetLastError());
    return PDPLQR_OK;
}

int launch_infeas_snapshot(const Shape &sh, const int32_t *done, const double *y, const double *w, double *yp,
                           double *wp, hipStream_t st) {
    const long long Y = (long long)sh.batch * sh.ny, W = (long long)sh.batch * sh.perh;
    hipLaunchKernelGGL(k_infeas_snapshot, dim3((unsigned)((Y + W + 255) / 256)), dim3(256), 0, st, Y,
                       sh.ny > 0 ? sh.ny : 1, W, sh.perh, done, y, w, yp, wp);
    PDPLQR_HIP_TRY(hipGetLastError());
    return PDPLQR_OK;
}

int launch_infeas_delta(long long total, long long per, const int32_t *status, const double *cur, const double *prev,
                        double *out, hipStream_t st) {
    if (total <= 0) return PDPLQR_OK;
    hipLaunchKernelGGL(k_infeas_delta, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, total, per, status,
                       cur, prev, out);
    PDPLQR_HIP_TRY(hipGetLastError());
    return PDPLQR_OK;
}

}  // namespace pdplqr
