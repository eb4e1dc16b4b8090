// kernels_cone.hip -- second-order cone rows of the ADMM outer loop (DESIGN.md
// section 5.5 "Second-order cones"; the iteration is admm.hip's header with
//     z^{k+1} = Pi(v_rel + inv_rho o y^k)
// over a mixed set: rows in no cone stay box rows, the rows of cone i of a
// stage, with b = e_lb on them, ask  D w - b  in  K_q = {(t, x) : |x|_2 <= t}
// (first row = t; e_ub of a cone row is not read).  With rho constant within a
// cone the projection in the rho-norm is the Euclidean one of p = (t, x):
//     |x| <= t   ->  p            (interior, boundary included)
//     |x| <= -t  ->  0            (the polar cone)
//     otherwise  ->  a = (1 + t / |x|) / 2,  (a |x|, a x)
// evaluated in that order, so |x| = 0 never reaches the division.  |x| is the
// square root of the squares summed in row order, without rescaling: the
// loop's values are O(1) (rows of D w against bounds of a scaled problem), and
// anything whose square stays inside the double range (1e-150 .. 1e150) is
// exact to rounding.
//
//   k_admm_update_cone  k_admm_update's layout (one 256-thread block per problem,
//                       LPS lanes per stage, the block strides the horizon).  One
//                       sweep over the stage's rows: a box row is k_admm_update's
//                       statements; a cone row forms p_r on every lane of the
//                       stage, lane 0 keeps (p_r, v_rel, D w^{k+1}) in the stage's
//                       LDS tile and t, sum x^2 accumulate in row order; at the
//                       cone's last row the lanes walk the cone again (no
//                       butterflies: everything is in the tile) for z, y, g, the
//                       three D^T column sums and the five maxima, in row order.
//   k_cone_project      the projection onto the mixed set alone (pdplqr_admm_project)
//   k_cone_project_vjp  its transposed Jacobian applied to a cotangent (pdplqr_admm_project_vjp)
//   k_cone_validate     rho constant within a cone, e_lb finite on cone rows
// The cone arithmetic is compiled with contraction off (a value does not depend
// on the kernel instance, and k_cone_project gives the update's bits); the box
// rows keep the contraction k_admm_update is compiled with, so that they keep
// its bits (tests/test_gpu_cone.py pins both).
#include "admm.hpp"
#include "cone_math.hpp"
#include "device_common.hpp"

namespace pdplqr {

namespace {

constexpr int kConeTile = 66;      // doubles of one tile row: cone_dim <= n + m + 1 <= 65
constexpr int kNoCone = 1 << 30;   // "the stage has no further cone"
constexpr double kInfBound = 1e20;

// admm.hip's butterflies (every lane of the stage ends with the same bits)
template <int LPS>
__device__ __forceinline__ double stage_sum(double v) {
    if constexpr (LPS == 16) {
        return sum_row16(v);
    } else {
#pragma unroll
        for (int m = 1; m < LPS; m <<= 1) v += __shfl_xor(v, m, 64);
        return v;
    }
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
    return v;
}

}  // namespace

template <int LPS, bool FUSE, bool CHECK>
__global__ void __launch_bounds__(256) k_admm_update_cone(ConeArgs ca) {
    const AdmmArgs &a = ca.a;
    const Shape &sh = a.sh;
    const int b = blockIdx.x;
    if (a.done[b]) return;  // block-uniform
    constexpr int SPW = 64 / LPS;
    constexpr int NV = CHECK ? 3 : 2;  // p, v_rel (, D w^{k+1}) of every row of the open cone
    __shared__ double tile[4 * SPW][NV][kConeTile];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, sub = lane / LPS, j = lane % LPS;
    double(*tl)[kConeTile] = tile[wv * SPW + sub];
    const double al = a.alpha, bl = 1.0 - a.alpha;
    double rp = 0.0, dwm = 0.0, zm = 0.0, rd = 0.0, dty = 0.0, act = 0.0;
    for (int kb = wv * SPW; kb <= sh.N; kb += 4 * SPW) {
        // wave-uniform trip count: lanes past the horizon idle in the loop
        const int k = kb + sub;
        const bool stg = k <= sh.N;
        const int kk = stg ? k : sh.N;
        const int dim = kk < sh.N ? sh.s : sh.n;
        const bool col = stg && j < dim;
        const long long wo = (long long)b * sh.perh + (long long)kk * sh.s + (j < dim ? j : 0);
        const int yo0 = a.uni ? kk * a.uni : a.y_off[kk];
        const int nc = !stg ? 0 : (a.uni ? (kk < sh.N ? a.uni : 0) : a.y_off[kk + 1] - yo0);
        const long long yo = (long long)b * sh.ny + yo0;
        const double *Dk = a.D + (long long)b * sh.ndD + (a.uni ? (long long)kk * a.uni * sh.s : a.d_off[kk]);
        const double wtj = col ? a.wt[wo] : 0.0, wj = col ? a.w[wo] : 0.0;
        const double wn = al * wtj + bl * wj;
        double ag = 0.0, ad = 0.0, ay = 0.0;
        // the stage's cones, in row order: [cr, cr + cd) is the next (or the open) one
        int ci = stg ? ca.c_off[kk] : 0;
        const int ce = stg ? ca.c_off[kk + 1] : 0;
        int cr = ci < ce ? ca.c_row[ci] : kNoCone, cd = ci < ce ? ca.c_dim[ci] : 0;
        double ct = 0.0, css = 0.0;  // t and sum x^2 of the open cone
        for (int r = 0; r < a.max_nc; ++r) {
            const bool row = r < nc;
            const double d = (row && col) ? Dk[r + j * nc] : 0.0;
            const double v = stage_sum<LPS>(d * wtj);
            const double vw = stage_sum<LPS>(d * wj);
            if (row && r < cr) {
                // a box row: k_admm_update's statements
                const double zr = a.z[yo + r], yr = a.y[yo + r], rr = a.rho[yo + r], ir = a.irho[yo + r];
                const double vrel = al * v + bl * zr;
                const double zn = fmin(fmax(vrel + ir * yr, a.lb[yo + r]), a.ub[yo + r]);
                const double yn = yr + rr * (vrel - zn);
                const double gn = zn - ir * yn;
                if (j == 0) {
                    a.z[yo + r] = zn;
                    a.y[yo + r] = yn;
                    if (FUSE) a.gw[yo + r] = gn;
                }
                if (FUSE) ag += d * (rr * gn);  // k_penalty's order: D[q][i] * (rho_q * g_q)
                if (CHECK) {
                    const double dwn = al * v + bl * vw;  // D w^{k+1}
                    rp = fmax(rp, fabs(dwn - zn));
                    dwm = fmax(dwm, fabs(dwn));
                    zm = fmax(zm, fabs(zn));
                    ad += d * (rr * (zn - zr));
                    ay += d * yn;
                    if (zn <= a.lb[yo + r] || zn >= a.ub[yo + r]) act = 1.0;
                }
            } else if (row) {
#pragma clang fp contract(off)
                // pass one of a cone row: p_r = v_rel + inv_rho y - b, the same bits on every lane
                const int i = r - cr;
                const double zr = a.z[yo + r], yr = a.y[yo + r], ir = a.irho[yo + r];
                const double vrel = al * v + bl * zr;
                const double p = (vrel + ir * yr) - a.lb[yo + r];
                if (j == 0) {
                    tl[0][i] = p;
                    tl[1][i] = vrel;
                    if (CHECK) tl[2][i] = al * v + bl * vw;  // D w^{k+1}
                }
                if (i == 0) {
                    ct = p;
                    css = 0.0;
                } else {
                    css = css + p * p;
                }
                if (i == cd - 1) {
                    // pass two: the cone is complete
                    const double nx = sqrt(css);
                    double head, sc;
                    const int kind = cone_case(ct, nx, head, sc);
                    if (CHECK && nx >= ct) act = 1.0;  // the result lies on the cone's boundary
                    for (int q = 0; q < cd; ++q) {
                        const long long yq = yo + cr + q;
                        const double dq = col ? Dk[cr + q + j * nc] : 0.0;
                        const double zq = a.z[yq], yy = a.y[yq], rq = a.rho[yq], iq = a.irho[yq];
                        const double vq = tl[1][q];
                        const double zn = a.lb[yq] + cone_entry(kind, head, sc, q, tl[0][q]);
                        const double yn = yy + rq * (vq - zn);
                        const double gn = zn - iq * yn;
                        if (j == 0) {
                            a.z[yq] = zn;
                            a.y[yq] = yn;
                            if (FUSE) a.gw[yq] = gn;
                        }
                        if (FUSE) ag = ag + dq * (rq * gn);
                        if (CHECK) {
                            const double dwn = tl[2 % NV][q];
                            rp = fmax(rp, fabs(dwn - zn));
                            dwm = fmax(dwm, fabs(dwn));
                            zm = fmax(zm, fabs(zn));
                            ad = ad + dq * (rq * (zn - zq));
                            ay = ay + dq * yn;
                        }
                    }
                    ++ci;
                    cr = ci < ce ? ca.c_row[ci] : kNoCone;
                    cd = ci < ce ? ca.c_dim[ci] : 0;
                }
            }
        }
        if (col) {
            a.w[wo] = wn;
            if (FUSE) {
                // k_update_problem_data then k_penalty: (h - sigma w) - sum
                double hj = a.hv[wo] - a.sigma * wn;
                if (nc > 0 && !a.no_penalty) hj -= ag;
                a.hw[wo] = hj;
            }
        }
        if (CHECK) {
            rd = fmax(rd, fabs(ad));
            dty = fmax(dty, fabs(ay));
        }
    }
    if (CHECK) {
        __shared__ double red[4][6];
        rp = wave_max(rp);
        dwm = wave_max(dwm);
        zm = wave_max(zm);
        rd = wave_max(rd);
        dty = wave_max(dty);
        act = wave_max(act);
        if (lane == 0) {
            red[wv][0] = rp;
            red[wv][1] = dwm;
            red[wv][2] = zm;
            red[wv][3] = rd;
            red[wv][4] = dty;
            red[wv][5] = act;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
#pragma unroll
            for (int q = 1; q < 4; ++q) {
                rp = fmax(rp, red[q][0]);
                dwm = fmax(dwm, red[q][1]);
                zm = fmax(zm, red[q][2]);
                rd = fmax(rd, red[q][3]);
                dty = fmax(dty, red[q][4]);
                act = fmax(act, red[q][5]);
            }
            admm_decide(a, b, rp, dwm, zm, rd, dty, act);
        }
    }
}

// One thread per (stage, problem): the stage's rows in order, a box row clamps,
// a cone takes its two passes (the update kernel's arithmetic on p = v - b).
// c_off null: no cones.
__global__ void __launch_bounds__(64) k_cone_project(Shape sh, const int32_t *__restrict__ y_off,
                                                     const int32_t *__restrict__ c_off,
                                                     const int32_t *__restrict__ c_row,
                                                     const int32_t *__restrict__ c_dim, const double *v,
                                                     const double *lb, const double *ub, double *out) {
#pragma clang fp contract(off)
    const int k = blockIdx.y * blockDim.x + threadIdx.x, b = blockIdx.x;
    if (k > sh.N) return;
    const int yo = y_off[k], nc = y_off[k + 1] - yo;
    const long long base = (long long)b * sh.ny + yo;
    int ci = c_off ? c_off[k] : 0;
    const int ce = c_off ? c_off[k + 1] : 0;
    int r = 0;
    while (r < nc) {
        if (ci < ce && r == c_row[ci]) {
            const int cd = c_dim[ci];
            const double t = v[base + r] - lb[base + r];
            double ss = 0.0;
            for (int i = 1; i < cd; ++i) {
                const double p = v[base + r + i] - lb[base + r + i];
                ss = ss + p * p;
            }
            double head, sc;
            const int kind = cone_case(t, sqrt(ss), head, sc);
            for (int i = 0; i < cd; ++i) {
                const double l = lb[base + r + i];
                out[base + r + i] = l + cone_entry(kind, head, sc, i, v[base + r + i] - l);
            }
            r += cd;
            ++ci;
        } else {
            out[base + r] = fmin(fmax(v[base + r], lb[base + r]), ub[base + r]);
            ++r;
        }
    }
}

// The transposed Jacobian of k_cone_project at v applied to gout, on the same
// walk: gv = J^T gout, glb and gub the cotangents of the bounds (any NULL).  A
// box row passes gout to gv strictly inside, to glb where v <= lb, to gub where
// v >= ub.  A cone takes the case k_cone_project takes for the same bits (the
// same |x|, the same tests); out = b + Pi(v - b), so glb = g - J g and gub = 0.
__global__ void __launch_bounds__(64) k_cone_project_vjp(Shape sh, const int32_t *__restrict__ y_off,
                                                         const int32_t *__restrict__ c_off,
                                                         const int32_t *__restrict__ c_row,
                                                         const int32_t *__restrict__ c_dim, const double *v,
                                                         const double *lb, const double *ub, const double *gout,
                                                         double *gv, double *glb, double *gub) {
#pragma clang fp contract(off)
    const int k = blockIdx.y * blockDim.x + threadIdx.x, b = blockIdx.x;
    if (k > sh.N) return;
    const int yo = y_off[k], nc = y_off[k + 1] - yo;
    const long long base = (long long)b * sh.ny + yo;
    int ci = c_off ? c_off[k] : 0;
    const int ce = c_off ? c_off[k + 1] : 0;
    int r = 0;
    while (r < nc) {
        if (ci < ce && r == c_row[ci]) {
            const int cd = c_dim[ci];
            const double t = v[base + r] - lb[base + r];
            double ss = 0.0;
            for (int i = 1; i < cd; ++i) {
                const double p = v[base + r + i] - lb[base + r + i];
                ss = ss + p * p;
            }
            const double nx = sqrt(ss);
            double head, sc;
            const int kind = cone_case(t, nx, head, sc);
            const double g0 = gout[base + r];
            double d = 0.0;
            if (kind == 2)
                for (int i = 1; i < cd; ++i) d = d + ((v[base + r + i] - lb[base + r + i]) / nx) * gout[base + r + i];
            for (int i = 0; i < cd; ++i) {
                const double g = gout[base + r + i];
                const double jg = cone_vjp_entry(kind, i, v[base + r + i] - lb[base + r + i], g, g0, d, t, nx);
                if (gv) gv[base + r + i] = jg;
                if (glb) glb[base + r + i] = g - jg;
                if (gub) gub[base + r + i] = 0.0;
            }
            r += cd;
            ++ci;
        } else {
            const double x = v[base + r], l = lb[base + r], u = ub[base + r], g = gout[base + r];
            if (gv) gv[base + r] = (l < x && x < u) ? g : 0.0;
            if (glb) glb[base + r] = x <= l ? g : 0.0;
            if (gub) gub[base + r] = x >= u ? g : 0.0;
            ++r;
        }
    }
}

// One thread per (cone, problem): flag[0] counts cones whose rho is not
// constant, flag[1] cone rows whose e_lb is not finite (|e_lb| >= 1e20 is infinite)
__global__ void k_cone_validate(int num_cones, int ny, const int32_t *__restrict__ c_y0,
                                const int32_t *__restrict__ c_dim, const double *__restrict__ lb,
                                const double *__restrict__ rho, int32_t *flag) {
    const int i = blockIdx.y * blockDim.x + threadIdx.x, b = blockIdx.x;
    if (i >= num_cones) return;
    const long long base = (long long)b * ny + c_y0[i];
    const int cd = c_dim[i];
    const double r0 = rho[base];
    bool bad_rho = false;
    int bad_lb = 0;
    for (int q = 0; q < cd; ++q) {
        if (rho[base + q] != r0) bad_rho = true;
        if (!(fabs(lb[base + q]) < kInfBound)) ++bad_lb;  // (NaN fails the comparison)
    }
    if (bad_rho) atomicAdd(flag, 1);
    if (bad_lb) atomicAdd(flag + 1, bad_lb);
}

int launch_admm_update_cone(const ConeArgs &c, int lps, bool fuse, bool check, hipStream_t st) {
    const dim3 grid((unsigned)c.a.sh.batch), blk(256);
#define PDPLQR_CONE_LAUNCH(L, F, C) hipLaunchKernelGGL((k_admm_update_cone<L, F, C>), grid, blk, 0, st, c)
#define PDPLQR_CONE_LPS(L)                                 \
    do {                                                   \
        if (fuse && check) PDPLQR_CONE_LAUNCH(L, true, true);   \
        else if (fuse) PDPLQR_CONE_LAUNCH(L, true, false);      \
        else if (check) PDPLQR_CONE_LAUNCH(L, false, true);     \
        else PDPLQR_CONE_LAUNCH(L, false, false);               \
    } while (0)
    if (lps == 16) PDPLQR_CONE_LPS(16);
    else if (lps == 32) PDPLQR_CONE_LPS(32);
    else if (lps == 64) PDPLQR_CONE_LPS(64);
    else {
        set_error("cone update: nx + nu > 64");
        return PDPLQR_ERR_UNSUPPORTED;
    }
#undef PDPLQR_CONE_LPS
#undef PDPLQR_CONE_LAUNCH
    PDPLQR_HIP_TRY(hipGetLastError());
    return PDPLQR_OK;
}

int launch_cone_project(const Shape &sh, const int32_t *y_off, const int32_t *c_off, const int32_t *c_row,
                        const int32_t *c_dim, const double *v, const double *lb, const double *ub, double *out,
                        hipStream_t st) {
    hipLaunchKernelGGL(k_cone_project, dim3((unsigned)sh.batch, (unsigned)(sh.N / 64 + 1)), dim3(64), 0, st, sh, y_off,
                       c_off, c_row, c_dim, v, lb, ub, out);
    PDPLQR_HIP_TRY(hipGetLastError());
    return PDPLQR_OK;
}

int launch_cone_project_vjp(const Shape &sh, const int32_t *y_off, const int32_t *c_off, const int32_t *c_row,
                            const int32_t *c_dim, const double *v, const double *lb, const double *ub,
                            const double *gout, double *gv, double *glb, double *gub, hipStream_t st) {
    hipLaunchKernelGGL(k_cone_project_vjp, dim3((unsigned)sh.batch, (unsigned)(sh.N / 64 + 1)), dim3(64), 0, st, sh,
                       y_off, c_off, c_row, c_dim, v, lb, ub, gout, gv, glb, gub);
    PDPLQR_HIP_TRY(hipGetLastError());
    return PDPLQR_OK;
}

int launch_cone_validate(int batch, int ny, int num_cones, const int32_t *c_y0, const int32_t *c_dim, const double *lb,
                         const double *rho, int32_t *flag, hipStream_t st) {
    hipLaunchKernelGGL(k_cone_validate, dim3((unsigned)batch, (unsigned)((num_cones + 63) / 64)), dim3(64), 0, st,
                       num_cones, ny, c_y0, c_dim, lb, rho, flag);
    PDPLQR_HIP_TRY(hipGetLastError());
    return PDPLQR_OK;
}

}  // namespace pdplqr
