// kernels_fpadj.hip -- the device side of pdplqr_admm_adjoint_fixed_point
// (adjoint.hip): the fixed-point adjoint of the ADMM
// loop at its solution, box rows and second-order cone rows alike.  New: the
// reference has no such call.
//
// The state a = (a_w, a_y, a_z) starts at zero; with tt = zs + ys / rho the
// projection's argument at the fixed point and P^T the transposed Jacobian of
// the projection there (a 0/1 mask on box rows, cone_math.hpp's symmetric
// matrix on the rows of a cone), iteration k is
//     b_w = gws + a_w;  q = a_z - rho o a_y;  b_vr = rho o a_y + P^T q
//     v   = the adjoint solve with right-hand side alpha b_w + D^T (alpha b_vr)
//     a_w <- (1 - alpha) b_w - sigma v
//     a_y <- a_y + P^T q / rho + D v          (grad g = -rho o D v)
//     a_z <- (1 - alpha) b_vr - rho o D v
//
//   k_fpadj_step   everything of one iteration that is not the solve, in one
//                  pass (k_admm_update_cone's layout: a 256-thread block per
//                  problem, LPS lanes per stage, the block strides the horizon,
//                  ragged nc_k, terminal rows of width n): D v by a butterfly
//                  per row, the three state updates of iteration k, the
//                  max-norm change and max-norm of the state when k is a test
//                  iteration, then the cotangents of iteration k + 1 -- q,
//                  P^T q (kept in `jq` for the next update) -- and the next
//                  solve's right-hand side alpha b_w + D^T (alpha b_vr), which
//                  saves k_adjoint_rhs's pass.  D of a stage is read once and
//                  serves both D v and D^T.  A cone's tt - b, q and rho o a_y
//                  go through the stage's LDS tile, written by lane 0 and read
//                  by broadcast at the cone's last row (no butterflies in the
//                  walk: every lane of the stage holds the same bits).  With
//                  v null nothing is updated and only the cotangents are
//                  formed: the start (a = 0) and the final pass, which also
//                  writes alpha b_vr, grad lb and grad ub.  A frozen problem
//                  returns at the top.  One atomic: the count of active
//                  problems of a test iteration.
// Contraction is off: a value does not depend on the kernel instance, and the
// box rows repeat BoxLQRLayer.backward's torch statements in their order.
#include "adjoint.hpp"
#include "cone_math.hpp"
#include "device_common.hpp"

namespace pdplqr {

namespace {

constexpr int kFpTile = 66;      // doubles of one tile row: cone_dim <= n + m + 1 <= 65
constexpr int kFpNoCone = 1 << 30;

__device__ __forceinline__ double fp_wave_max(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
    return v;
}

template <int LPS>
__device__ __forceinline__ double fp_stage_sum(double v) {
#pragma unroll
    for (int m = 1; m < LPS; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

}  // namespace

template <int LPS>
__global__ void __launch_bounds__(256) k_fpadj_step(FpadjArgs a) {
#pragma clang fp contract(off)
    const Shape &sh = a.sh;
    const int b = blockIdx.x;
    const bool upd = a.v != nullptr;  // kernel-uniform
    if (upd && a.done[b]) return;     // block-uniform
    constexpr int SPW = 64 / LPS;
    __shared__ double tile[4 * SPW][3][kFpTile];  // tt - b, q, rho o a_y of every row of the open cone
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, sub = lane / LPS, j = lane % LPS;
    double(*tl)[kFpTile] = tile[wv * SPW + sub];
    const int N = sh.N, s = sh.s;
    const double al = a.alpha, bl = 1.0 - a.alpha;
    double ch = 0.0, nrm = 0.0;
    for (int kb = wv * SPW; kb <= N; kb += 4 * SPW) {
        // wave-uniform trip count: lanes past the horizon idle in the loop
        const int k = kb + sub;
        const bool stg = k <= N;
        const int kk = stg ? k : N;
        const int dim = kk < N ? s : sh.n;
        const bool col = stg && j < dim;
        const long long wo = (long long)b * sh.perh + (long long)kk * s + (j < dim ? j : 0);
        const int yo0 = a.y_off[kk];
        const int nc = stg ? a.y_off[kk + 1] - yo0 : 0;
        const long long yo = (long long)b * sh.ny + yo0;
        const double *Dk = a.D + (long long)b * sh.ndD + a.d_off[kk];
        const double awj = col ? a.aw[wo] : 0.0, gj = col ? a.gws[wo] : 0.0;
        const double vj = (upd && col) ? a.v[wo] : 0.0;
        double awn = awj;
        if (upd) awn = bl * (gj + awj) - a.sigma * vj;
        if (a.test && col) {
            ch = fmax(ch, fabs(awn - awj));
            nrm = fmax(nrm, fabs(awn));
        }
        // the stage's cones, in row order: [cr, cr + cd) is the next (or the open) one
        int ci = (stg && a.c_off) ? a.c_off[kk] : 0;
        const int ce = (stg && a.c_off) ? a.c_off[kk + 1] : 0;
        int cr = ci < ce ? a.c_row[ci] : kFpNoCone, cd = ci < ce ? a.c_dim[ci] : 0;
        double ct = 0.0, css = 0.0;  // t and sum x^2 of the open cone
        double acc = 0.0;            // D^T (alpha b_vr), in row order
        for (int r = 0; r < a.max_nc; ++r) {  // uniform
            const bool row = r < nc;
            const double d = (row && col) ? Dk[r + j * nc] : 0.0;
            const double dv = upd ? fp_stage_sum<LPS>(d * vj) : 0.0;
            if (!row) continue;
            const long long yq = yo + r;
            // (every lane of the stage reads the row's state before lane 0 stores it)
            const double rr = a.rho[yq], ay = a.ay[yq], az = a.az[yq];
            double ayn = ay, azn = az;
            if (upd) {
                const double jo = a.jq[yq];  // P^T q of this iteration
                const double bvr = rr * ay + jo;
                const double gg = -(rr * dv);
                ayn = (ay + jo / rr) - gg / rr;
                azn = bl * bvr + gg;
            }
            if (a.test) {
                ch = fmax(ch, fmax(fabs(ayn - ay), fabs(azn - az)));
                nrm = fmax(nrm, fmax(fabs(ayn), fabs(azn)));
            }
            const double ray = rr * ayn, qn = azn - ray;
            const double l = a.lb[yq], tt = a.zs[yq] + a.ys[yq] / rr;
            if (r < cr) {
                // a box row: the mask of BoxLQRLayer.backward
                const double u = a.ub[yq];
                const double jn = (l < tt && tt < u) ? qn : 0.0;
                const double bv = al * (ray + jn);
                acc = acc + d * bv;
                if (j == 0) {
                    if (upd) {
                        a.ay[yq] = ayn;
                        a.az[yq] = azn;
                    }
                    a.jq[yq] = jn;
                    if (a.gvs) a.gvs[yq] = bv;
                    if (a.glb) a.glb[yq] = tt <= l ? qn : 0.0;
                    if (a.gub) a.gub[yq] = tt >= u ? qn : 0.0;
                }
            } else {
                // pass one of a cone row: the same bits on every lane of the stage
                const int i = r - cr;
                const double p = tt - l;
                if (j == 0) {
                    tl[0][i] = p;
                    tl[1][i] = qn;
                    tl[2][i] = ray;
                    if (upd) {
                        a.ay[yq] = ayn;
                        a.az[yq] = azn;
                    }
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
                    const double g0 = tl[1][0];
                    double dd = 0.0;  // xh . q_x, in row order
                    if (kind == 2)
                        for (int q = 1; q < cd; ++q) dd = dd + (tl[0][q] / nx) * tl[1][q];
                    for (int q = 0; q < cd; ++q) {
                        const long long yc = yo + cr + q;
                        const double gq = tl[1][q];
                        const double jn = cone_vjp_entry(kind, q, tl[0][q], gq, g0, dd, ct, nx);
                        const double bv = al * (tl[2][q] + jn);
                        const double dq = col ? Dk[cr + q + j * nc] : 0.0;
                        acc = acc + dq * bv;
                        if (j == 0) {
                            a.jq[yc] = jn;
                            if (a.gvs) a.gvs[yc] = bv;
                            if (a.glb) a.glb[yc] = gq - jn;
                            if (a.gub) a.gub[yc] = 0.0;
                        }
                    }
                    ++ci;
                    cr = ci < ce ? a.c_row[ci] : kFpNoCone;
                    cd = ci < ce ? a.c_dim[ci] : 0;
                }
            }
        }
        if (col) {
            if (upd) a.aw[wo] = awn;
            a.rhs[wo] = al * (gj + awn) + acc;  // k_adjoint_rhs's statement
        }
    }
    if (a.test) {
        __shared__ double red[4][2];
        ch = fp_wave_max(ch);
        nrm = fp_wave_max(nrm);
        if (lane == 0) {
            red[wv][0] = ch;
            red[wv][1] = nrm;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
#pragma unroll
            for (int q = 1; q < 4; ++q) {
                ch = fmax(ch, red[q][0]);
                nrm = fmax(nrm, red[q][1]);
            }
            a.iters[b] = a.it;
            a.resid[2 * (long long)b] = ch;
            a.resid[2 * (long long)b + 1] = nrm;
            if (ch <= a.tol * nrm) {
                a.done[b] = 1;
                a.conv[b] = 1;
            } else {
                atomicAdd(a.active, 1);
            }
        }
    }
}

int launch_fpadj_step(const FpadjArgs &a, hipStream_t st) {
    const Shape &sh = a.sh;
    if (sh.s > 64) return PDPLQR_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)sh.batch), blk(256);
    if (sh.s <= 16) hipLaunchKernelGGL((k_fpadj_step<16>), grid, blk, 0, st, a);
    else if (sh.s <= 32) hipLaunchKernelGGL((k_fpadj_step<32>), grid, blk, 0, st, a);
    else hipLaunchKernelGGL((k_fpadj_step<64>), grid, blk, 0, st, a);
    PDPLQR_HIP_TRY(hipGetLastError());
    return PDPLQR_OK;
}

}  // namespace pdplqr
