// cone_math.hpp -- the second-order cone projection's case split and its
// Jacobian, shared by kernels_cone.hip (the projection, its vector-Jacobian
// product) and kernels_fpadj.hip (the fixed-point adjoint).  Everything here is
// compiled with contraction off: a value does not depend on the kernel instance.
#pragma once
#include <hip/hip_runtime.h>

namespace pdplqr {

// which case p = (t, x) with |x| = nx falls in: 0 keep, 1 zero, 2 the boundary
// point (head = a |x|, the tail scales by a)
__device__ __forceinline__ int cone_case(double t, double nx, double &head, double &sc) {
#pragma clang fp contract(off)
    head = sc = 0.0;
    if (nx <= t) return 0;
    if (nx <= -t) return 1;
    sc = (1.0 + t / nx) / 2.0;
    head = sc * nx;
    return 2;
}

// entry i of the projection of the cone's p
__device__ __forceinline__ double cone_entry(int kind, double head, double sc, int i, double p) {
#pragma clang fp contract(off)
    return kind == 0 ? p : (kind == 1 ? 0.0 : (i == 0 ? head : sc * p));
}

// Entry i of J g, J the Jacobian of the projection at p = (t, x) (symmetric: also
// J^T g).  Case 0: J = I, case 1: J = 0; on the boundary piece, with xh = x / |x|,
// tr = t / |x| and d = xh . g_x,
//     (J g)_t = (g_t + d) / 2,   (J g)_x = (g_t xh + (1 + tr) g_x - tr d xh) / 2.
// pi, gi: entry i of p and g; g0 = g_t; nx = |x| (not read unless kind == 2).
__device__ __forceinline__ double cone_vjp_entry(int kind, int i, double pi, double gi, double g0, double d, double t,
                                                 double nx) {
#pragma clang fp contract(off)
    if (kind == 0) return gi;
    if (kind == 1) return 0.0;
    if (i == 0) return (g0 + d) / 2.0;
    const double xh = pi / nx, tr = t / nx;
    return ((g0 * xh + (1.0 + tr) * gi) - (tr * d) * xh) / 2.0;
}

}  // namespace pdplqr
