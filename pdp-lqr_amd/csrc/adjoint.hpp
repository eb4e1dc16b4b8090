// adjoint.hpp -- the adjoint solve's gradient pass (kernels_adjoint.hip) and
// its per-handle scratch (adjoint.hip).
#pragma once
#include "internal.hpp"

namespace pdplqr {

struct AdjointArgs {
    Shape sh;
    const double *ws, *v;     // primal and adjoint solutions [b][N*s + n]
    const double *Lc;         // factor cache [b][N*ps + pn]
    const double *lpc, *lpa;  // lp_k = [lu'; p_k] of the primal and of the adjoint solve
    double *gE, *gc, *gH, *gh, *gx;  // outputs in the boundary layouts; NULL = not wanted
    int ts = 0;               // stages per block (set by the launcher)
};

// writes the requested gradients (device pointers)
int launch_adjoint_grad(const AdjointArgs &a, hipStream_t st);
// lu'_k of the rollout record KD to buf [b][N][m], or back
int launch_adjoint_lu(const Shape &sh, double *KD, double *buf, bool restore, hipStream_t st);
size_t adjoint_lds_bytes(const Shape &sh, int ts);
int adjoint_tile(const Shape &sh);

}  // namespace pdplqr
