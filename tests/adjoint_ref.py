"""Reference gradients of the LQ solve for the adjoint tests (CPU, torch float64).

``dense_kkt_solution`` assembles the full KKT matrix of ONE problem

    min  sum_k 1/2 w_k^T sym(H_k) w_k + h_k^T w_k
    s.t. x_0 = x0,  x_{k+1} = E_k w_k + c_k          (w_k = [u_k; x_k], w_N = x_N)

from the boundary-layout arrays (include/pdplqr.h: column-major blocks,
stage-major) and solves it with ``torch.linalg.solve``, so the solution is
differentiable by autograd with respect to every input.  Nothing here comes
from the product or the oracle: the reference gradients are
``torch.autograd.grad(sum(g * w), inputs)`` and nothing else.
"""
from __future__ import annotations

import functools

import numpy as np
import torch


def _dims(c, h, x0):
    n = x0.numel()
    N = c.numel() // n
    s = (h.numel() - n) // N
    return n, s - n, N


def dense_kkt_solution(E, c, H, h, x0):
    """ws (flat, [u_k; x_k] per stage, then x_N) of one problem; 1-D float64
    torch tensors in the boundary layout."""
    n, m, N = _dims(c, h, x0)
    s = n + m
    nw = N * s + n
    dim = nw + (N + 1) * n
    K = torch.zeros(dim, dim, dtype=torch.float64)
    r = torch.zeros(dim, dtype=torch.float64)
    for k in range(N + 1):
        d = s if k < N else n
        o = k * s
        Hk = H[k * s * s:k * s * s + d * d].view(d, d).t()  # column-major block
        K[o:o + d, o:o + d] = 0.5 * (Hk + Hk.t())
    r[:nw] = -h
    # x_0 = x0
    eye = torch.eye(n, dtype=torch.float64)
    K[nw:nw + n, m:s] = eye
    K[m:s, nw:nw + n] = eye
    r[nw:nw + n] = x0
    for k in range(N):
        Ek = E[k * n * s:(k + 1) * n * s].view(s, n).t()  # n x s
        row = nw + (k + 1) * n
        xo = (k + 1) * s + (m if k + 1 < N else 0)  # x_{k+1}
        K[row:row + n, xo:xo + n] = eye
        K[xo:xo + n, row:row + n] = eye
        K[row:row + n, k * s:(k + 1) * s] = -Ek
        K[k * s:(k + 1) * s, row:row + n] = -Ek.t()
        r[row:row + n] = c[k * n:(k + 1) * n]
    return torch.linalg.solve(K, r)[:nw]


def random_problem(n, m, N, batch, seed):
    """(E, c, H, h, x0, g), numpy, batch-major boundary layout.  E = [B, I + 0.3 randn],
    H = M M^T / s + 0.5 I (symmetric positive definite), unit-normal c, h, x0, g."""
    rng = np.random.default_rng(seed)
    s = n + m
    E = np.zeros((batch, N, s, n))  # [..., j, i] = E_k[i, j]: column-major blocks
    c = rng.standard_normal((batch, N * n))
    H = np.zeros((batch, N * s * s + n * n))
    for b in range(batch):
        for k in range(N + 1):
            d = s if k < N else n
            M = rng.standard_normal((d, d))
            Hk = M @ M.T / s + 0.5 * np.eye(d)
            H[b, k * s * s:k * s * s + d * d] = Hk.reshape(-1, order="F")
            if k < N:
                B = rng.standard_normal((n, m))
                A = np.eye(n) + 0.3 * rng.standard_normal((n, n))
                E[b, k] = np.concatenate([B, A], axis=1).T
    h = rng.standard_normal((batch, N * s + n))
    x0 = rng.standard_normal((batch, n))
    g = rng.standard_normal((batch, N * s + n))
    return E.reshape(batch, -1), c, H, h, x0, g


def reference_gradients(E, c, H, h, x0, g):
    """Batch arrays (numpy): ws and d(sum g . ws)/d(E, c, H, h, x0) by autograd
    through the dense KKT solve, problem by problem."""
    batch = E.shape[0]
    out = {k: [] for k in ("ws", "gE", "gc", "gH", "gh", "gx")}
    for b in range(batch):
        ins = [torch.tensor(a[b], dtype=torch.float64, requires_grad=True) for a in (E, c, H, h, x0)]
        w = dense_kkt_solution(*ins)
        grads = torch.autograd.grad((torch.tensor(g[b], dtype=torch.float64) * w).sum(), ins)
        out["ws"].append(w.detach().numpy())
        for key, gr in zip(("gE", "gc", "gH", "gh", "gx"), grads):
            out[key].append(gr.numpy())
    return {k: np.stack(v) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def case(n, m, N, batch, seed=0, sigma=0.0):
    """One random batch and its reference gradients, computed once per session
    (callers must not modify the arrays).  sigma > 0: a proximal centre wbar is
    drawn too and the reference runs on H + sigma I, h - sigma wbar."""
    E, c, H, h, x0, g = random_problem(n, m, N, batch, seed)
    s = n + m
    wbar = np.zeros_like(h)
    Hs, hs = H, h
    if sigma != 0.0:
        wbar = np.random.default_rng(seed + 1000).standard_normal(h.shape)
        Hs = H.copy()
        for k in range(N + 1):
            d = s if k < N else n
            Hs[:, k * s * s:k * s * s + d * d:d + 1] += sigma
        hs = h - sigma * wbar
    ref = reference_gradients(E, c, Hs, hs, x0, g)
    return dict(E=E, c=c, H=H, h=h, x0=x0, g=g, wbar=wbar, **ref)


def rel(a, b):
    """Frobenius relative error of a against b over the whole array."""
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300))
