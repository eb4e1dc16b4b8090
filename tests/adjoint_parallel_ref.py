"""Numpy restatement of the per-stage costates of a segmented solve, in the
form k_seg_costate (csrc/kernels_adjoint_parallel.hip) uses, for the CPU tests
of pdplqr_adjoint_parallel.

A device segment [N0, N1) keeps the value function of its own sub-problem
under a free end (P = 0, p = 0 at N1; the last segment: the real terminal).
With y the costate at the segment's end,

    lambda_k = P_k x_k + p_k + t_k,    t_k = Acl_k^T t_{k+1},    t_{N1} = y,

and t is carried through the stage factor as the kernel does it:
r = E_k^T t_{k+1}, z = Luu^{-1} r_u, t_k = r_x - Lxu z.  The boundary costates
come from the global value functions, y = P_{N1} x_{N1} + p_{N1}.

``open_loop_costates`` is the recursion the kernel does NOT use,
lambda_k = [H_k w_k + h_k]_x + A_k^T lambda_{k+1}: exact in exact arithmetic,
but its rounding grows with norm(A^T)^L along a segment.
"""
from __future__ import annotations

import numpy as np


def blocks(n, m, N, E, c, H, h):
    s = n + m
    Ek = [E[k * n * s:(k + 1) * n * s].reshape(n, s, order="F") for k in range(N)]
    ck = [c[k * n:(k + 1) * n] for k in range(N)]
    Hk = [H[k * s * s:(k + 1) * s * s].reshape(s, s, order="F") for k in range(N)]
    Hk.append(H[N * s * s:].reshape(n, n, order="F"))
    hk = [h[k * s:(k + 1) * s] for k in range(N)] + [h[N * s:]]
    return Ek, ck, Hk, hk


def xof(w, k, n, m, N):
    s = n + m
    return w[k * s + m:(k + 1) * s] if k < N else w[N * s:]


def _stage(m, Ek, ck, Hk, hk, P1, p1):
    """One factored stage under (P1, p1) at k + 1: (P, p, Luu, Lxu)."""
    b = P1 @ ck + p1
    M = Hk + Ek.T @ P1 @ Ek
    M = 0.5 * (M + M.T)
    Luu = np.linalg.cholesky(M[:m, :m])
    Lxu = np.linalg.solve(Luu, M[:m, m:]).T
    lp = hk + Ek.T @ b
    lu = np.linalg.solve(Luu, lp[:m])
    P = M[m:, m:] - Lxu @ Lxu.T
    return 0.5 * (P + P.T), lp[m:] - Lxu @ lu, Luu, Lxu


def value_functions(n, m, N, Ek, ck, Hk, hk):
    """The global (P_k, p_k), k = 0 .. N."""
    P, p = [None] * (N + 1), [None] * (N + 1)
    P[N], p[N] = Hk[N], hk[N]
    for k in range(N - 1, -1, -1):
        P[k], p[k], _, _ = _stage(m, Ek[k], ck[k], Hk[k], hk[k], P[k + 1], p[k + 1])
    return P, p


def segment_costates(n, m, N, Ek, ck, Hk, hk, w, segs, terminal_in_last=True):
    """lambda_k, k = 0 .. N, of the solution w by the segment recursion.

    ``segs``: (start, length) of the device segments, covering [0, N).
    ``terminal_in_last`` = False treats the last segment like an inner one: it
    starts from P = 0 and takes the terminal costate H_N x_N + h_N as its end
    costate (a segment of full length under the recursion for t)."""
    P, p = value_functions(n, m, N, Ek, ck, Hk, hk)
    lam = [None] * (N + 1)
    for j, (N0, L) in enumerate(segs):
        N1 = N0 + L
        real = terminal_in_last and j == len(segs) - 1
        y = P[N1] @ xof(w, N1, n, m, N) + p[N1]  # the boundary costate (N1 = N: the terminal's)
        lam[N1] = y
        Pl, pl = (Hk[N], hk[N]) if real else (np.zeros((n, n)), np.zeros(n))
        t = np.zeros(n) if real else y
        for k in range(N1 - 1, N0 - 1, -1):
            Pl, pl, Luu, Lxu = _stage(m, Ek[k], ck[k], Hk[k], hk[k], Pl, pl)
            r = Ek[k].T @ t
            z = np.linalg.solve(Luu, r[:m])
            t = r[m:] - Lxu @ z
            if k > N0 or j == 0:
                lam[k] = Pl @ xof(w, k, n, m, N) + pl + t
    return lam


def open_loop_costates(n, m, N, Ek, Hk, hk, w, N0, N1, y):
    """lambda_k, N0 < k <= N1, by lambda_k = [H_k w_k + h_k]_x + A_k^T lambda_{k+1} from lambda_{N1} = y."""
    s = n + m
    lam = {N1: y}
    for k in range(N1 - 1, N0, -1):
        lam[k] = (Hk[k] @ w[k * s:(k + 1) * s] + hk[k])[m:] + Ek[k][:, m:].T @ lam[k + 1]
    return lam


def gradients(n, m, N, E, w, v, lam, mu):
    """pdplqr_adjoint's formulas on the costates lam (primal) and mu (adjoint)."""
    s = n + m
    gE, gc, gH = np.zeros(N * n * s), np.zeros(N * n), np.zeros(N * s * s + n * n)
    for k in range(N + 1):
        d = s if k < N else n
        wk, vk = w[k * s:k * s + d], v[k * s:k * s + d]
        gH[k * s * s:k * s * s + d * d] = (0.5 * (np.outer(vk, wk) + np.outer(wk, vk))).reshape(-1, order="F")
        if k < N:
            gc[k * n:(k + 1) * n] = mu[k + 1]
            gE[k * n * s:(k + 1) * n * s] = (np.outer(mu[k + 1], wk) + np.outer(lam[k + 1], vk)).reshape(-1, order="F")
    return dict(gE=gE, gc=gc, gH=gH, gh=v, gx=mu[0])
