"""CPU checks of the adjoint solve (pdplqr_adjoint): the closed-form gradients
the device evaluates agree with autograd through a dense KKT solve, and the
C ABI declares, exports and guards the entry point.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import adjoint_ref
from conftest import ROOT


def _blocks(n, m, N, E, c, H, h):
    s = n + m
    Ek = [E[k * n * s:(k + 1) * n * s].reshape(n, s, order="F") for k in range(N)]
    ck = [c[k * n:(k + 1) * n] for k in range(N)]
    Hk = [H[k * s * s:(k + 1) * s * s].reshape(s, s, order="F") for k in range(N)]
    Hk.append(H[N * s * s:].reshape(n, n, order="F"))
    hk = [h[k * s:(k + 1) * s] for k in range(N)] + [h[N * s:]]
    return Ek, ck, Hk, hk


def _value_functions(n, m, N, Ek, ck, Hk, hk):
    """Textbook Riccati recursion: (P_k, p_k), k = 0..N."""
    P, p = [None] * (N + 1), [None] * (N + 1)
    P[N], p[N] = Hk[N], hk[N]
    for k in range(N - 1, -1, -1):
        A, B = Ek[k][:, m:], Ek[k][:, :m]
        R, S, Q = Hk[k][:m, :m], Hk[k][:m, m:], Hk[k][m:, m:]
        b = P[k + 1] @ ck[k] + p[k + 1]
        Huu, Hux = R + B.T @ P[k + 1] @ B, S + B.T @ P[k + 1] @ A
        P[k] = Q + A.T @ P[k + 1] @ A - Hux.T @ np.linalg.solve(Huu, Hux)
        P[k] = 0.5 * (P[k] + P[k].T)
        p[k] = hk[k][m:] + A.T @ b - Hux.T @ np.linalg.solve(Huu, hk[k][:m] + B.T @ b)
    return P, p


def formula_gradients(n, m, N, E, c, H, h, x0, g):
    """The gradients of one problem by the adjoint formulas (the issue's
    "mathematics"): costates from dense value functions, v from a second KKT
    solve with h := g, c := 0, x0 := 0."""
    s = n + m
    t = lambda a: torch.tensor(a, dtype=torch.float64)  # noqa: E731
    w = adjoint_ref.dense_kkt_solution(t(E), t(c), t(H), t(h), t(x0)).numpy()
    v = adjoint_ref.dense_kkt_solution(t(E), t(0 * c), t(H), t(g), t(0 * x0)).numpy()
    Ek, ck, Hk, hk = _blocks(n, m, N, E, c, H, h)
    P, p = _value_functions(n, m, N, Ek, ck, Hk, hk)
    _, _, _, gk = _blocks(n, m, N, E, c, H, g)
    _, ph = _value_functions(n, m, N, Ek, [0 * x for x in ck], Hk, gk)

    def xof(a, k):
        return a[k * s + m:(k + 1) * s] if k < N else a[N * s:]

    gE, gc, gH = np.zeros_like(E), np.zeros_like(c), np.zeros_like(H)
    for k in range(N + 1):
        d = s if k < N else n
        wk, vk = w[k * s:k * s + d], v[k * s:k * s + d]
        gH[k * s * s:k * s * s + d * d] = (0.5 * (np.outer(vk, wk) + np.outer(wk, vk))).reshape(-1, order="F")
        if k < N:
            lam = P[k + 1] @ xof(w, k + 1) + p[k + 1]
            mu = P[k + 1] @ xof(v, k + 1) + ph[k + 1]
            gc[k * n:(k + 1) * n] = mu
            gE[k * n * s:(k + 1) * n * s] = (np.outer(mu, wk) + np.outer(lam, vk)).reshape(-1, order="F")
    return dict(gE=gE, gc=gc, gH=gH, gh=v, gx=ph[0])


@pytest.mark.parametrize("shape", [(3, 2, 5), (12, 4, 6)])
def test_formulas_match_autograd(shape):
    n, m, N = shape
    cs = adjoint_ref.case(n, m, N, 2, seed=3)
    for b in range(2):
        f = formula_gradients(n, m, N, *(cs[k][b] for k in ("E", "c", "H", "h", "x0", "g")))
        for key in ("gE", "gc", "gH", "gh", "gx"):
            err = adjoint_ref.rel(f[key], cs[key][b])
            print(shape, b, key, err)
            assert err < 1e-11, (key, err)


def test_abi_declares_and_exports_adjoint():
    from pdplqr import _lib

    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pdplqr.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+pdplqr_adjoint\s*\(", txt)
    assert "pdplqr_adjoint" in _lib.EXPORTS
    assert hasattr(_lib.lib(), "pdplqr_adjoint")
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True)
    if nm.returncode == 0:
        assert re.search(r"\bT pdplqr_adjoint$", nm.stdout, flags=re.M)


def test_adjoint_rejects_null_handle_without_gpu():
    from pdplqr import _lib

    L = _lib.lib()
    buf = np.zeros(4)
    p = C.c_void_p(buf.ctypes.data)
    assert L.pdplqr_adjoint(None, p, p, None, None, None, None, None, _lib.PDPLQR_MEM_HOST) == -1
    assert L.pdplqr_last_error()
