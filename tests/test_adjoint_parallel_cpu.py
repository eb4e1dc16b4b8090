"""CPU checks of pdplqr_adjoint_parallel: the segment form of the costates
(tests/adjoint_parallel_ref.py, the recursion k_seg_costate runs) reproduces
the closed form P_k x_k + p_k on long segments of unstable dynamics, the
gradients assembled from it agree with autograd through a dense KKT solve, and
the C ABI declares, exports and guards the entry point.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import adjoint_parallel_ref as apr
import adjoint_ref
from conftest import ROOT

N64 = (12, 4, 64)
# device segments of the N = 64 horizon: one segment (its t passes 64 stages),
# segments of 8, unequal lengths with a one-stage segment
SEGMENTATIONS = {
    "one-64": ([(0, 64)], False),
    "eight-8": ([(8 * j, 8) for j in range(8)], True),
    "unequal": ([(0, 7), (7, 1), (8, 20), (28, 36)], True),
}


def _problem():
    n, m, N = N64
    E, c, H, h, x0, g = (a[0] for a in adjoint_ref.random_problem(n, m, N, 1, seed=5))
    t = lambda a: torch.tensor(a, dtype=torch.float64)  # noqa: E731
    w = adjoint_ref.dense_kkt_solution(t(E), t(c), t(H), t(h), t(x0)).numpy()
    v = adjoint_ref.dense_kkt_solution(t(E), t(0 * c), t(H), t(g), t(0 * x0)).numpy()
    return E, c, H, h, x0, g, w, v


@pytest.fixture(scope="module")
def prob():
    return _problem()


def _closed_form(n, m, N, Ek, ck, Hk, hk, w):
    P, p = apr.value_functions(n, m, N, Ek, ck, Hk, hk)
    return [P[k] @ apr.xof(w, k, n, m, N) + p[k] for k in range(N + 1)]


def _worst(a, b, ks):
    return max(np.linalg.norm(a[k] - b[k]) / np.linalg.norm(b[k]) for k in ks)


@pytest.mark.parametrize("name", list(SEGMENTATIONS))
def test_segment_costates_match_closed_form(prob, name):
    n, m, N = N64
    E, c, H, h, x0, g, w, v = prob
    segs, term = SEGMENTATIONS[name]
    Ek, ck, Hk, hk = apr.blocks(n, m, N, E, c, H, h)
    _, _, _, gk = apr.blocks(n, m, N, E, c, H, g)
    zk = [0 * x for x in ck]
    for what, sol, lin, off in (("lambda", w, hk, ck), ("mu", v, gk, zk)):
        ref = _closed_form(n, m, N, Ek, off, Hk, lin, sol)
        got = apr.segment_costates(n, m, N, Ek, off, Hk, lin, sol, segs, terminal_in_last=term)
        err = _worst(got, ref, range(N + 1))
        print(name, what, err)
        assert err < 1e-11, (name, what, err)


def test_open_loop_form_fails_the_bound(prob):
    """The bound separates the two forms: the open-loop recursion over the same
    64-stage segment is off by orders of magnitude more."""
    n, m, N = N64
    E, c, H, h, x0, g, w, v = prob
    Ek, ck, Hk, hk = apr.blocks(n, m, N, E, c, H, h)
    ref = _closed_form(n, m, N, Ek, ck, Hk, hk, w)
    ol = apr.open_loop_costates(n, m, N, Ek, Hk, hk, w, 0, N, ref[N])
    err = _worst(ol, ref, range(1, N + 1))
    print("open loop, L = 64:", err)
    assert err > 1e-9


@pytest.mark.parametrize("name", list(SEGMENTATIONS))
def test_gradients_from_segment_costates_match_autograd(prob, name):
    n, m, N = N64
    cs = adjoint_ref.case(n, m, N, 1, seed=5)
    E, c, H, h, x0, g, w, v = prob
    segs, term = SEGMENTATIONS[name]
    Ek, ck, Hk, hk = apr.blocks(n, m, N, E, c, H, h)
    _, _, _, gk = apr.blocks(n, m, N, E, c, H, g)
    lam = apr.segment_costates(n, m, N, Ek, ck, Hk, hk, w, segs, terminal_in_last=term)
    mu = apr.segment_costates(n, m, N, Ek, [0 * x for x in ck], Hk, gk, v, segs, terminal_in_last=term)
    f = apr.gradients(n, m, N, E, w, v, lam, mu)
    for key in ("gE", "gc", "gH", "gh", "gx"):
        err = adjoint_ref.rel(f[key], cs[key][0])
        print(name, key, err)
        assert err < 1e-11, (key, err)


def test_abi_declares_and_exports_adjoint_parallel():
    from pdplqr import _lib

    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pdplqr.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+pdplqr_adjoint_parallel\s*\(", txt)
    assert "pdplqr_adjoint_parallel" in _lib.EXPORTS
    assert hasattr(_lib.lib(), "pdplqr_adjoint_parallel")
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True)
    if nm.returncode == 0:
        assert re.search(r"\bT pdplqr_adjoint_parallel$", nm.stdout, flags=re.M)


def test_adjoint_parallel_rejects_null_handle_without_gpu():
    from pdplqr import _lib

    L = _lib.lib()
    buf = np.zeros(4)
    p = C.c_void_p(buf.ctypes.data)
    assert L.pdplqr_adjoint_parallel(None, p, p, None, None, None, None, None, _lib.PDPLQR_MEM_HOST) == -1
    assert L.pdplqr_last_error()
