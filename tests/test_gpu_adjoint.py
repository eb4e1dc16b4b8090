"""GPU checks of the adjoint solve (pdplqr_adjoint, csrc/adjoint.hip and
csrc/kernels_adjoint.hip) and of the torch layer over it (pdplqr/diff.py)
against autograd through a dense KKT solve (tests/adjoint_ref.py).

Tolerance: the project's parity bound 1e-9 (tests/test_gpu_serial.py: fp64 on
both sides, different summation order), as the Frobenius relative error of
each gradient array over the whole batch, every array checked on its own.
"""
import ctypes as C

import numpy as np
import pytest

import adjoint_ref

pytestmark = pytest.mark.gpu

TOL = 1e-9
KEYS = ("gE", "gc", "gH", "gh", "gx")

# (n, m, N, batch)
SHAPES = [
    (12, 4, 3, 3),   # the compiled instance
    (5, 3, 4, 2),    # generic kernel, odd sizes (8-byte stores)
    (3, 2, 1, 2),    # N = 1: the only k + 1 is the terminal block
    (24, 8, 5, 2),   # s = 32, the one-wave boundary
    (36, 8, 3, 2),   # s = 44, the 33..64 path
    (40, 24, 2, 1),  # s = 64, the upper boundary
    (4, 2, 7, 70),   # more problems than one wave or block covers, grid tails
]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from pdplqr import device_count

    assert device_count() > 0, "no HIP device visible: GPU tests must run on an MI355X"


def _sizes(n, m, N):
    s = n + m
    return dict(gE=N * n * s, gc=N * n, gH=N * s * s + n * n, gh=N * s + n, gx=n)


def _solved(cs, shape, sigma=0.0, **kw):
    """A serial handle that has solved the case; returns (solver, ws)."""
    from pdplqr import BatchedLQRSolver

    n, m, N, batch = shape
    kw.setdefault("keep_factors", True)
    bs = BatchedLQRSolver(n, m, N, batch, **kw)
    bs.set_model(cs["E"], cs["c"], cs["H"], cs["h"])
    bs.update_problem_data(np.ascontiguousarray(cs["wbar"]), sigma=sigma)
    bs.backward()
    ws = np.zeros((batch, N * (n + m) + n))
    bs.forward(cs["x0"], ws)
    return bs, ws


def _adjoint_host(bs, shape, ws, g, want=KEYS):
    n, m, N, batch = shape
    out = {k: (np.full((batch, v), 7.0) if k in want else None) for k, v in _sizes(n, m, N).items()}
    bs.adjoint(ws, np.ascontiguousarray(g), **out)
    return out


def _check(out, cs, what):
    for k in KEYS:
        err = adjoint_ref.rel(out[k], cs[k])
        print(what, k, err)
        assert err < TOL, (what, k, err)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_adjoint_matches_autograd(shape):
    cs = adjoint_ref.case(*shape)
    bs, ws = _solved(cs, shape)
    assert adjoint_ref.rel(ws, cs["ws"]) < TOL
    _check(_adjoint_host(bs, shape, ws, cs["g"]), cs, shape)


@pytest.mark.parametrize("shape", [(12, 4, 3, 3), (5, 3, 4, 2)], ids=lambda s: "-".join(map(str, s)))
def test_adjoint_device_buffers(shape):
    import torch

    cs = adjoint_ref.case(*shape)
    bs, ws = _solved(cs, shape)
    host = _adjoint_host(bs, shape, ws, cs["g"])
    n, m, N, batch = shape
    dev = {k: torch.full((batch, v), 7.0, dtype=torch.float64, device="cuda") for k, v in _sizes(n, m, N).items()}
    bs.adjoint(torch.tensor(ws, device="cuda"), torch.tensor(cs["g"], device="cuda"), **dev)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in dev.items()}
    _check(out, cs, shape)
    for k in KEYS:
        assert np.array_equal(out[k], host[k]), k


def test_adjoint_null_outputs():
    shape = (12, 4, 3, 3)
    cs = adjoint_ref.case(*shape)
    bs, ws = _solved(cs, shape)
    full = _adjoint_host(bs, shape, ws, cs["g"])
    for k in KEYS:
        one = _adjoint_host(bs, shape, ws, cs["g"], want=(k,))
        assert np.array_equal(one[k], full[k]), k
    bs.adjoint(ws, np.ascontiguousarray(cs["g"]))  # nothing requested: OK
    shape = (5, 3, 4, 2)  # the 8-byte-store kernel
    cs = adjoint_ref.case(*shape)
    bs, ws = _solved(cs, shape)
    full = _adjoint_host(bs, shape, ws, cs["g"])
    for k in KEYS:
        assert np.array_equal(_adjoint_host(bs, shape, ws, cs["g"], want=(k,))[k], full[k]), k


@pytest.mark.parametrize("shape", [(12, 4, 3, 3), (5, 3, 4, 2)], ids=lambda s: "-".join(map(str, s)))
def test_adjoint_with_sigma(shape):
    """sigma = 0.1, random proximal centre: the gradients are those of the
    problem with H + sigma I, h - sigma wbar."""
    cs = adjoint_ref.case(*shape, seed=5, sigma=0.1)
    bs, ws = _solved(cs, shape, sigma=0.1)
    assert adjoint_ref.rel(ws, cs["ws"]) < TOL
    _check(_adjoint_host(bs, shape, ws, cs["g"]), cs, shape)


@pytest.mark.parametrize("shape", [(12, 4, 3, 3), (5, 3, 4, 2), (36, 8, 3, 2)], ids=lambda s: "-".join(map(str, s)))
def test_handle_state_preserved(shape):
    n, m, N, batch = shape
    cs = adjoint_ref.case(*shape)
    bs, ws = _solved(cs, shape)
    vf = [bs.value_function(0, k) for k in range(N + 1)]
    _adjoint_host(bs, shape, ws, cs["g"])
    ws2 = np.zeros_like(ws)
    bs.forward(cs["x0"], ws2)
    assert np.array_equal(ws2, ws)
    for k in range(N + 1):
        P, p = bs.value_function(0, k)
        assert np.array_equal(P, vf[k][0]) and np.array_equal(p, vf[k][1])
    # a new linear term on the kept factor: same answer as a fresh handle
    wbar = np.random.default_rng(11).standard_normal(ws.shape)
    bs.update_problem_data(wbar, sigma=0.0)  # sigma = 0: h~ = h, the recursion re-runs
    bs.backward_without_factorization()
    ws3 = np.zeros_like(ws)
    bs.forward(cs["x0"], ws3)
    fresh, ws4 = _solved(cs, shape)
    assert adjoint_ref.rel(ws3, ws4) < TOL
    # ... and with a linear term that does change (sigma > 0 in both handles)
    cs2 = dict(cs, wbar=wbar)
    a, wa = _solved(cs2, shape, sigma=0.05)
    _adjoint_host(a, shape, wa, cs["g"])
    wbar2 = np.random.default_rng(12).standard_normal(ws.shape)
    a.update_problem_data(wbar2, sigma=0.05)
    a.backward_without_factorization()
    wa2 = np.zeros_like(ws)
    a.forward(cs["x0"], wa2)
    b, wb2 = _solved(dict(cs, wbar=wbar2), shape, sigma=0.05)
    assert adjoint_ref.rel(wa2, wb2) < TOL


def test_adjoint_errors():
    from pdplqr import BatchedLQRSolver, _lib

    L = _lib.lib()
    shape = (4, 2, 7, 70)
    n, m, N, batch = shape
    cs = adjoint_ref.case(*shape)
    g = np.ascontiguousarray(cs["g"])

    def refused(bs, ws, code):
        out = {k: np.full((batch, v), 7.0) for k, v in _sizes(n, m, N).items()}
        with pytest.raises(_lib.PdplqrError) as ei:
            bs.adjoint(ws, g, **out)
        assert ei.value.code == code, ei.value
        assert L.pdplqr_last_error()
        assert all(np.all(v == 7.0) for v in out.values())  # nothing was written

    # keep_factors = 0
    bs, ws = _solved(cs, shape, keep_factors=False)
    refused(bs, ws, -4)
    w2 = np.zeros_like(ws)
    bs.forward(cs["x0"], w2)
    assert np.array_equal(w2, ws)
    # before backward
    bs = BatchedLQRSolver(n, m, N, batch, keep_factors=True)
    bs.set_model(cs["E"], cs["c"], cs["H"], cs["h"])
    bs.update_problem_data(np.zeros_like(ws), sigma=0.0)
    refused(bs, ws, -4)
    bs.backward()
    w2 = np.zeros_like(ws)
    bs.forward(cs["x0"], w2)
    assert adjoint_ref.rel(w2, cs["ws"]) < TOL  # the handle still solves
    # the other solver kinds
    for kw in (dict(solver="parallel", num_segments=2, keep_factors=True), dict(solver="kkt", keep_factors=False)):
        bs, wk = _solved(cs, shape, **kw)
        refused(bs, wk, -5)
        # the protocol again (a KKT forward accumulates x0 into its right-hand
        # side, as the reference's does, so a bare second forward would differ)
        bs.update_problem_data(np.zeros_like(ws), sigma=0.0)
        bs.backward()
        w2 = np.zeros_like(ws)
        bs.forward(cs["x0"], w2)
        assert adjoint_ref.rel(w2, wk) < TOL
    # constraint rows
    ncs = np.zeros(N + 1, dtype=np.int32)
    ncs[2] = 1
    bs = BatchedLQRSolver(n, m, N, batch, keep_factors=True, ncs=ncs)
    refused(bs, ws, -5)
    # n + m > 64
    big = (60, 8, 2, 1)
    bs = BatchedLQRSolver(*big, keep_factors=True)
    wbig = np.zeros((1, 2 * 68 + 60))
    with pytest.raises(_lib.PdplqrError) as ei:
        bs.adjoint(wbig, wbig.copy())
    assert ei.value.code == -5 and L.pdplqr_last_error()
    # null ws / gws
    bs, ws = _solved(cs, shape)
    p = C.c_void_p(ws.ctypes.data)
    assert L.pdplqr_adjoint(bs.handle.h, None, p, None, None, None, None, None, 0) == -1
    assert L.pdplqr_adjoint(bs.handle.h, p, None, None, None, None, None, None, 0) == -1
    _check(_adjoint_host(bs, shape, ws, g), cs, "after errors")


@pytest.mark.parametrize("shape", [(12, 4, 3, 3), (5, 3, 4, 2)], ids=lambda s: "-".join(map(str, s)))
def test_layer_backward_matches_autograd(shape):
    import torch

    from pdplqr import LQRLayer

    n, m, N, batch = shape
    cs = adjoint_ref.case(*shape)
    layer = LQRLayer(n, m, N, batch)
    leaves = [torch.tensor(cs[k], device="cuda", requires_grad=True) for k in ("E", "c", "H", "h", "x0")]
    g = torch.tensor(cs["g"], device="cuda")
    ws = layer(*leaves)
    assert adjoint_ref.rel(ws.detach().cpu().numpy(), cs["ws"]) < TOL
    (g * ws).sum().backward()
    _check({k: t.grad.cpu().numpy() for k, t in zip(KEYS, leaves)}, cs, shape)
    # only h and x0 need gradients
    leaves = [torch.tensor(cs[k], device="cuda", requires_grad=(k in ("h", "x0"))) for k in ("E", "c", "H", "h", "x0")]
    (g * layer(*leaves)).sum().backward()
    assert leaves[0].grad is None and leaves[1].grad is None and leaves[2].grad is None
    assert adjoint_ref.rel(leaves[3].grad.cpu().numpy(), cs["gh"]) < TOL
    assert adjoint_ref.rel(leaves[4].grad.cpu().numpy(), cs["gx"]) < TOL


def test_layer_detects_stale_factor():
    import torch

    from pdplqr import LQRLayer

    shape = (5, 3, 4, 2)
    n, m, N, batch = shape
    cs = adjoint_ref.case(*shape)
    layer = LQRLayer(n, m, N, batch)
    leaves = [torch.tensor(cs[k], device="cuda", requires_grad=True) for k in ("E", "c", "H", "h", "x0")]
    first = layer(*leaves)
    second = layer(*leaves)
    with pytest.raises(RuntimeError, match="factorization"):
        first.sum().backward()
    second.sum().backward()  # the live one still differentiates
    assert leaves[3].grad is not None


@pytest.mark.parametrize("shape", [(12, 4, 3, 3), (4, 2, 7, 70)], ids=lambda s: "-".join(map(str, s)))
def test_adjoint_repeatable(shape):
    cs = adjoint_ref.case(*shape)
    bs, ws = _solved(cs, shape)
    a = _adjoint_host(bs, shape, ws, cs["g"])
    b = _adjoint_host(bs, shape, ws, cs["g"])
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
