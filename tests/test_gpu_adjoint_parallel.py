"""GPU checks of pdplqr_adjoint_parallel (csrc/adjoint_parallel.hip,
csrc/kernels_adjoint_parallel.hip) and of LQRLayer(solver="parallel") against
autograd through a dense KKT solve (tests/adjoint_ref.py) and, on long
segments of unstable dynamics, against pdplqr_adjoint on a SERIAL handle.

Tolerance: the bound of tests/test_gpu_adjoint.py, 1e-9 as the Frobenius
relative error of each gradient array over the whole batch.
"""
import ctypes as C

import numpy as np
import pytest

import adjoint_ref

pytestmark = pytest.mark.gpu

TOL = 1e-9
KEYS = ("gE", "gc", "gH", "gh", "gx")

# (n, m, N, batch, num_segments, segment_len, condensed)
CASES = [
    (12, 4, 8, 3, 2, 2, "CHOLESKY"),   # the compiled n = 12 scan, 4 device segments
    (5, 3, 9, 2, 3, 2, "CHOLESKY"),    # odd sizes, unequal segments, 8-byte stores
    (3, 2, 3, 2, 2, 0, "CHOLESKY"),    # a one-stage segment
    (24, 8, 8, 2, 2, 0, "CHOLESKY"),   # s = 32, the 4-wave family
    (36, 8, 6, 2, 2, 0, "CHOLESKY"),   # the 33..64 kernels
    (40, 24, 4, 1, 2, 0, "CHOLESKY"),  # s = 64
    (4, 2, 16, 70, 4, 3, "CHOLESKY"),  # grid tails, more problems than a block covers
    (12, 4, 8, 2, 1, 4, "LU"),         # LU condensed form (num_segments = 1 is allowed there only)
]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from pdplqr import device_count

    assert device_count() > 0, "no HIP device visible: GPU tests must run on an MI355X"


def _sizes(n, m, N):
    s = n + m
    return dict(gE=N * n * s, gc=N * n, gH=N * s * s + n * n, gh=N * s + n, gx=n)


def _handle(cs, shape, sigma=0.0, forward=True, **kw):
    """A handle (PARALLEL unless told otherwise) that has solved the case: (solver, ws)."""
    from pdplqr import BatchedLQRSolver

    n, m, N, batch = shape
    kw.setdefault("solver", "parallel")
    kw.setdefault("keep_factors", True)
    if kw["solver"] == "parallel":
        kw.setdefault("num_segments", 2)
    bs = BatchedLQRSolver(n, m, N, batch, **kw)
    bs.set_model(cs["E"], cs["c"], cs["H"], cs["h"])
    bs.update_problem_data(np.ascontiguousarray(cs["wbar"]), sigma=sigma)
    bs.backward()
    ws = np.zeros((batch, N * (n + m) + n))
    if forward:
        bs.forward(cs["x0"], ws)
    return bs, ws


def _adjoint_host(bs, shape, ws, g, want=KEYS, call="adjoint_parallel"):
    n, m, N, batch = shape
    out = {k: (np.full((batch, v), 7.0) if k in want else None) for k, v in _sizes(n, m, N).items()}
    getattr(bs, call)(ws, np.ascontiguousarray(g), **out)
    return out


def _check(out, ref, what):
    for k in KEYS:
        err = adjoint_ref.rel(out[k], ref[k])
        print(what, k, err)
        assert err < TOL, (what, k, err)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_matches_autograd(case):
    n, m, N, batch, ns, sl, cond = case
    shape = (n, m, N, batch)
    cs = adjoint_ref.case(*shape)
    bs, ws = _handle(cs, shape, num_segments=ns, segment_len=sl, condensed=cond)
    assert adjoint_ref.rel(ws, cs["ws"]) < TOL
    out = _adjoint_host(bs, shape, ws, cs["g"])
    _check(out, cs, case)
    gH = out["gH"]
    s = n + m
    for k in range(N):  # exactly symmetric
        blk = gH[:, k * s * s:(k + 1) * s * s].reshape(batch, s, s)
        assert np.array_equal(blk, blk.transpose(0, 2, 1))


@pytest.mark.parametrize("N,kw", [(128, dict(num_segments=2, load_balancing=False, segment_len=64)),
                                  (256, dict(num_segments=2))], ids=["two-64-stage-segments", "auto-plan-256"])
def test_long_segments_match_serial(N, kw):
    """A = I + 0.3 randn has spectral radius ~ 1.9: an open-loop costate
    recursion loses seven digits over a 64-stage segment.  The comparator is
    pdplqr_adjoint on a SERIAL handle (closed-form costates from Lxx)."""
    from pdplqr import _lib

    shape = (12, 4, N, 2)
    n, m, _, batch = shape
    E, c, H, h, x0, g = adjoint_ref.random_problem(*shape, seed=5)
    cs = dict(E=E, c=c, H=H, h=h, x0=x0, wbar=np.zeros_like(h))
    ser, ws_s = _handle(cs, shape, solver="serial")
    ref = _adjoint_host(ser, shape, ws_s, g, call="adjoint")
    par, ws_p = _handle(cs, shape, **kw)
    if "segment_len" in kw:
        seg = np.zeros(64, dtype=np.int32)
        S = _lib.lib().pdplqr_debug_parallel(par.handle.h, 5, C.c_void_p(seg.ctypes.data), C.c_longlong(seg.nbytes))
        assert S == 2 and list(seg[:4]) == [0, 64, 64, 64]
    assert adjoint_ref.rel(ws_p, ws_s) < TOL
    _check(_adjoint_host(par, shape, ws_p, g), ref, ("long", N))


@pytest.mark.parametrize("case", [CASES[0], CASES[1]], ids=lambda c: "-".join(map(str, c)))
def test_device_buffers_and_null_outputs(case):
    import torch

    n, m, N, batch, ns, sl, cond = case
    shape = (n, m, N, batch)
    cs = adjoint_ref.case(*shape)
    bs, ws = _handle(cs, shape, num_segments=ns, segment_len=sl, condensed=cond)
    host = _adjoint_host(bs, shape, ws, cs["g"])
    again = _adjoint_host(bs, shape, ws, cs["g"])
    for k in KEYS:  # two consecutive calls: the same bits
        assert np.array_equal(again[k], host[k]), k
    dev = {k: torch.full((batch, v), 7.0, dtype=torch.float64, device="cuda") for k, v in _sizes(n, m, N).items()}
    bs.adjoint_parallel(torch.tensor(ws, device="cuda"), torch.tensor(cs["g"], device="cuda"), **dev)
    torch.cuda.synchronize()
    for k in KEYS:
        assert np.array_equal(dev[k].cpu().numpy(), host[k]), k
    # some outputs NULL: the rest keep their bits, the NULL ones' sentinels stay
    for want in (("gc", "gh", "gx"), ("gE",), ("gH",), ("gx",)):
        dev = {k: torch.full((batch, v), 7.0, dtype=torch.float64, device="cuda") for k, v in _sizes(n, m, N).items()}
        args = {k: (t if k in want else None) for k, t in dev.items()}
        bs.adjoint_parallel(torch.tensor(ws, device="cuda"), torch.tensor(cs["g"], device="cuda"), **args)
        torch.cuda.synchronize()
        for k in KEYS:
            got = dev[k].cpu().numpy()
            assert np.array_equal(got, host[k]) if k in want else np.all(got == 7.0), (want, k)
        one = _adjoint_host(bs, shape, ws, cs["g"], want=want)
        for k in want:
            assert np.array_equal(one[k], host[k]), (want, k)
    bs.adjoint_parallel(ws, np.ascontiguousarray(cs["g"]))  # nothing requested: OK


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[4]], ids=lambda c: "-".join(map(str, c)))
def test_handle_state_preserved(case):
    n, m, N, batch, ns, sl, cond = case
    shape = (n, m, N, batch)
    kw = dict(num_segments=ns, segment_len=sl, condensed=cond)
    cs = adjoint_ref.case(*shape)
    bs, ws = _handle(cs, shape, **kw)
    status = bs.status().copy()
    _adjoint_host(bs, shape, ws, cs["g"])
    assert np.array_equal(bs.status(), status)
    ws2 = np.zeros_like(ws)
    bs.forward(cs["x0"], ws2)
    assert np.array_equal(ws2, ws)
    # a new linear term on the kept factor: same answer as a fresh handle
    wbar = np.random.default_rng(11).standard_normal(ws.shape)
    bs.update_problem_data(wbar, sigma=0.0)
    bs.backward_without_factorization()
    ws3 = np.zeros_like(ws)
    bs.forward(cs["x0"], ws3)
    fresh, ws4 = _handle(cs, shape, **kw)
    assert adjoint_ref.rel(ws3, ws4) < TOL
    # ... and with a linear term that does change (sigma > 0 in both handles)
    a, wa = _handle(dict(cs, wbar=wbar), shape, sigma=0.05, **kw)
    _adjoint_host(a, shape, wa, cs["g"])
    wbar2 = np.random.default_rng(12).standard_normal(ws.shape)
    a.update_problem_data(wbar2, sigma=0.05)
    a.backward_without_factorization()
    wa2 = np.zeros_like(ws)
    a.forward(cs["x0"], wa2)
    b, wb2 = _handle(dict(cs, wbar=wbar2), shape, sigma=0.05, **kw)
    assert adjoint_ref.rel(wa2, wb2) < TOL


def test_works_without_a_forward():
    """After backward only, with ws from another handle's solve of the same data."""
    case = CASES[0]
    n, m, N, batch, ns, sl, cond = case
    shape = (n, m, N, batch)
    kw = dict(num_segments=ns, segment_len=sl, condensed=cond)
    cs = adjoint_ref.case(*shape)
    other, ws = _handle(cs, shape, **kw)
    full = _adjoint_host(other, shape, ws, cs["g"])
    bs, _ = _handle(cs, shape, forward=False, **kw)
    out = _adjoint_host(bs, shape, ws, cs["g"])
    _check(out, cs, "no forward")
    for k in KEYS:
        assert np.array_equal(out[k], full[k]), k
    w2 = np.zeros_like(ws)
    bs.forward(cs["x0"], w2)
    assert np.array_equal(w2, ws)


def test_refusals():
    from pdplqr import BatchedLQRSolver, _lib

    L = _lib.lib()
    shape = (4, 2, 7, 70)
    n, m, N, batch = shape
    cs = adjoint_ref.case(*shape)
    g = np.ascontiguousarray(cs["g"])

    def refused(bs, ws, code):
        out = {k: np.full((batch, v), 7.0) for k, v in _sizes(n, m, N).items()}
        with pytest.raises(_lib.PdplqrError) as ei:
            bs.adjoint_parallel(ws, g, **out)
        assert ei.value.code == code, ei.value
        assert L.pdplqr_last_error()
        assert all(np.all(v == 7.0) for v in out.values())  # nothing was written

    def still_solves(bs, ref):
        w2 = np.zeros_like(ref)
        bs.forward(cs["x0"], w2)
        assert adjoint_ref.rel(w2, ref) < TOL

    # keep_factors = 0
    bs, ws = _handle(cs, shape, keep_factors=False)
    refused(bs, ws, -4)
    still_solves(bs, ws)
    # before backward
    bs = BatchedLQRSolver(n, m, N, batch, solver="parallel", num_segments=2, keep_factors=True)
    bs.set_model(cs["E"], cs["c"], cs["H"], cs["h"])
    bs.update_problem_data(np.zeros_like(ws), sigma=0.0)
    refused(bs, ws, -4)
    bs.backward()
    still_solves(bs, cs["ws"])
    # SERIAL and KKT handles
    for kw in (dict(solver="serial", keep_factors=True), dict(solver="kkt", keep_factors=False)):
        bs, wk = _handle(cs, shape, **kw)
        refused(bs, wk, -5)
        # the protocol again (a KKT forward accumulates x0 into its right-hand side, and its
        # regularised solution is compared with its own first one)
        bs.update_problem_data(np.zeros_like(ws), sigma=0.0)
        bs.backward()
        still_solves(bs, wk)
    # constraint rows
    ncs = np.zeros(N + 1, dtype=np.int32)
    ncs[2] = 1
    bs = BatchedLQRSolver(n, m, N, batch, solver="parallel", num_segments=2, keep_factors=True, ncs=ncs)
    refused(bs, ws, -5)
    # a one-device multi-device handle
    bs, wmd = _handle(cs, shape, devices=[0])
    refused(bs, wmd, -5)
    still_solves(bs, wmd)
    # n + m > 64
    bs = BatchedLQRSolver(60, 8, 4, 1, solver="parallel", num_segments=2, keep_factors=True)
    wbig = np.zeros((1, 4 * 68 + 60))
    with pytest.raises(_lib.PdplqrError) as ei:
        bs.adjoint_parallel(wbig, wbig.copy())
    assert ei.value.code == -5 and L.pdplqr_last_error()
    # null ws / gws
    bs, ws = _handle(cs, shape)
    p = C.c_void_p(ws.ctypes.data)
    assert L.pdplqr_adjoint_parallel(bs.handle.h, None, p, None, None, None, None, None, 0) == -1
    assert L.pdplqr_adjoint_parallel(bs.handle.h, p, None, None, None, None, None, None, 0) == -1
    _check(_adjoint_host(bs, shape, ws, g), cs, "after errors")


@pytest.mark.parametrize("shape", [(12, 4, 8, 3), (5, 3, 9, 2)], ids=lambda s: "-".join(map(str, s)))
def test_layer_backward_matches_autograd(shape):
    import torch

    from pdplqr import LQRLayer, _lib

    n, m, N, batch = shape
    cs = adjoint_ref.case(*shape)
    layer = LQRLayer(n, m, N, batch, solver="parallel", num_segments=2)
    assert layer.handle.cfg.solver == _lib.PDPLQR_SOLVER_PARALLEL
    leaves = [torch.tensor(cs[k], device="cuda", requires_grad=True) for k in ("E", "c", "H", "h", "x0")]
    g = torch.tensor(cs["g"], device="cuda")
    ws = layer(*leaves)
    assert adjoint_ref.rel(ws.detach().cpu().numpy(), cs["ws"]) < TOL
    (g * ws).sum().backward()
    _check({k: t.grad.cpu().numpy() for k, t in zip(KEYS, leaves)}, cs, shape)
    # only h and x0 need gradients: only they are asked for
    asked = []
    real = layer.handle.adjoint_parallel

    def spy(ws_, gws_, *outs):
        asked.append([o is not None for o in outs])
        return real(ws_, gws_, *outs)

    layer.handle.adjoint_parallel = spy
    leaves = [torch.tensor(cs[k], device="cuda", requires_grad=(k in ("h", "x0"))) for k in ("E", "c", "H", "h", "x0")]
    (g * layer(*leaves)).sum().backward()
    assert asked == [[False, False, False, True, True]]
    assert leaves[0].grad is None and leaves[1].grad is None and leaves[2].grad is None
    assert adjoint_ref.rel(leaves[3].grad.cpu().numpy(), cs["gh"]) < TOL
    assert adjoint_ref.rel(leaves[4].grad.cpu().numpy(), cs["gx"]) < TOL


def test_layer_stale_factor_and_default_solver():
    import torch

    from pdplqr import LQRLayer, _lib

    shape = (5, 3, 9, 2)
    n, m, N, batch = shape
    cs = adjoint_ref.case(*shape)
    layer = LQRLayer(n, m, N, batch, solver="parallel", num_segments=2)
    leaves = [torch.tensor(cs[k], device="cuda", requires_grad=True) for k in ("E", "c", "H", "h", "x0")]
    first = layer(*leaves)
    second = layer(*leaves)
    with pytest.raises(RuntimeError, match="factorization"):
        first.sum().backward()
    second.sum().backward()  # the live one still differentiates
    assert leaves[3].grad is not None
    # the default-argument layer still builds a serial handle
    default = LQRLayer(n, m, N, batch)
    assert default.solver == "serial" and default.handle.cfg.solver == _lib.PDPLQR_SOLVER_SERIAL
