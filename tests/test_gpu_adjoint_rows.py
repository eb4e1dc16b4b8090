"""GPU checks of pdplqr_adjoint_rows (csrc/adjoint.hip,
csrc/kernels_adjoint_rows.hip): the adjoint of the penalised x-update against
autograd through a dense KKT solve whose H~, h~ are built in torch from
(H, D, rho, g, wbar, sigma) (tests/adjoint_rows_ref.py).

Tolerance: the project's parity bound 1e-9 (tests/test_gpu_adjoint.py), as the
Frobenius relative error of each gradient array over the whole batch, every
array checked on its own.
"""
import numpy as np
import pytest

import adjoint_ref
import adjoint_rows_ref as rr

pytestmark = pytest.mark.gpu

TOL = 1e-9
KEYS = rr.ROW_KEYS

# (n, m, N, batch, ncs)
CASES = [
    (12, 4, 3, 3, (4, 4, 4, 0)),      # the C5 row layout
    (12, 4, 3, 3, (4, 4, 4, 2)),      # terminal rows
    (5, 3, 4, 2, (2, 0, 3, 1, 2)),    # ragged rows, a rowless stage, odd sizes, 8-byte stores
    (3, 2, 1, 2, (1, 1)),             # N = 1
    (24, 8, 5, 2, (8,) * 5 + (0,)),   # s = 32
    (36, 8, 3, 2, (3,) * 3 + (1,)),   # s = 44
    (40, 24, 2, 1, (5, 5, 0)),        # s = 64
    (4, 2, 7, 70, (2,) * 7 + (0,)),   # grid tails
    # the kernel's lanes-per-row choices the shapes above do not reach (they take 4 and 16)
    (4, 2, 7, 2, (3,) * 7 + (1,)),    # 22 rows in the tile: 8 lanes per row
    (4, 2, 7, 2, (10,) * 8),          # 80 rows: 2 lanes per row
    (4, 2, 7, 2, (40,) * 7 + (3,)),   # 283 rows: 1 lane per row, two passes of the block
    (4, 2, 2, 1, (1200, 1, 0)),       # 1201 rows in one tile: 37.7 KB of the 40 KB LDS limit, five passes
]
C5, RAGGED = CASES[0], CASES[2]


def _id(cse):
    return "-".join(map(str, cse[:4])) + "-nc" + "".join(map(str, cse[4]))


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from pdplqr import device_count

    assert device_count() > 0, "no HIP device visible: GPU tests must run on an MI355X"


def _sizes(n, m, N, ncs):
    s = n + m
    d_off, y_off = rr.offsets(n, m, N, ncs)
    return dict(gE=N * n * s, gc=N * n, gH=N * s * s + n * n, gh=N * s + n, gx=n, gD=d_off[-1], gg=y_off[-1],
                grho=y_off[-1])


def _solved(cs, cse, **kw):
    """A serial handle that has run the penalised x-update of the case: (solver, ws)."""
    from pdplqr import BatchedLQRSolver

    n, m, N, batch, ncs = cse
    kw.setdefault("keep_factors", True)
    bs = BatchedLQRSolver(n, m, N, batch, ncs=list(ncs), **kw)
    bs.set_model(cs["E"], cs["c"], cs["H"], cs["h"], np.ascontiguousarray(cs["D"]))
    bs.update_problem_data(np.ascontiguousarray(cs["wbar"]), cs["ys"], cs["zs"], cs["irho"], sigma=cs["sigma"])
    bs.backward(cs["rho"])
    ws = np.zeros((batch, N * (n + m) + n))
    bs.forward(cs["x0"], ws)
    return bs, ws


def _blank(cse, want=KEYS):
    n, m, N, batch, ncs = cse
    return {k: (np.full((batch, v), 7.0) if k in want else None) for k, v in _sizes(n, m, N, ncs).items()}


def _rows_host(bs, cse, ws, cs, want=KEYS, gvs=True):
    out = _blank(cse, want)
    bs.adjoint_rows(ws, cs["rho"], np.ascontiguousarray(cs["gws"]), cs["gvs"] if gvs is True else gvs, **out)
    return out


def _check(out, cs, what):
    for k in KEYS:
        err = adjoint_ref.rel(out[k], cs[k])
        print(what, k, err)
        assert err < TOL, (what, k, err)


@pytest.mark.parametrize("cse", CASES, ids=_id)
def test_rows_match_autograd(cse):
    cs = rr.case(*cse)
    bs, ws = _solved(cs, cse)
    assert adjoint_ref.rel(ws, cs["ws"]) < TOL
    _check(_rows_host(bs, cse, ws, cs), cs, _id(cse))


def test_rows_with_sigma():
    """sigma = 0.1, random proximal centre: the gradients are those of the
    problem with H + sigma I + D^T R D, h - sigma wbar - D^T R g."""
    cse = RAGGED
    cs = rr.case(*cse, seed=5, sigma=0.1)
    bs, ws = _solved(cs, cse)
    assert adjoint_ref.rel(ws, cs["ws"]) < TOL
    _check(_rows_host(bs, cse, ws, cs), cs, "sigma")


@pytest.mark.parametrize("cse", [C5, RAGGED], ids=_id)
def test_rows_gvs_none_is_zero(cse):
    cs = rr.case(*cse)
    bs, ws = _solved(cs, cse)
    a = _rows_host(bs, cse, ws, cs, gvs=None)
    b = _rows_host(bs, cse, ws, cs, gvs=np.zeros_like(cs["gvs"]))
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("cse", [C5, RAGGED], ids=_id)
def test_rows_single_outputs_and_repeat(cse):
    cs = rr.case(*cse)
    bs, ws = _solved(cs, cse)
    full = _rows_host(bs, cse, ws, cs)
    again = _rows_host(bs, cse, ws, cs)
    for k in KEYS:
        assert np.array_equal(again[k], full[k]), k
        one = _rows_host(bs, cse, ws, cs, want=(k,))
        assert np.array_equal(one[k], full[k]), k
    bs.adjoint_rows(ws, cs["rho"], np.ascontiguousarray(cs["gws"]), cs["gvs"])  # nothing requested: OK


@pytest.mark.parametrize("cse", [C5, RAGGED], ids=_id)
def test_rows_device_buffers(cse):
    import torch

    cs = rr.case(*cse)
    bs, ws = _solved(cs, cse)
    host = _rows_host(bs, cse, ws, cs)
    n, m, N, batch, ncs = cse
    dev = {k: torch.full((batch, v), 7.0, dtype=torch.float64, device="cuda") for k, v in _sizes(n, m, N, ncs).items()}
    t = lambda a: torch.tensor(a, device="cuda")  # noqa: E731
    bs.adjoint_rows(t(ws), t(cs["rho"]), t(cs["gws"]), t(cs["gvs"]), **dev)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in dev.items()}
    _check(out, cs, "device")
    for k in KEYS:
        assert np.array_equal(out[k], host[k]), k


def test_no_rows_equals_adjoint():
    shape = (5, 3, 4, 2)
    n, m, N, batch = shape
    cse = shape + ((0,) * (N + 1),)
    cs = adjoint_ref.case(*shape)
    from pdplqr import BatchedLQRSolver

    bs = BatchedLQRSolver(n, m, N, batch, keep_factors=True)
    bs.set_model(cs["E"], cs["c"], cs["H"], cs["h"])
    bs.update_problem_data(np.ascontiguousarray(cs["wbar"]), sigma=0.0)
    bs.backward()
    ws = np.zeros((batch, N * (n + m) + n))
    bs.forward(cs["x0"], ws)
    g = np.ascontiguousarray(cs["g"])
    a = {k: v for k, v in _blank(cse).items() if k in KEYS[:5]}
    bs.adjoint(ws, g, **a)
    b = {k: v for k, v in _blank(cse).items() if k in KEYS[:5]}
    bs.adjoint_rows(ws, None, g, None, **b)
    for k in KEYS[:5]:
        assert np.array_equal(a[k], b[k]), k
        assert adjoint_ref.rel(b[k], cs[k]) < TOL


@pytest.mark.parametrize("cse", [C5, RAGGED, CASES[5]], ids=_id)
def test_handle_state_preserved_with_rows(cse):
    n, m, N, batch, ncs = cse
    cs = rr.case(*cse)
    bs, ws = _solved(cs, cse)
    vf = [bs.value_function(0, k) for k in range(N + 1)]
    _rows_host(bs, cse, ws, cs)
    ws2 = np.zeros_like(ws)
    bs.forward(cs["x0"], ws2)
    assert np.array_equal(ws2, ws)
    for k in range(N + 1):
        P, p = bs.value_function(0, k)
        assert np.array_equal(P, vf[k][0]) and np.array_equal(p, vf[k][1])
    # a new penalty target on the kept factor: same answer as a fresh handle
    zs2 = np.random.default_rng(11).standard_normal(cs["zs"].shape)
    bs.update_problem_data(np.ascontiguousarray(cs["wbar"]), cs["ys"], zs2, cs["irho"], sigma=cs["sigma"])
    bs.backward_without_factorization(cs["rho"])
    ws3 = np.zeros_like(ws)
    bs.forward(cs["x0"], ws3)
    fresh, ws4 = _solved(dict(cs, zs=zs2), cse)
    assert adjoint_ref.rel(ws3, ws4) < TOL
    assert adjoint_ref.rel(ws3, ws) > 1e-6  # the new target did change the solution


def test_rows_errors():
    from pdplqr import BatchedLQRSolver, _lib

    L = _lib.lib()
    cse = CASES[7]
    n, m, N, batch, ncs = cse
    cs = rr.case(*cse)
    gws = np.ascontiguousarray(cs["gws"])

    def refused(bs, ws, code, rho=cs["rho"], c=cse):
        out = _blank(c)
        with pytest.raises(_lib.PdplqrError) as ei:
            bs.adjoint_rows(ws, rho, gws if c is cse else np.zeros_like(ws), None, **out)
        assert ei.value.code == code, ei.value
        assert L.pdplqr_last_error()
        assert all(np.all(v == 7.0) for v in out.values())  # nothing was written

    bs, ws = _solved(cs, cse)
    refused(bs, ws, -1, rho=None)  # NULL rho with rows
    _check(_rows_host(bs, cse, ws, cs), cs, "after a refusal")
    bs, wk = _solved(cs, cse, keep_factors=False)
    refused(bs, wk, -4)
    w2 = np.zeros_like(wk)
    bs.forward(cs["x0"], w2)
    assert np.array_equal(w2, wk)
    # before backward
    bs = BatchedLQRSolver(n, m, N, batch, keep_factors=True, ncs=list(ncs))
    bs.set_model(cs["E"], cs["c"], cs["H"], cs["h"], np.ascontiguousarray(cs["D"]))
    bs.update_problem_data(np.ascontiguousarray(cs["wbar"]), cs["ys"], cs["zs"], cs["irho"], sigma=0.0)
    refused(bs, ws, -4)
    # the other solver kinds
    bs, wp = _solved(cs, cse, solver="parallel", num_segments=2)
    assert adjoint_ref.rel(wp, cs["ws"]) < TOL
    refused(bs, wp, -5)
    bs = BatchedLQRSolver(n, m, N, batch, solver="kkt", keep_factors=False, ncs=list(ncs))
    refused(bs, ws, -5)
    # one stage with more rows than the rows kernel's 40 KB LDS tile holds
    # (32 bytes per row + 16 (n + m) + 16 at one stage per block: 1276 rows at n + m = 6)
    wide = (4, 2, 2, 1, (1300, 1, 0))
    cw = dict(zip(("E", "c", "H", "h", "x0", "gws"), adjoint_ref.random_problem(*wide[:4], 0)))
    cw.update(zip(("D", "rho", "ys", "zs", "gvs"), rr.random_rows(*wide, 0)))
    cw.update(irho=1.0 / cw["rho"], wbar=np.zeros_like(cw["h"]), sigma=0.0)
    bs, ww = _solved(cw, wide)
    refused(bs, ww, -5, rho=cw["rho"], c=wide)
    w2 = np.zeros_like(ww)
    bs.forward(cw["x0"], w2)
    assert np.array_equal(w2, ww)
    # n + m > 64
    big = (60, 8, 2, 1, (2, 2, 0))
    bs = BatchedLQRSolver(*big[:4], keep_factors=True, ncs=list(big[4]))
    refused(bs, np.zeros((1, 2 * 68 + 60)), -5, rho=np.ones((1, 4)), c=big)
