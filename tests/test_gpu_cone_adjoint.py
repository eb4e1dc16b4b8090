"""GPU checks of pdplqr_admm_project_vjp, pdplqr_admm_adjoint_fixed_point and
pdplqr.ConeLQRLayer (csrc/kernels_cone.hip, csrc/kernels_fpadj.hip,
pdplqr/diff.py) against the CPU restatement
tests/cone_adjoint_ref.py.

The cone problems, seeds and stopping rules are those of
tests/test_cone_adjoint_cpu.py (cone_adjoint_ref.LAYER: eps = 1e-9, adj_tol =
1e-10, tests every 25 iterations), where the dense restatement of the same two
iterations reaches a worst gradient error against its tight run of 8.3e-9 at
(4, 2, 6) and 5.0e-10 at (6, 3, 5) (cone_adjoint_ref.CONE_LAYER_CPU_ERR:
truncation of the iterations, not rounding).  The tolerance here is 10 times
that, for the device's summation order, on every gradient array of every
problem (cone_adjoint_ref.grad_err).
"""
import functools

import numpy as np
import pytest

import adjoint_rows_ref as rr
import admm_cone_ref as acr
import cone_adjoint_ref as cr
from test_adjoint_rows_cpu import BOX_CASES
from test_adjoint_rows_cpu import LAYER as BOX_LAYER

pytestmark = pytest.mark.gpu

INVALID, STATE, UNSUPPORTED = -1, -4, -5
OUT_NAMES = ("gE", "gc", "gH", "gh", "gx", "gD", "glb", "gub")


def _box_inputs():
    """The (3, 2, 6) box problems of tests/test_gpu_box_layer.py, a batch of 2."""
    n, m, N, seeds = BOX_CASES[0]
    bcs = [rr.box_case(n, m, N, seed) for seed in seeds[:2]]
    P = {k: np.ascontiguousarray(np.stack([bc[k] for bc in bcs])) for k in cr.KEYS + ("gws",)}
    return (n, m, N), bcs[0]["dims"][3], P


def _rows_run():
    """admm_solve + the x-update + adjoint_rows on a fresh handle that never
    calls the new entry points: every output, host arrays."""
    from pdplqr import BatchedLQRSolver

    (n, m, N), ncs, P = _box_inputs()
    B = P["h"].shape[0]
    bs = BatchedLQRSolver(n, m, N, B, keep_factors=True, ncs=list(ncs))
    wt, ws, ys, zs, rho = _fixed_point(bs, P, BOX_LAYER["eps_abs"], BOX_LAYER["max_iter"])
    gvs = np.random.default_rng(3).standard_normal(ys.shape)
    sizes = dict(gE=P["E"], gc=P["c"], gH=P["H"], gh=P["h"], gx=P["x0"], gD=P["D"], gg=ys, grho=ys)
    outs = {k: np.full_like(v, np.nan) for k, v in sizes.items()}
    bs.adjoint_rows(wt, rho, P["gws"], gvs, **outs)
    bs.close()
    return dict(outs, ws=ws, ys=ys, zs=zs, wt=wt)


_BASELINE = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from pdplqr import device_count

    assert device_count() > 0, "no HIP device visible: GPU tests must run on an MI355X"
    # the nothing-changes guard's stored run: before this module's first call of a new entry point
    # (no other module calls them)
    _BASELINE.update(_rows_run())


def _fixed_point(bs, P, eps, max_iter, cones=()):
    """BoxLQRLayer.forward's steps on a BatchedLQRSolver (host arrays): the solve
    from a zero start at rho = 10, then the explicit x-update at the returned
    point.  (wt, ws, ys, zs, rho)."""
    bs.set_model(P["E"], P["c"], P["H"], P["h"], P["D"])
    if len(cones):
        bs.set_cones(cones)
    B = P["h"].shape[0]
    rho = np.full(P["lb"].shape, cr.RHO)
    ws, ys, zs = np.zeros_like(P["h"]), np.zeros_like(P["lb"]), np.zeros_like(P["lb"])
    info = bs.admm_solve(P["x0"], P["lb"], P["ub"], rho, ws, ys, zs, sigma=cr.SIGMA, alpha=cr.ALPHA,
                         max_iter=max_iter, check_every=25, eps_abs=eps, eps_rel=0.0, adaptive_rho=False)
    assert info["converged"].all(), info
    bs.update_problem_data(ws, ys, zs, 1.0 / rho, cr.SIGMA)
    bs.backward(rho)
    wt = bs.forward(P["x0"], np.zeros_like(ws))
    assert B == wt.shape[0]
    return wt, ws, ys, zs, rho


def _outs(P, names=OUT_NAMES, fill=np.nan):
    like = dict(gE=P["E"], gc=P["c"], gH=P["H"], gh=P["h"], gx=P["x0"], gD=P["D"], glb=P["lb"], gub=P["lb"])
    return {k: np.full_like(like[k], fill) for k in names}


# ---------------------------------------------------------------------------
# 1. pdplqr_admm_project_vjp
# ---------------------------------------------------------------------------
VJP_NCS = [18, 0, 11, 9]
# 6/3, N = 3: box rows around cones of dimension 2, 3 and s + 1 = 10; a stage without rows;
# a cone of dimension 10 then a box row; a terminal cone of dimension n + 1 = 7 between box rows
VJP_CONES = [(0, 1, 2), (0, 4, 3), (0, 8, 10), (2, 0, 10), (3, 1, 7)]


def _crafted():
    """A batch of 8 [ny] vectors (tests/test_gpu_cone.py's patterns): problem b
    gives every cone pattern b -- inside, |x| = t, |x| = -t, the polar cone, a
    generic boundary point, x = 0 with t > 0, t < 0, t = 0 -- cone i at
    magnitude 1e-100 / 1e-3 / 1 / 1e100 by (b + i) % 4, lb zero on the even
    cones (the ties are then exact) and random on the odd ones; box rows inside,
    outside and on their bounds.  gout: unit normal times 1e-50 / 1 / 1e50."""
    g = np.random.default_rng(7)
    ny = int(sum(VJP_NCS))
    scales = [1e-100, 1e-3, 1.0, 1e100]
    v, lb, ub, gout = (np.zeros((8, ny)) for _ in range(4))
    for b in range(8):
        lb[b] = -g.uniform(0.5, 1.5, ny)
        ub[b] = g.uniform(0.5, 1.5, ny)
        v[b] = g.choice([0.0, 0.3, -0.7, 3.0, -3.0], ny)
        v[b, ::5] = ub[b, ::5]
        v[b, 1::7] = lb[b, 1::7]
        lb[b, 3] = ub[b, 3] = v[b, 3] = 0.25  # a box row with lb == ub, met exactly
        gout[b] = g.standard_normal(ny)
        for i, (q, d) in enumerate(acr.cone_rows(VJP_NCS, VJP_CONES)):
            sc = scales[(b + i) % 4]
            x = np.zeros(d - 1)
            x[0] = 3.0
            if d > 2:
                x[-1] = 4.0
            nx = 5.0 if d > 2 else 3.0
            if b in (5, 6, 7):
                x[:] = 0.0
            t = {0: 2 * nx, 1: nx, 2: -nx, 3: -2 * nx, 4: 0.25 * nx, 5: 1.0, 6: -1.0, 7: 0.0}[b]
            if b == 4:
                x = g.standard_normal(d - 1)
            l = sc * g.standard_normal(d) if i % 2 else np.zeros(d)
            lb[b, q:q + d] = ub[b, q:q + d] = l
            v[b, q:q + d] = l + sc * np.concatenate([[t], x])
            gout[b, q:q + d] *= [1e-50, 1.0, 1e50][(b + i) % 3]
    return v, lb, ub, gout


def test_project_vjp_matches_operator():
    import torch
    from pdplqr import BatchedLQRSolver

    v, lb, ub, gout = _crafted()
    rows = acr.cone_rows(VJP_NCS, VJP_CONES)
    box = np.ones(v.shape[1], dtype=bool)
    for (q, d) in rows:
        box[q:q + d] = False
    bs = BatchedLQRSolver(6, 3, 3, 8, ncs=VJP_NCS)
    bs.set_cones(VJP_CONES)
    out = bs.project(v, lb, ub)
    got = bs.project_vjp(v, lb, ub, gout)
    seen, ties = set(), set()
    for b in range(8):
        gv, glb, gub, cases = cr.project_vjp(v[b], lb[b], ub[b], gout[b], VJP_NCS, VJP_CONES)
        for nm, ref in (("gv", gv), ("glb", glb), ("gub", gub)):
            assert np.array_equal(got[nm][b][box], ref[box]), (nm, b)  # box rows: to the bit
        for (q, d), case in zip(rows, cases):
            sl = slice(q, q + d)
            p = v[b, sl] - lb[b, sl]
            nx = acr.cone_norm(p[1:])
            if nx > 0 and nx == p[0]:
                ties.add("t")
            if nx > 0 and nx == -p[0]:
                ties.add("-t")
            # the case the projection took on the same bits
            if np.array_equal(out[b, sl], v[b, sl]):
                assert np.array_equal(got["gv"][b, sl], gout[b, sl]), (b, q)
                assert case == 0
            elif np.array_equal(out[b, sl], lb[b, sl]):
                assert np.all(got["gv"][b, sl] == 0.0), (b, q)
                assert case == 1
            else:
                assert case == 2
            gmax = np.max(np.abs(gout[b, sl]))
            # d = xh . g_x: at most 64 products on xh (a root of <= 64 squares, a division), then five
            # operations per entry: within (64 + 40) 2^-53 = 1.2e-14 of max|g|; eight times that
            for nm, ref in (("gv", gv), ("glb", glb)):
                err = np.max(np.abs(got[nm][b, sl] - ref[sl]))
                assert err <= 1e-13 * gmax, (nm, b, q, d, case, err, gmax)
            assert np.all(got["gub"][b, sl] == 0.0)
            seen.add(case)
    assert seen == {0, 1, 2} and ties == {"t", "-t"}
    # any output may be left out; device buffers give the host buffers' bits
    only = bs.project_vjp(v, lb, ub, gout, want=("glb",))
    assert set(only) == {"glb"} and np.array_equal(only["glb"], got["glb"])
    dev = torch.device("cuda", 0)
    dgot = bs.project_vjp(*[torch.from_numpy(a).to(dev) for a in (v, lb, ub, gout)])
    torch.cuda.synchronize()
    for nm in ("gv", "glb", "gub"):
        assert np.array_equal(dgot[nm].cpu().numpy(), got[nm]), nm
    bs.set_cones([])  # cleared: every row a box row
    allbox = bs.project_vjp(v, lb, ub, gout)
    assert np.array_equal(allbox["gv"], np.where((lb < v) & (v < ub), gout, 0.0))
    assert np.array_equal(allbox["glb"], np.where(v <= lb, gout, 0.0))
    assert np.array_equal(allbox["gub"], np.where(v >= ub, gout, 0.0))
    bs.close()


# ---------------------------------------------------------------------------
# 2. pdplqr_admm_adjoint_fixed_point without cones: BoxLQRLayer's backward
# ---------------------------------------------------------------------------
def test_fixed_point_without_cones_is_the_box_layer_backward():
    import torch
    from pdplqr import BatchedLQRSolver, BoxLQRLayer

    (n, m, N), ncs, P = _box_inputs()
    B = P["h"].shape[0]
    L = BOX_LAYER
    layer = BoxLQRLayer(n, m, N, B, ncs, rho=cr.RHO, sigma=cr.SIGMA, alpha=cr.ALPHA, eps=L["eps_abs"],
                        max_iter=L["max_iter"], adj_tol=L["adj_tol"], adj_max_iter=L["adj_max_iter"],
                        check_every=L["check_every"])
    leaves = [torch.tensor(P[k], device="cuda", requires_grad=True) for k in cr.KEYS]
    ws = layer(*leaves)
    (torch.tensor(P["gws"], device="cuda") * ws).sum().backward()
    bs = BatchedLQRSolver(n, m, N, B, keep_factors=True, ncs=list(ncs))
    wt, ws2, ys, zs, rho = _fixed_point(bs, P, L["eps_abs"], L["max_iter"])
    assert np.array_equal(ws2, ws.detach().cpu().numpy())
    outs = _outs(P)
    bs.admm_adjoint_fixed_point(wt, ys, zs, P["lb"], P["ub"], rho, P["gws"], cr.SIGMA, cr.ALPHA, L["adj_tol"],
                                L["adj_max_iter"], L["check_every"], **outs)
    info = bs.admm_adjoint_fixed_point_info()
    print("iterations", info["iters"], "layer", layer.adjoint_iterations, "resid", info["resid"])
    assert info["converged"].all()
    assert int(info["iters"].max()) == layer.adjoint_iterations
    tol = 10 * rr.LAYER_CPU_ERR[(n, m, N)]
    for k, nm, leaf in zip(cr.KEYS, OUT_NAMES, leaves):
        ref = leaf.grad.cpu().numpy().reshape(B, -1)
        for b in range(B):
            err = cr.grad_err(outs[nm][b], ref[b])
            print(k, b, err)
            assert err < tol, (k, b, err)
        # the box rows repeat the layer's torch statements in their order: the same bits
        assert np.array_equal(outs[nm], ref), k
    # device buffers give the host buffers' bits
    dev = torch.device("cuda", 0)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    douts = {k: torch.full_like(d(v), float("nan")) for k, v in outs.items()}
    bs.admm_adjoint_fixed_point(d(wt), d(ys), d(zs), d(P["lb"]), d(P["ub"]), d(rho), d(P["gws"]), cr.SIGMA, cr.ALPHA,
                                L["adj_tol"], L["adj_max_iter"], L["check_every"], **douts)
    torch.cuda.synchronize()
    for nm in OUT_NAMES:
        assert np.array_equal(douts[nm].cpu().numpy(), outs[nm]), nm
    # the handle's factor, record and lp are the caller's: adjoint_rows still gives the baseline's bits
    gvs = np.random.default_rng(3).standard_normal(ys.shape)
    again = {k: np.full_like(_BASELINE[k], np.nan) for k in ("gE", "gc", "gH", "gh", "gx", "gD", "gg", "grho")}
    bs.adjoint_rows(wt, rho, P["gws"], gvs, **again)
    for k, v in again.items():
        assert np.array_equal(v, _BASELINE[k]), k
    bs.close()
    layer.close()


# ---------------------------------------------------------------------------
# 3. pdplqr_admm_adjoint_fixed_point with cones
# ---------------------------------------------------------------------------
CONE_BATCHES = {"4-2-6": cr.GPU_BATCH, "6-3-5-ragged": [cr.CONE_PROBLEMS[4]]}


@functools.lru_cache(maxsize=None)
def _cone_batch(name):
    keys = CONE_BATCHES[name]
    probs = [cr.problem(k) for k in keys]
    P = {k: np.ascontiguousarray(np.stack([p[0][k] for p in probs])) for k in cr.KEYS + ("gws",)}
    return keys, probs[0][1], probs[0][2], P


@functools.lru_cache(maxsize=None)
def _cone_direct(name, max_iter=None):
    """The direct call on the batch at LAYER's rules: (outs, info, ws)."""
    from pdplqr import BatchedLQRSolver

    keys, (n, m, N, ncs), cones, P = _cone_batch(name)
    L = cr.LAYER
    bs = BatchedLQRSolver(n, m, N, len(keys), keep_factors=True, ncs=list(ncs))
    wt, ws, ys, zs, rho = _fixed_point(bs, P, L["eps_abs"], L["max_iter"], cones)
    outs = _outs(P)
    bs.admm_adjoint_fixed_point(wt, ys, zs, P["lb"], P["ub"], rho, P["gws"], cr.SIGMA, cr.ALPHA, L["adj_tol"],
                                max_iter or L["adj_max_iter"], L["check_every"], **outs)
    info = bs.admm_adjoint_fixed_point_info()
    bs.close()
    return outs, info, ws


@pytest.mark.parametrize("name", sorted(CONE_BATCHES))
def test_fixed_point_with_cones_matches_restatement(name):
    keys, (n, m, N, ncs), cones, P = _cone_batch(name)
    outs, info, _ = _cone_direct(name)
    tol = 10 * cr.CONE_LAYER_CPU_ERR[(n, m, N)]
    print(name, "iterations", info["iters"], "converged", info["converged"], "resid", info["resid"])
    conerow = np.zeros(P["lb"].shape[1], dtype=bool)
    for (q, d) in acr.cone_rows(ncs, cones):
        conerow[q:q + d] = True
    for b, key in enumerate(keys):
        ref, ly = cr.cone_case(key), cr.cone_case(key, True)
        assert info["converged"][b]
        assert info["iters"][b] == ly["adj_iters"], (key, info["iters"][b], ly["adj_iters"])
        assert info["resid"][b, 0] <= cr.LAYER["adj_tol"] * info["resid"][b, 1]
        for k, nm in zip(cr.KEYS, OUT_NAMES):
            err = cr.grad_err(outs[nm][b], ref["grads"][k])
            print(key, k, err)
            assert err < tol, (key, k, err)
        assert np.all(outs["gub"][b][conerow] == 0.0)
    # (the ragged case has box rows active at their lower bound)
    assert conerow.all() or np.any(outs["glb"][:, ~conerow] != 0.0)


def test_frozen_problem_keeps_its_results():
    """The r = 1.2 problem (cones inactive) passes its test hundreds of
    iterations before the others; what it had then is what the call returns."""
    outs, info, _ = _cone_direct("4-2-6")
    its = info["iters"]
    print("iterations", its)
    assert its[2] + 200 <= min(its[0], its[1])
    early, einfo, _ = _cone_direct("4-2-6", max_iter=int(its[2]))
    assert einfo["iters"][2] == its[2] and einfo["converged"][2] and not einfo["converged"][:2].any()
    for nm in OUT_NAMES:
        assert np.array_equal(early[nm][2], outs[nm][2]), nm
    assert np.array_equal(einfo["resid"][2], info["resid"][2])


# ---------------------------------------------------------------------------
# 4. ConeLQRLayer
# ---------------------------------------------------------------------------
def _cone_layer(name, **kw):
    from pdplqr import ConeLQRLayer

    keys, (n, m, N, ncs), cones, P = _cone_batch(name)
    L = cr.LAYER
    cfg = dict(rho=cr.RHO, cones=cones, sigma=cr.SIGMA, alpha=cr.ALPHA, eps=L["eps_abs"], max_iter=L["max_iter"],
               adj_tol=L["adj_tol"], adj_max_iter=L["adj_max_iter"], check_every=L["check_every"])
    cfg.update(kw)
    return ConeLQRLayer(n, m, N, len(keys), ncs, **cfg), P


def _leaves(P, need=cr.KEYS):
    import torch

    return [torch.tensor(P[k], device="cuda", requires_grad=(k in need)) for k in cr.KEYS]


def test_cone_layer_autograd_gives_the_direct_call():
    import torch

    layer, P = _cone_layer("4-2-6")
    outs, info, ws_direct = _cone_direct("4-2-6")
    leaves = _leaves(P)
    ws = layer(*leaves)
    assert layer.admm_info["converged"].all()
    assert np.array_equal(ws.detach().cpu().numpy(), ws_direct)
    (torch.tensor(P["gws"], device="cuda") * ws).sum().backward()
    assert layer.adjoint_iterations == int(info["iters"].max())
    assert np.array_equal(layer.adjoint_info["iters"], info["iters"])
    for nm, leaf in zip(OUT_NAMES, leaves):
        assert np.array_equal(leaf.grad.cpu().numpy().reshape(outs[nm].shape), outs[nm]), nm
    # only h and lb need gradients: nothing else is asked for
    leaves = _leaves(P, need=("h", "lb"))
    ws = layer(*leaves)
    hd, asked = layer.handle, []
    inner = hd.admm_adjoint_fixed_point

    def recording(*a, **kw):
        asked.append([x is not None for x in a[12:]])
        return inner(*a, **kw)

    hd.admm_adjoint_fixed_point = recording
    try:
        (torch.tensor(P["gws"], device="cuda") * ws).sum().backward()
    finally:
        del hd.admm_adjoint_fixed_point
    assert asked == [[False, False, False, True, False, False, True, False]]
    for k, nm, leaf in zip(cr.KEYS, OUT_NAMES, leaves):
        if k in ("h", "lb"):
            assert np.array_equal(leaf.grad.cpu().numpy().reshape(outs[nm].shape), outs[nm]), k
        else:
            assert leaf.grad is None, k
    layer.close()


def test_cone_layer_without_cones_is_the_box_layer_forward():
    from pdplqr import BoxLQRLayer, ConeLQRLayer

    (n, m, N), ncs, P = _box_inputs()
    B = P["h"].shape[0]
    cfg = dict(rho=cr.RHO, sigma=cr.SIGMA, alpha=cr.ALPHA, eps=BOX_LAYER["eps_abs"], max_iter=BOX_LAYER["max_iter"])
    box, cone = BoxLQRLayer(n, m, N, B, ncs, **cfg), ConeLQRLayer(n, m, N, B, ncs, cones=[], **cfg)
    a, b = box(*_leaves(P)), cone(*_leaves(P))
    assert np.array_equal(a.detach().cpu().numpy(), b.detach().cpu().numpy())
    box.close()
    cone.close()


def test_cone_layer_guards():
    layer, P = _cone_layer("4-2-6", max_iter=2)
    leaves = _leaves(P)
    ws = layer(*leaves)
    assert not layer.admm_info["converged"].all()
    with pytest.raises(RuntimeError, match="converge"):
        ws.sum().backward()
    layer.close()
    layer, P = _cone_layer("4-2-6", max_iter=2, allow_unconverged=True, adj_max_iter=3)
    layer(*leaves).sum().backward()
    assert leaves[3].grad is not None and layer.adjoint_iterations == 3
    assert not layer.adjoint_info["converged"].any()
    layer.close()
    layer, P = _cone_layer("6-3-5-ragged")
    leaves = _leaves(P)
    first = layer(*leaves)
    layer(*leaves)
    with pytest.raises(RuntimeError, match="factorization"):
        first.sum().backward()
    layer.close()


# ---------------------------------------------------------------------------
# 5. error codes; a refused call writes nothing
# ---------------------------------------------------------------------------
def _raises(code, fn, *a, **k):
    from pdplqr import PdplqrError

    with pytest.raises(PdplqrError) as ei:
        fn(*a, **k)
    assert ei.value.code == code, ei.value


def _call(bs, P, wt, ys, zs, rho, outs):
    bs.admm_adjoint_fixed_point(wt, ys, zs, P["lb"], P["ub"], rho, P["gws"], cr.SIGMA, cr.ALPHA, 1e-8, 100, 25, **outs)


def test_fixed_point_refusals_write_nothing():
    from pdplqr import BatchedLQRSolver

    keys, (n, m, N, ncs), cones, P = _cone_batch("6-3-5-ragged")
    ws, ys = np.zeros_like(P["h"]), np.zeros_like(P["lb"])
    rho = np.full_like(ys, cr.RHO)

    def refused(bs, code, Q=P, w=ws, y=ys, r=rho):
        outs = _outs(Q, fill=7.0)
        _raises(code, _call, bs, Q, w, y, y, r, outs)
        for nm, v in outs.items():
            assert np.all(v == 7.0), nm

    bs = BatchedLQRSolver(n, m, N, 1, keep_factors=True, ncs=list(ncs))
    _raises(STATE, bs.admm_adjoint_fixed_point_info)  # before any call
    bs.set_model(P["E"], P["c"], P["H"], P["h"], P["D"])
    bs.set_cones(cones)
    refused(bs, STATE)  # before backward
    _raises(STATE, bs.admm_adjoint_fixed_point_info)
    wt, _, ysol, zsol, _ = _fixed_point(bs, P, 1e-6, 4000, cones)
    q0, d0 = acr.cone_rows(ncs, cones)[0]
    bad_rho = rho.copy()
    bad_rho[0, q0 + 1] = 2.0 * cr.RHO  # rho varies within the first cone
    outs = _outs(P, fill=7.0)
    _raises(INVALID, _call, bs, P, wt, ysol, zsol, bad_rho, outs)
    assert all(np.all(v == 7.0) for v in outs.values())
    _raises(INVALID, bs.admm_adjoint_fixed_point, wt, ysol, zsol, P["lb"], P["ub"], rho, P["gws"], cr.SIGMA, 2.5, 1e-8,
            100, 25, **outs)  # alpha outside (0, 2)
    assert all(np.all(v == 7.0) for v in outs.values())
    _raises(STATE, bs.admm_adjoint_fixed_point_info)  # nothing ran yet
    _call(bs, P, wt, ysol, zsol, rho, outs)  # the same handle then serves the call
    assert all(np.isfinite(v).all() for v in outs.values())
    assert bs.admm_adjoint_fixed_point_info()["iters"][0] > 0
    bs.close()

    bs = BatchedLQRSolver(n, m, N, 1, solver="parallel", num_segments=2, keep_factors=True, ncs=list(ncs))
    refused(bs, UNSUPPORTED)
    bs.close()
    bs = BatchedLQRSolver(n, m, N, 1, keep_factors=False, ncs=list(ncs))
    refused(bs, UNSUPPORTED)
    bs.close()
    bs = BatchedLQRSolver(n, m, N, 1, keep_factors=True)  # no rows
    refused(bs, UNSUPPORTED, w=ws, y=np.zeros((1, 1)), r=np.ones((1, 1)))
    bs.close()
    nb, mb, Nb = 40, 25, 1  # n + m = 65
    Qb = dict(E=np.zeros((1, Nb * nb * 65)), c=np.zeros((1, Nb * nb)), H=np.zeros((1, Nb * 65 * 65 + nb * nb)),
              h=np.zeros((1, Nb * 65 + nb)), x0=np.zeros((1, nb)), D=np.zeros((1, 65)), lb=np.zeros((1, 1)),
              ub=np.zeros((1, 1)), gws=np.zeros((1, Nb * 65 + nb)))
    bs = BatchedLQRSolver(nb, mb, Nb, 1, keep_factors=True, ncs=[1, 0])
    refused(bs, UNSUPPORTED, Q=Qb, w=Qb["h"], y=Qb["lb"], r=np.ones((1, 1)))
    bs.close()


# ---------------------------------------------------------------------------
# 6. nothing changes for a handle that never calls the new entry points
# ---------------------------------------------------------------------------
def test_handles_without_the_new_calls_keep_their_bits():
    """admm_solve + adjoint_rows on a fresh handle, after this process has run
    the new entry points, against the run stored before it had (_gpu)."""
    now = _rows_run()
    assert set(now) == set(_BASELINE)
    for k, v in now.items():
        assert np.array_equal(v, _BASELINE[k]), k
