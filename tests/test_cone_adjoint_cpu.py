"""CPU checks of the mathematics behind pdplqr_admm_project_vjp,
pdplqr_admm_adjoint_fixed_point and ConeLQRLayer (no GPU; DESIGN.md section
5.11): the closed-form transposed Jacobian of the cone projection, the
recursion built on it and that recursion's limit, each against autograd or
central differences (tests/cone_adjoint_ref.py).

Measured here (CPU, float64; rho = 10, sigma = 1e-6, alpha = 1.6):
  * run to the end (iterate change <= 1e-13, adjoint tol 1e-12), forward /
    adjoint iterations, cone margin | |x| - t | at the fixed point, cases:
      (4, 2, 6) seed 0 r 0.3   1128 / 865   2.9     all on the boundary
      (4, 2, 6) seed 0 r 0.7    676 / 553   0.107   all on the boundary
      (6, 3, 5) seed 2 r 0.8    413 / 316   0.026   all on the boundary
      (4, 2, 6) seed 1 r 1.2    124 / 116   0.156   all inactive
      (6, 3, 5) ragged          189 / 170   0.30    boundary, boundary, inactive, boundary
  * with the GPU test's stopping rules (cone_adjoint_ref.LAYER: eps = 1e-9,
    adj_tol = 1e-10, both tested every 25 iterations), the worst gradient
    error against the tight run (truncation of the two iterations):
      (4, 2, 6)   forward 100 .. 700, adjoint 100 .. 700, worst 8.3e-9
      (6, 3, 5)   forward 125 .. 275, adjoint 150 .. 275, worst 4.9e-10
"""
import os
import re

import numpy as np
import pytest
import torch

import adjoint_ref
import adjoint_rows_ref as rr
import admm_cone_ref as acr
import cone_adjoint_ref as cr
from conftest import ROOT

F64 = torch.float64
NEW_SYMBOLS = ("pdplqr_admm_project_vjp", "pdplqr_admm_adjoint_fixed_point", "pdplqr_admm_adjoint_fixed_point_info")


@pytest.fixture(scope="module", autouse=True)
def _feature():
    """What these checks are the mathematics of exists: the three symbols in
    the header and the binding's export list, the layer in the package."""
    from pdplqr import _lib, diff

    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pdplqr.h")).read(), flags=re.S)
    for nm in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + nm + r"\s*\(", txt), nm
        assert nm in _lib.EXPORTS, nm
    assert hasattr(diff, "ConeLQRLayer")


def t64(x, rg=False):
    return torch.tensor(x, dtype=F64, requires_grad=rg)


def _cone_points(rng, dim):
    """p of dimension `dim` in each of the three cases: {case: p}."""
    out = {}
    while len(out) < 3:
        p = rng.standard_normal(dim) * np.array([2.0] + [1.0] * (dim - 1))
        out.setdefault(acr.proj_cone(p)[1], p)
    return out


@pytest.mark.parametrize("dim", [2, 3, 5, 9])
def test_operator_matches_autograd(dim):
    """(a) J g of the closed form = autograd through the projection, 1e-14 of |g|."""
    rng = np.random.default_rng(dim)
    for trial in range(20):
        for case, p in _cone_points(rng, dim).items():
            g = rng.standard_normal(dim)
            pt = t64(p, True)
            out = cr.proj_cone_t(pt)
            ref_out, ref_case = acr.proj_cone(p)
            assert ref_case == case
            # (the torch restatement sums the squares in torch's order: a few ulps of the result's size)
            assert np.abs(out.detach().numpy() - ref_out).max() <= 2e-15 * np.abs(p).max()
            (ref,) = torch.autograd.grad((t64(g) * out).sum(), pt)
            mine, mcase = cr.cone_vjp(p, g)
            assert mcase == case
            err = np.linalg.norm(mine - ref.numpy()) / np.linalg.norm(g)
            assert err <= 1e-14, (dim, case, err)


def test_mixed_set_operator_matches_autograd():
    """(a) on a ragged mixed set: gv, glb, gub against autograd in v, lb, ub."""
    p, dims, cones = cr.ragged_problem()
    ncs = dims[3]
    rng = np.random.default_rng(5)
    seen = set()
    for trial in range(40):
        v = rng.standard_normal(p["lb"].size) * 1.5
        g = rng.standard_normal(v.size)
        lv = [t64(v, True), t64(p["lb"], True), t64(p["ub"], True)]
        out = cr.project_t(*lv, ncs, cones)
        ref_out, _ = acr.project(v, p["lb"], p["ub"], ncs, cones)
        assert np.abs(out.detach().numpy() - ref_out).max() <= 1e-15
        refs = torch.autograd.grad((t64(g) * out).sum(), lv)
        gv, glb, gub, cases = cr.project_vjp(v, p["lb"], p["ub"], g, ncs, cones)
        seen.update(cases)
        for nm, mine, ref in zip(("gv", "glb", "gub"), (gv, glb, gub), refs):
            err = np.linalg.norm(mine - ref.numpy()) / np.linalg.norm(g)
            assert err <= 1e-14, (nm, err)
        for (q, d) in acr.cone_rows(ncs, cones):
            assert np.all(gub[q:q + d] == 0.0)
    assert seen == {0, 1, 2}


@pytest.mark.parametrize("key", [cr.CONE_PROBLEMS[1], cr.CONE_PROBLEMS[4]], ids=str)
def test_recursion_is_the_adjoint_of_one_cone_admm_step(key):
    """(b) one application of the recursion = autograd through one dense ADMM
    step with the cone projection at the fixed point, states and inputs, 1e-13."""
    cs = cr.cone_case(key)
    p, dims, cones, rec = cs["p"], cs["dims"], cs["cones"], cs["rec"]
    rng = np.random.default_rng(1)
    a = tuple(rng.standard_normal(x.shape) for x in (cs["w"], cs["y"], cs["y"]))
    gws = p["gws"]
    ins = [t64(p[k], True) for k in cr.KEYS]
    st = [t64(cs[k], True) for k in ("w", "y", "z")]
    nxt = cr.admm_step(*ins, *st, t64(rec.rho), cr.SIGMA, cr.ALPHA, dims, cones)
    b = (gws + a[0], a[1], a[2])
    grads = torch.autograd.grad(sum((t64(bi) * ni).sum() for bi, ni in zip(b, nxt)), st + ins, allow_unused=True)
    mine = rec.apply(gws, a)
    for nm, x, ref in zip("wyz", mine, grads[:3]):
        err = adjoint_ref.rel(x, ref.numpy())
        print(key, "state", nm, err)
        assert err < 1e-13, (nm, err)
    direct = rec.gradients(gws, a)
    for k, ref in zip(cr.KEYS, grads[3:]):
        ref = np.zeros_like(p[k]) if ref is None else ref.numpy()
        err = cr.grad_err(direct[k], ref)
        print(key, "input", k, err)
        assert err < 1e-13, (k, err)


FD_STEP = 1e-6


@pytest.mark.parametrize("key", cr.CONE_PROBLEMS, ids=str)
def test_recursion_limit_matches_central_differences(key):
    """(c) run to its limit the recursion gives the derivative of the tightly
    solved fixed point: central differences (step 1e-6) of sum(gws * w) in a
    random direction of each of E, c, H, h, x0, D, lb, relative 1e-6.  The
    error is taken relative to max(|grad|, 0.1) |direction|, the scale of the
    inner product being compared (a direction nearly orthogonal to the gradient
    has a small derivative, not a more accurate one; the floor is
    cone_adjoint_ref.grad_err's, for the gradients that are exactly zero: D and
    lb of the problem whose cones are all inactive)."""
    cs = cr.cone_case(key)
    p, dims, cones = cs["p"], cs["dims"], cs["cones"]
    print(key, "margin", cs["margin"], "cases", cs["cases"], "iters", cs["iters"], cs["adj_iters"])
    assert cs["margin"] >= 1e-2
    assert cs["adj_converged"]
    rng = np.random.default_rng(11)
    for k in cr.KEYS[:7]:
        d = rng.standard_normal(p[k].shape)
        vals = []
        for sgn in (1.0, -1.0):
            pp = dict(p)
            pp[k] = p[k] + sgn * FD_STEP * d
            if k == "lb":  # (a cone row's ub is not read; box rows keep lb <= ub)
                pp["ub"] = np.maximum(p["ub"], pp["lb"])
            w = cr.admm_solve(pp, dims, cones)[0]
            vals.append(float(p["gws"] @ w))
        fd = (vals[0] - vals[1]) / (2.0 * FD_STEP)
        mine = float(cs["grads"][k].ravel() @ d.ravel())
        err = abs(fd - mine) / (max(np.linalg.norm(cs["grads"][k]), 0.1) * np.linalg.norm(d))
        print(key, k, "fd", fd, "recursion", mine, "err", err)
        assert err < 1e-6, (k, err)
        # ... and relative to the derivative itself wherever that is not tiny against the scale above
        if abs(fd) >= 1e-3 * max(np.linalg.norm(cs["grads"][k]), 0.1) * np.linalg.norm(d):
            strict = abs(fd - mine) / abs(fd)
            print(key, k, "strict", strict)
            assert strict < 1e-6, (k, strict)


def test_problems_show_both_cases():
    cases = set()
    for key in cr.CONE_PROBLEMS:
        cases.update(cr.cone_case(key)["cases"])
    assert {0, 2} <= cases


def test_no_cones_is_the_box_recursion():
    """(d) without cones the recursion is BoxLQRLayer.backward's: the state of
    tests/test_adjoint_rows_cpu.py's restatement, and the active-set gradients
    of adjoint_rows_ref.box_case within LAYER_CPU_ERR at the layer's rules."""
    from test_adjoint_rows_cpu import BOX_CASES, LAYER, Recursion

    n, m, N, seeds = BOX_CASES[0]
    worst = 0.0
    for seed in seeds:
        bc = rr.box_case(n, m, N, seed, eps_abs=LAYER["eps_abs"], max_iter=LAYER["max_iter"])
        ref = rr.box_case(n, m, N, seed)
        p = {k: bc[k] for k in cr.KEYS + ("gws",)}
        rec = cr.ConeRecursion(p, bc["dims"], [], bc["w"], bc["y"], bc["z"], bc["rho"], bc["sigma"], bc["alpha"])
        a, it, conv = rec.solve(p["gws"], LAYER["adj_tol"], LAYER["adj_max_iter"], LAYER["check_every"])
        a0, it0 = Recursion(bc).solve(bc["gws"], LAYER["adj_tol"], LAYER["adj_max_iter"], LAYER["check_every"])
        assert conv and it == it0
        for x, y in zip(a, a0):
            assert np.array_equal(x, y)
        g = rec.gradients(p["gws"], a)
        for k in cr.KEYS:
            err = adjoint_ref.rel(g[k], ref["grads"][k])
            worst = max(worst, err)
            print(seed, k, err, "adjoint iters", it)
    print("worst", worst)
    assert worst < rr.LAYER_CPU_ERR[(n, m, N)]


@pytest.mark.parametrize("shape", sorted(cr.CONE_LAYER_CPU_ERR), ids=str)
def test_recursion_at_layer_settings(shape):
    """(e) at the GPU test's stopping rules (cone_adjoint_ref.LAYER) the
    restatement's worst gradient error against the tight run is
    CONE_LAYER_CPU_ERR[shape], within a factor 2: what
    tests/test_gpu_cone_adjoint.py's tolerance is 10 times of."""
    worst = 0.0
    for key in cr.CONE_PROBLEMS:
        if key[:3] != shape:
            continue
        ly, ref = cr.cone_case(key, True), cr.cone_case(key)
        assert ly["iters"] < cr.LAYER["max_iter"] and ly["adj_converged"]
        for k in cr.KEYS:
            err = cr.grad_err(ly["grads"][k], ref["grads"][k])
            worst = max(worst, err)
            print(key, k, err, "admm iters", ly["iters"], "adjoint iters", ly["adj_iters"])
    print(shape, "worst", worst)
    assert cr.CONE_LAYER_CPU_ERR[shape] / 2 < worst < 2 * cr.CONE_LAYER_CPU_ERR[shape]
