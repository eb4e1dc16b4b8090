"""CPU checks of the mathematics behind pdplqr_adjoint_rows and BoxLQRLayer
(no GPU): the closed-form row gradients the device evaluates, the hand-written
fixed-point adjoint recursion of the layer's backward, and that recursion's
limit, each against autograd (tests/adjoint_rows_ref.py).

Measured here (CPU, float64; rho = 10, sigma = 1e-6, alpha = 1.6, u-box rows
of half-width 0.4), the figures tests/test_gpu_box_layer.py takes its settings
from:
  * run to the end (iterate change <= 1e-14, adj_tol = 1e-13):
      (3, 2, 6)   seeds 4, 5, 7: forward 77..86 iterations, adjoint 68..84,
                  worst gradient error 2.1e-13
      (12, 4, 4)  seeds 1, 2, 5: forward 166..214 iterations, adjoint 144..165,
                  worst gradient error 7.7e-13
  * with the layer test's stopping rules (LAYER below: eps_abs = 1e-9, adj_tol =
    1e-10, both tested every 25 iterations), where truncation, not rounding,
    sets the error:
      (3, 2, 6)   forward 75 iterations, adjoint 75, worst error 2.2e-12
      (12, 4, 4)  forward 100..150 iterations, adjoint 125, worst error 3.0e-10
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import adjoint_ref
import adjoint_rows_ref as rr
from conftest import ROOT
from test_adjoint_cpu import formula_gradients

F64 = torch.float64


def closed_forms(n, m, N, ncs, E, c, H, h, x0, D, rho, g, wbar, sigma, gws, gvs):
    """pdplqr_adjoint_rows' outputs of one problem by its formulas, dense numpy
    per stage: (gradients, ws)."""
    s = n + m
    d_off, y_off = rr.offsets(n, m, N, ncs)
    Ht, ht, rhs = H.copy(), h - sigma * wbar, gws.copy()
    Dk = []
    for k in range(N + 1):
        d = s if k < N else n
        Dk.append(D[d_off[k]:d_off[k + 1]].reshape(int(ncs[k]), d, order="F"))
        rk, gk = rho[y_off[k]:y_off[k + 1]], g[y_off[k]:y_off[k + 1]]
        Hk = H[k * s * s:k * s * s + d * d].reshape(d, d, order="F")
        Hs = 0.5 * (Hk + Hk.T) + sigma * np.eye(d) + Dk[k].T @ (rk[:, None] * Dk[k])
        Ht[k * s * s:k * s * s + d * d] = Hs.reshape(-1, order="F")
        ht[k * s:k * s + d] -= Dk[k].T @ (rk * gk)
        rhs[k * s:k * s + d] += Dk[k].T @ gvs[y_off[k]:y_off[k + 1]]
    t = lambda a: torch.tensor(a, dtype=F64)  # noqa: E731
    w = adjoint_ref.dense_kkt_solution(t(E), t(c), t(Ht), t(ht), t(x0)).numpy()
    f = formula_gradients(n, m, N, E, c, Ht, ht, x0, rhs)
    v = f["gh"]
    f["gD"], f["gg"], f["grho"] = np.zeros_like(D), np.zeros_like(rho), np.zeros_like(rho)
    for k in range(N + 1):
        d = s if k < N else n
        ys = slice(y_off[k], y_off[k + 1])
        wk, vk = w[k * s:k * s + d], v[k * s:k * s + d]
        r, e = Dk[k] @ vk, Dk[k] @ wk - g[ys]
        f["gD"][d_off[k]:d_off[k + 1]] = (np.outer(rho[ys] * e, vk) + np.outer(rho[ys] * r + gvs[ys], wk)).reshape(-1, order="F")
        f["gg"][ys] = -rho[ys] * r
        f["grho"][ys] = r * e
    return f, w


CASES = [(3, 2, 5, (1, 0, 2, 1, 2, 1), 0.0), (12, 4, 4, (4, 4, 4, 4, 2), 0.1), (5, 3, 3, (2, 0, 3, 1), 0.05)]


@pytest.mark.parametrize("case", CASES, ids=lambda cse: "-".join(map(str, cse[:3])))
def test_closed_forms_match_autograd(case):
    n, m, N, ncs, sigma = case
    cs = rr.case(n, m, N, 2, ncs, seed=3, sigma=sigma)
    for b in range(2):
        args = [cs[k][b] for k in ("E", "c", "H", "h", "x0", "D", "rho", "g", "wbar")]
        f, w = closed_forms(n, m, N, ncs, *args, sigma, cs["gws"][b], cs["gvs"][b])
        assert adjoint_ref.rel(w, cs["ws"][b]) < 1e-10
        for key in rr.ROW_KEYS:
            err = adjoint_ref.rel(f[key], cs[key][b])
            print(case, b, key, err)
            assert err < 1e-10, (key, err)
        # the identities of include/pdplqr.h: autograd with ys, zs, inv_rho, wbar as leaves
        t = lambda a, rg=False: torch.tensor(a, dtype=F64, requires_grad=rg)  # noqa: E731
        lv = [t(cs[k][b], True) for k in ("ys", "zs", "irho", "wbar")]
        Df = rr.dense_D(t(cs["D"][b]), n, m, N, ncs)
        wt = rr.x_update(*[t(cs[k][b]) for k in ("E", "c", "H", "h", "x0")], Df, t(cs["rho"][b]),
                         lv[1] - lv[2] * lv[0], lv[3], sigma)
        loss = (t(cs["gws"][b]) * wt).sum() + (t(cs["gvs"][b]) * (Df @ wt)).sum()
        gy, gz, gir, gwb = [x.numpy() if x is not None else 0 * lv[3].detach().numpy()
                            for x in torch.autograd.grad(loss, lv, allow_unused=True)]
        ident = {"ys": (-cs["irho"][b] * f["gg"], gy), "zs": (f["gg"], gz), "inv_rho": (-cs["ys"][b] * f["gg"], gir)}
        for key, (mine, ref) in ident.items():
            assert adjoint_ref.rel(mine, ref) < 1e-10, key
        if sigma:
            assert adjoint_ref.rel(-sigma * f["gh"], gwb) < 1e-10
        else:
            assert np.all(gwb == 0)


# ---- the fixed-point adjoint of the box-constrained solve ---------------------

class Recursion:
    """BoxLQRLayer.backward restated on dense numpy for ONE problem at the
    fixed point (w, y, z) of rr.box_case."""

    def __init__(self, bc):
        self.bc = bc
        n, m, N, ncs = bc["dims"]
        t = lambda a: torch.tensor(a, dtype=F64)  # noqa: E731
        self.rho = np.full(bc["y"].shape, bc["rho"])
        with torch.no_grad():
            self.Df = rr.dense_D(t(bc["D"]), n, m, N, ncs)
            Kp, _, self.nw = rr.penalised_system(*[t(bc[k]) for k in ("E", "c", "H", "h", "x0")], self.Df, t(self.rho),
                                                 t(0 * bc["y"]), t(0 * bc["w"]), bc["sigma"])
            self.Ki = torch.linalg.inv(Kp).numpy()[:self.nw, :self.nw]
            self.Df = self.Df.numpy()
        tt = bc["z"] + bc["y"] / self.rho
        self.M = ((tt > bc["lb"]) & (tt < bc["ub"])).astype(float)
        self.lo, self.hi = tt <= bc["lb"], tt >= bc["ub"]

    def cotangents(self, gws, a):
        bw, by, bz = gws + a[0], a[1], a[2]
        q = bz - self.rho * by
        return bw, by, bz, q, self.rho * by + self.M * q

    def apply(self, gws, a):
        """a <- dl/ds + J^T a, with the x-update's adjoint as pdplqr_adjoint_rows gives it."""
        al, sg = self.bc["alpha"], self.bc["sigma"]
        bw, by, bz, q, bvr = self.cotangents(gws, a)
        gh = -self.Ki @ (al * bw + self.Df.T @ (al * bvr))
        gg = -self.rho * (self.Df @ gh)
        return ((1 - al) * bw - sg * gh, by + self.M * q / self.rho - gg / self.rho, (1 - al) * bvr + gg)

    def gradients(self, gws, a):
        """The final call: gradients of the eight inputs at the cotangents of a."""
        bc = self.bc
        n, m, N, ncs = bc["dims"]
        al = bc["alpha"]
        bw, by, bz, q, bvr = self.cotangents(gws, a)
        f, _ = closed_forms(n, m, N, ncs, *[bc[k] for k in ("E", "c", "H", "h", "x0", "D")], self.rho,
                            bc["z"] - bc["y"] / self.rho, bc["w"], bc["sigma"], al * bw, al * bvr)
        return dict(E=f["gE"], c=f["gc"], H=f["gH"], h=f["gh"], x0=f["gx"], D=f["gD"], lb=q * self.lo, ub=q * self.hi)

    def solve(self, gws, adj_tol, max_iter, check_every=1):
        a = tuple(np.zeros_like(x) for x in (self.bc["w"], self.bc["y"], self.bc["y"]))
        for it in range(1, max_iter + 1):
            an = self.apply(gws, a)
            ch = max(np.abs(x - y).max() for x, y in zip(an, a))
            a = an
            if it % check_every == 0 and ch <= adj_tol * max(np.abs(x).max() for x in a):
                break
        return a, it


def test_recursion_is_the_adjoint_of_one_admm_step():
    bc = rr.box_case(3, 2, 6, 4)
    rec = Recursion(bc)
    rng = np.random.default_rng(1)
    a = tuple(rng.standard_normal(x.shape) for x in (bc["w"], bc["y"], bc["y"]))
    gws = bc["gws"]
    t = lambda x, rg=False: torch.tensor(x, dtype=F64, requires_grad=rg)  # noqa: E731
    ins = [t(bc[k], True) for k in rr.BOX_KEYS]
    st = [t(bc[k], True) for k in ("w", "y", "z")]
    nxt = rr.admm_step(*ins, *st, t(rec.rho), bc["sigma"], bc["alpha"], bc["dims"])
    b = (gws + a[0], a[1], a[2])
    grads = torch.autograd.grad(sum((t(bi) * ni).sum() for bi, ni in zip(b, nxt)), st + ins)
    mine = rec.apply(gws, a)
    for nm, x, ref in zip("wyz", mine, grads[:3]):
        err = adjoint_ref.rel(x, ref.numpy())
        print("state", nm, err)
        assert err < 1e-10, (nm, err)
    direct = rec.gradients(gws, a)
    for k, ref in zip(rr.BOX_KEYS, grads[3:]):
        err = adjoint_ref.rel(direct[k], ref.numpy())
        print("input", k, err)
        assert err < 1e-10, (k, err)


# (n, m, N, seeds): the cases of tests/test_gpu_box_layer.py
BOX_CASES = [(3, 2, 6, (4, 5, 7)), (12, 4, 4, (1, 2, 5))]


@pytest.mark.parametrize("case", BOX_CASES, ids=lambda cse: "-".join(map(str, cse[:3])))
def test_recursion_limit_matches_active_set(case):
    """The recursion's limit is the gradient of the active-set KKT solve.  The
    inputs are strictly complementary on the reference (asserted: margin >=
    1e-2); bound 1e-10 at adj_tol = 1e-13, measured 2.1e-13 and 7.7e-13
    at 165 iterations at most (module docstring)."""
    n, m, N, seeds = case
    for seed in seeds:
        bc = rr.box_case(n, m, N, seed)
        act = bc["at_lb"] | bc["at_ub"]
        print(case, seed, "margin", bc["margin"], "active", int(act.sum()), "of", act.size, "admm iters", bc["iters"])
        assert bc["margin"] >= 1e-2
        assert 0.25 <= act.mean() <= 0.75
        assert adjoint_ref.rel(bc["w"], bc["ws"]) < 1e-10  # the ADMM fixed point is the active-set optimum
        rec = Recursion(bc)
        a, it = rec.solve(bc["gws"], 1e-13, 5000)
        g = rec.gradients(bc["gws"], a)
        for k in rr.BOX_KEYS:
            err = adjoint_ref.rel(g[k], bc["grads"][k])
            print(case, seed, k, err, "adjoint iters", it)
            assert err < 1e-10, (k, err)


# BoxLQRLayer's settings in tests/test_gpu_box_layer.py
LAYER = dict(eps_abs=1e-9, max_iter=2000, adj_tol=1e-10, adj_max_iter=2000, check_every=25)


@pytest.mark.parametrize("case", BOX_CASES, ids=lambda cse: "-".join(map(str, cse[:3])))
def test_recursion_at_layer_settings(case):
    """The same with the stopping rules the GPU layer test runs with (LAYER):
    the error this restatement reaches (rr.LAYER_CPU_ERR: 2.2e-12 and 3.0e-10,
    truncation of the two iterations) is what that test's tolerance is 10 times
    of.  Asserted here within a factor 2 of the recorded figure."""
    n, m, N, seeds = case
    worst = 0.0
    for seed in seeds:
        bc = rr.box_case(n, m, N, seed, eps_abs=LAYER["eps_abs"], max_iter=LAYER["max_iter"])
        ref = rr.box_case(n, m, N, seed)
        assert bc["iters"] < LAYER["max_iter"]
        assert adjoint_ref.rel(bc["w"], ref["ws"]) < 2 * rr.LAYER_CPU_WS_ERR[(n, m, N)]
        rec = Recursion(bc)
        a, it = rec.solve(bc["gws"], LAYER["adj_tol"], LAYER["adj_max_iter"], LAYER["check_every"])
        assert it < LAYER["adj_max_iter"]
        g = rec.gradients(bc["gws"], a)
        for k in rr.BOX_KEYS:
            err = adjoint_ref.rel(g[k], ref["grads"][k])
            worst = max(worst, err)
            print(case, seed, k, err, "admm iters", bc["iters"], "adjoint iters", it)
    print(case, "worst", worst)
    assert worst < 2 * rr.LAYER_CPU_ERR[(n, m, N)]


def test_abi_declares_and_exports_adjoint_rows():
    from pdplqr import _lib

    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pdplqr.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+pdplqr_adjoint_rows\s*\(", txt)
    assert "pdplqr_adjoint_rows" in _lib.EXPORTS
    L = _lib.lib()
    buf = np.zeros(4)
    p = C.c_void_p(buf.ctypes.data)
    assert L.pdplqr_adjoint_rows(None, p, p, p, None, None, None, None, None, None, None, None, None, 0) == -1
    assert L.pdplqr_last_error()
