"""CPU restatement of the cone-aware fixed-point adjoint (numpy / torch float64)
for the tests of pdplqr_admm_project_vjp, pdplqr_admm_adjoint_fixed_point and
ConeLQRLayer.  Nothing here comes from the product.

  * ``cone_vjp`` / ``project_vjp``: the closed-form transposed Jacobian of the
    projection onto the mixed set (box rows: the 0/1 mask and the two bound
    masks; the rows of a cone, with p = v - lb = (t, x), r = |x|:
    r <= t: J = I; r <= -t: J = 0; otherwise, xh = x / r, d = xh . g_x,
    (J g)_t = (g_t + d) / 2, (J g)_x = (g_t xh + (1 + t / r) g_x - (t / r) d xh) / 2;
    gv = J g, glb = g - J g, gub = 0).  The case is admm_cone_ref.proj_cone's.
  * ``proj_cone_t`` / ``project_t``: the projection restated in torch on the
    case admm_cone_ref takes, so that autograd can differentiate it.
  * ``admm_step`` / ``admm_solve``: one iteration of csrc/admm.hip's header
    with that projection on adjoint_rows_ref's dense x-update, and its fixed
    point from a zero start.
  * ``ConeRecursion``: the recursion of DESIGN.md 5.11 for ONE problem at a
    fixed point, on the same dense x-update, and the final gradients.
  * the cone problems: ``cone_problem`` (one cone |u_k| <= r per stage k < N)
    and ``ragged_problem`` (box rows, a stage without rows, a cone between box
    rows, a terminal-stage cone), and ``cone_case``: a problem solved tightly
    with its reference gradients.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import adjoint_ref
import adjoint_rows_ref as rr
import admm_cone_ref as acr

F64 = torch.float64
KEYS = rr.BOX_KEYS  # E, c, H, h, x0, D, lb, ub
RHO, SIGMA, ALPHA = 10.0, 1e-6, 1.6


# ---- the operator -------------------------------------------------------------

def cone_vjp(p, g):
    """(J g, case) at p = (t, x): J the Jacobian of admm_cone_ref.proj_cone (symmetric)."""
    p, g = np.asarray(p, dtype=np.float64), np.asarray(g, dtype=np.float64)
    t, nx = float(p[0]), acr.cone_norm(p[1:])
    if nx <= t:
        return g.copy(), 0
    if nx <= -t:
        return np.zeros_like(g), 1
    xh, tr = p[1:] / nx, t / nx
    d = 0.0
    for a, b in zip(xh, g[1:]):
        d = d + float(a) * float(b)
    out = np.empty_like(g)
    out[0] = (g[0] + d) / 2.0
    out[1:] = ((g[0] * xh + (1.0 + tr) * g[1:]) - (tr * d) * xh) / 2.0
    return out, 2


def project_vjp(v, lb, ub, gout, ncs, cones):
    """(gv, glb, gub, cases) of one problem's rows [ny]."""
    gv = np.where((lb < v) & (v < ub), gout, 0.0)
    glb = np.where(v <= lb, gout, 0.0)
    gub = np.where(v >= ub, gout, 0.0)
    cases = []
    for (q, d) in acr.cone_rows(ncs, cones):
        jg, case = cone_vjp(v[q:q + d] - lb[q:q + d], gout[q:q + d])
        gv[q:q + d] = jg
        glb[q:q + d] = gout[q:q + d] - jg
        gub[q:q + d] = 0.0
        cases.append(case)
    return gv, glb, gub, cases


def proj_cone_t(p):
    """admm_cone_ref.proj_cone in torch, on the case it takes for p's values."""
    _, case = acr.proj_cone(p.detach().numpy())
    if case == 0:
        return p * 1.0
    if case == 1:
        return p * 0.0
    nx = p[1:].square().sum().sqrt()
    a = (1.0 + p[0] / nx) / 2.0
    return torch.cat([(a * nx).reshape(1), a * p[1:]])


def project_t(v, lb, ub, ncs, cones):
    """admm_cone_ref.project in torch (differentiable in v, lb, ub)."""
    out = torch.minimum(torch.maximum(v, lb), ub)
    parts, at = [], 0
    for (q, d) in acr.cone_rows(ncs, cones):
        parts += [out[at:q], lb[q:q + d] + proj_cone_t(v[q:q + d] - lb[q:q + d])]
        at = q + d
    parts.append(out[at:])
    return torch.cat(parts)


# ---- the ADMM step and its fixed point ------------------------------------------

def admm_step(E, c, H, h, x0, D, lb, ub, w, y, z, rho, sigma, alpha, dims, cones):
    """adjoint_rows_ref.admm_step with the projection onto the mixed set."""
    n, m, N, ncs = dims
    Df = rr.dense_D(D, n, m, N, ncs)
    wt = rr.x_update(E, c, H, h, x0, Df, rho, z - y / rho, w, sigma)
    vrel = alpha * (Df @ wt) + (1.0 - alpha) * z
    wn = alpha * wt + (1.0 - alpha) * w
    zn = project_t(vrel + y / rho, lb, ub, ncs, cones)
    yn = y + rho * (vrel - zn)
    return wn, yn, zn


def admm_solve(p, dims, cones, rho=RHO, sigma=SIGMA, alpha=ALPHA, tol=1e-13, max_iter=20000, eps_abs=None,
               check_every=25):
    """The fixed point (w, y, z) of admm_step from a zero start (numpy) and the
    iterations taken: until the max-norm change of the iterate is <= tol, or,
    with ``eps_abs``, by pdplqr_admm_solve's test with eps_rel = 0 every
    ``check_every`` iterations (adjoint_rows_ref.admm_solve's rules)."""
    n, m, N, ncs = dims
    t = lambda a: torch.tensor(a, dtype=F64)  # noqa: E731
    with torch.no_grad():
        Df = rr.dense_D(t(p["D"]), n, m, N, ncs)
        ny, nw = Df.shape
        rho_t = torch.full((ny,), rho, dtype=F64)
        args = [t(p[k]) for k in ("E", "c", "H", "h", "x0")]
        Kp, _, _ = rr.penalised_system(*args, Df, rho_t, torch.zeros(ny, dtype=F64), torch.zeros(nw, dtype=F64), sigma)
        Ki = torch.linalg.inv(Kp).numpy()
        _, r0, _ = rr.kkt_system(*args)
        r0, Df = r0.numpy(), Df.numpy()
    lb, ub = p["lb"], p["ub"]
    w, y, z = np.zeros(nw), np.zeros(ny), np.zeros(ny)
    for it in range(1, max_iter + 1):
        r = r0.copy()
        r[:nw] += sigma * w + Df.T @ (rho * (z - y / rho))
        wt = (Ki @ r)[:nw]
        vrel = alpha * (Df @ wt) + (1.0 - alpha) * z
        wn = alpha * wt + (1.0 - alpha) * w
        zn, _ = acr.project(vrel + y / rho, lb, ub, ncs, cones)
        yn = y + rho * (vrel - zn)
        if eps_abs is None:
            stop = max(np.abs(wn - w).max(), np.abs(yn - y).max(), np.abs(zn - z).max()) <= tol
        else:
            stop = (it % check_every == 0 and np.abs(Df @ wn - zn).max() <= eps_abs
                    and np.abs(Df.T @ (rho * (zn - z))).max() <= eps_abs)
        w, y, z = wn, yn, zn
        if stop:
            break
    return w, y, z, it


# ---- the recursion ----------------------------------------------------------------

class ConeRecursion:
    """DESIGN.md 5.11's recursion for ONE problem at the fixed point (w, y, z):
    BoxLQRLayer.backward's statements with the mask replaced by the operator."""

    def __init__(self, p, dims, cones, w, y, z, rho=RHO, sigma=SIGMA, alpha=ALPHA):
        self.p, self.dims, self.cones = p, dims, cones
        self.w, self.y, self.z = w, y, z
        self.sigma, self.alpha = sigma, alpha
        n, m, N, ncs = dims
        t = lambda a: torch.tensor(a, dtype=F64)  # noqa: E731
        self.rho = np.full(y.shape, rho)
        with torch.no_grad():
            Df = rr.dense_D(t(p["D"]), n, m, N, ncs)
            Kp, _, self.nw = rr.penalised_system(*[t(p[k]) for k in ("E", "c", "H", "h", "x0")], Df, t(self.rho),
                                                 t(0 * y), t(0 * w), sigma)
            self.Ki = torch.linalg.inv(Kp).numpy()[:self.nw, :self.nw]
            self.Df = Df.numpy()
        self.tt = z + y / self.rho

    def jt(self, q):
        """(J^T q, glb, gub) at tt."""
        return project_vjp(self.tt, self.p["lb"], self.p["ub"], q, self.dims[3], self.cones)[:3]

    def margin(self):
        """The least | |x| - t | of the cones at tt (inf without cones)."""
        out = np.inf
        for (q, d) in acr.cone_rows(self.dims[3], self.cones):
            pp = self.tt[q:q + d] - self.p["lb"][q:q + d]
            out = min(out, abs(acr.cone_norm(pp[1:]) - float(pp[0])))
        return out

    def cases(self):
        return [acr.proj_cone(self.tt[q:q + d] - self.p["lb"][q:q + d])[1]
                for (q, d) in acr.cone_rows(self.dims[3], self.cones)]

    def cotangents(self, gws, a):
        b_w = gws + a[0]
        q = a[2] - self.rho * a[1]
        jq, glb, gub = self.jt(q)
        return b_w, q, jq, self.rho * a[1] + jq, glb, gub

    def apply(self, gws, a):
        """One iteration: a <- dl/ds + J_step^T a."""
        al, sg = self.alpha, self.sigma
        b_w, q, jq, b_vr, _, _ = self.cotangents(gws, a)
        gh = -self.Ki @ (al * b_w + self.Df.T @ (al * b_vr))
        gg = -self.rho * (self.Df @ gh)
        return ((1.0 - al) * b_w - sg * gh, a[1] + jq / self.rho - gg / self.rho, (1.0 - al) * b_vr + gg)

    def solve(self, gws, tol, max_iter, check_every=1):
        """(a, iterations, converged): frozen at the first test it passes."""
        a = (np.zeros_like(self.w), np.zeros_like(self.y), np.zeros_like(self.y))
        for it in range(1, max_iter + 1):
            an = self.apply(gws, a)
            ch = max(np.abs(x - y).max() for x, y in zip(an, a))
            a = an
            if (it % check_every == 0 or it == max_iter) and ch <= tol * max(np.abs(x).max() for x in a):
                return a, it, True
        return a, max_iter, False

    def gradients(self, gws, a):
        """The final pass: the eight gradients at the cotangents of a (autograd
        through the dense x-update with gws := alpha b_w, gvs := alpha b_vr)."""
        n, m, N, ncs = self.dims
        al = self.alpha
        b_w, q, jq, b_vr, glb, gub = self.cotangents(gws, a)
        t = lambda x, rg=False: torch.tensor(x, dtype=F64, requires_grad=rg)  # noqa: E731
        lv = [t(self.p[k], True) for k in KEYS[:6]]
        Df = rr.dense_D(lv[5], n, m, N, ncs)
        wt = rr.x_update(*lv[:5], Df, t(self.rho), t(self.z - self.y / self.rho), t(self.w), self.sigma)
        loss = (t(al * b_w) * wt).sum() + (t(al * b_vr) * (Df @ wt)).sum()
        grads = [g.numpy() for g in torch.autograd.grad(loss, lv)]
        return dict(zip(KEYS, grads + [glb, gub]))


# ---- the problems -------------------------------------------------------------------

def layout_problem(n, m, N, seed, layout):
    """adjoint_ref.random_problem(n, m, N, 1, seed) with the rows of `layout`
    (admm_cone_ref.build_problem's groups): (p, dims, cones)."""
    E, c, H, h, x0, g = adjoint_ref.random_problem(n, m, N, 1, seed)
    s = n + m
    ncs, cones, Ds, lbs, ubs = [], [], [], [], []
    for k, groups in enumerate(layout):
        dim = s if k < N else n
        rows = []
        for (kind, cols, val) in groups:
            cols = list(cols)
            if kind == "ball":
                cones.append((k, len(rows), len(cols) + 1))
                rows.append(np.zeros(dim))
                lbs.append(-val)
                ubs.append(-val)
            for col in cols:
                e = np.zeros(dim)
                e[col] = 1.0
                rows.append(e)
                lbs.append(-val if kind == "box" else 0.0)
                ubs.append(val if kind == "box" else 0.0)
        ncs.append(len(rows))
        if rows:
            Ds.append(np.array(rows).reshape(len(rows), dim).reshape(-1, order="F"))
    p = dict(E=E[0], c=c[0], H=H[0], h=h[0], x0=x0[0], D=np.concatenate(Ds), lb=np.array(lbs), ub=np.array(ubs),
             gws=g[0])
    return p, (n, m, N, tuple(ncs)), cones


def cone_problem(n, m, N, seed, radius):
    """nc = m + 1 rows per stage k < N, D_k = [0; I_m 0], lb = ub = (-r, 0, ..):
    one cone |u_k| <= r per stage, none at the terminal."""
    return layout_problem(n, m, N, seed, [[("ball", range(m), radius)] for _ in range(N)] + [[]])


RAGGED = (6, 3, 5, 2)  # n, m, N, seed


def ragged_layout(n=6, m=3, N=5):
    """6/3, N = 5: a cone |u_0| <= 0.8; a stage with no rows; a box row, a cone
    over (u_1, u_2), a box row on a state; box rows on every input; a cone
    again; a terminal cone |x_N| <= 2.5 of width n + 1."""
    return [[("ball", range(m), 0.8)], [], [("box", (0,), 0.4), ("ball", (1, 2), 0.5), ("box", (m,), 1.5)],
            [("box", range(m), 0.4)], [("ball", range(m), 0.8)], [("ball", range(n), 2.5)]]


def ragged_problem():
    n, m, N, seed = RAGGED
    return layout_problem(n, m, N, seed, ragged_layout(n, m, N))


# (n, m, N, seed, radius): the cone problems of the tests; radius None is the ragged one
CONE_PROBLEMS = [(4, 2, 6, 0, 0.3), (4, 2, 6, 0, 0.7), (6, 3, 5, 2, 0.8), (4, 2, 6, 1, 1.2), RAGGED + (None,)]
# the batch of tests/test_gpu_cone_adjoint.py at (4, 2, 6)
GPU_BATCH = [(4, 2, 6, 0, 0.3), (4, 2, 6, 0, 0.7), (4, 2, 6, 1, 1.2)]
# ConeLQRLayer's settings in tests/test_gpu_cone_adjoint.py
LAYER = dict(eps_abs=1e-9, max_iter=4000, adj_tol=1e-10, adj_max_iter=4000, check_every=25)


def problem(key):
    n, m, N, seed, radius = key
    return ragged_problem() if radius is None else cone_problem(n, m, N, seed, radius)


@functools.lru_cache(maxsize=None)
def cone_case(key, layer=False):
    """The problem `key` of CONE_PROBLEMS solved to its fixed point and
    differentiated by the recursion (computed once per session; callers must
    not modify the arrays).  layer = False: the tight run (iterate change <=
    1e-13, adjoint tol 1e-12); True: LAYER's stopping rules."""
    p, dims, cones = problem(key)
    if layer:
        w, y, z, iters = admm_solve(p, dims, cones, eps_abs=LAYER["eps_abs"], max_iter=LAYER["max_iter"],
                                    check_every=LAYER["check_every"])
    else:
        w, y, z, iters = admm_solve(p, dims, cones)
    rec = ConeRecursion(p, dims, cones, w, y, z)
    if layer:
        a, adj_iters, conv = rec.solve(p["gws"], LAYER["adj_tol"], LAYER["adj_max_iter"], LAYER["check_every"])
    else:
        a, adj_iters, conv = rec.solve(p["gws"], 1e-12, 20000)
    return dict(p=p, dims=dims, cones=cones, w=w, y=y, z=z, iters=iters, rec=rec, a=a, adj_iters=adj_iters,
                adj_converged=conv, grads=rec.gradients(p["gws"], a), margin=rec.margin(), cases=rec.cases())


def grad_err(got, ref):
    """Frobenius error of a gradient array against its reference, relative to
    max(|ref|, 0.1).  The floor: an array that is identically zero in exact
    arithmetic (grad D and grad lb of a problem whose cones are all inactive,
    grad ub on cone rows) has no relative error, and one far below the unit
    scale of the problem data carries the absolute error of the O(1 .. 10)
    arrays it is computed with; those are held to an absolute error at a tenth
    of the data's unit scale."""
    got, ref = np.asarray(got).ravel(), np.asarray(ref).ravel()
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 0.1))


# The worst gradient error tests/test_cone_adjoint_cpu.py::test_recursion_at_layer_settings
# measures on the CPU at LAYER's stopping rules against the tight run, per shape
# (checked there within a factor 2; tests/test_gpu_cone_adjoint.py allows 10 times this)
CONE_LAYER_CPU_ERR = {(4, 2, 6): 8.3e-9, (6, 3, 5): 5.0e-10}
