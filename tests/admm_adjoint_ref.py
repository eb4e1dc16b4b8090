"""Dense restatement of pdplqr_admm_adjoint for ONE problem (CPU, torch
float64) and its autograd reference.

``restate`` runs the four steps of include/pdplqr.h on dense matrices: the
polishing x-update at (w, y), g~ = gws + D^T gvs, refine_iter + 1 adjoint
solves with the matrix of the polishing system, and the gradients -- gE, gc,
gx from the dense multipliers of the dynamics.  ``reference`` is autograd
through ``adjoint_rows_ref.active_set_solution`` (the KKT solve with the active
rows as equalities, no regularisation) and nothing else.  ``problem`` collects
the cases of tests/test_admm_adjoint_cpu.py and tests/test_gpu_admm_adjoint.py:
the u-box problems of ``adjoint_rows_ref.box_case`` and one ragged problem with
dense rows.  Nothing here comes from the product or the oracle.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import adjoint_ref
import adjoint_rows_ref as rr

F64 = torch.float64
KEYS = rr.BOX_KEYS
INF = 1e20


def _t(a):
    return torch.tensor(np.asarray(a), dtype=F64)


def restate(p, dims, at_lb, at_ub, w, y, gws, gvs=None, delta=1e-6, refine_iter=3):
    """The gradients of BOX_KEYS by the call's steps, the per-step max|D_a v|
    and max|v|, and w~.  ``p``: numpy arrays of BOX_KEYS; (w, y): the returned
    point; the active set and the side of every row are given."""
    n, m, N, ncs = dims
    s = n + m
    with torch.no_grad():
        K, r, nw = rr.kkt_system(*[_t(p[k]) for k in ("E", "c", "H", "h", "x0")])
        Df = rr.dense_D(_t(p["D"]), n, m, N, ncs)
        act = _t((at_lb | at_ub).astype(float))
        bt = _t(np.where(at_lb, p["lb"], np.where(at_ub, p["ub"], 0.0)))
        Da = act[:, None] * Df
        Kp = K.clone()
        Kp[:nw, :nw] += delta * torch.eye(nw, dtype=F64) + Da.t() @ Da / delta
        # 1. the polishing x-update at (w, y): -h~ = -h + delta w + D_a^T b / delta - D_a^T y
        rp = r.clone()
        rp[:nw] += delta * _t(w) + Da.t() @ (bt / delta - _t(y))
        z = torch.linalg.solve(Kp, rp)
        wt, lam = z[:nw], z[nw:]
        # 2., 3.
        gt = _t(gws) + (Df.t() @ _t(gvs) if gvs is not None else 0.0)
        v, eta, mu = torch.zeros(nw, dtype=F64), torch.zeros(Df.shape[0], dtype=F64), None
        steps = []
        for _ in range(refine_iter + 1):
            rhs = torch.zeros_like(r)
            rhs[:nw] = -(gt - delta * v + Da.t() @ eta)
            z = torch.linalg.solve(Kp, rhs)
            v, mu = z[:nw], z[nw:]
            eta = eta + act * (Df @ v) / delta
            steps.append((float((Da @ v).abs().max()), float(v.abs().max())))
        # 4. dl = [v; mu; eta]^T (dK z - dr) on the KKT system of the active set
        ya = act * _t(y)
        g = {"h": v.clone(), "x0": -mu[:n].clone(), "c": -mu[n:].clone()}
        gH, gE = torch.zeros_like(_t(p["H"])), torch.zeros_like(_t(p["E"]))
        for k in range(N + 1):
            d = s if k < N else n
            vk, wk = v[k * s:k * s + d], wt[k * s:k * s + d]
            gH[k * s * s:k * s * s + d * d] = (0.5 * (torch.outer(vk, wk) + torch.outer(wk, vk))).t().reshape(-1)
            if k < N:
                mk, lk = mu[(k + 1) * n:(k + 2) * n], lam[(k + 1) * n:(k + 2) * n]
                gE[k * n * s:(k + 1) * n * s] = (-torch.outer(mk, wk) - torch.outer(lk, vk)).t().reshape(-1)
        g["H"], g["E"] = gH, gE
        d_off, y_off = rr.offsets(n, m, N, ncs)
        gD = torch.zeros_like(_t(p["D"]))
        e2 = eta + (_t(gvs) if gvs is not None else 0.0)
        for k in range(N + 1):
            d = s if k < N else n
            ys = slice(y_off[k], y_off[k + 1])
            blk = torch.outer(ya[ys], v[k * s:k * s + d]) + torch.outer(e2[ys], wt[k * s:k * s + d])
            gD[d_off[k]:d_off[k + 1]] = blk.t().reshape(-1)
        g["D"] = gD
        g["lb"] = torch.where(torch.tensor(at_lb), -eta, torch.zeros_like(eta))
        g["ub"] = torch.where(torch.tensor(at_ub), -eta, torch.zeros_like(eta))
    return {k: g[k].numpy() for k in KEYS}, steps, wt.numpy()


def reference(p, dims, at_lb, at_ub, gws, gvs=None):
    """(ws, gradients of BOX_KEYS) of sum(gws * ws) + sum(gvs * (D ws)) by
    autograd through the active-set KKT solve."""
    n, m, N, ncs = dims
    t = {k: torch.tensor(p[k], dtype=F64, requires_grad=True) for k in KEYS}
    ws = rr.active_set_solution(*[t[k] for k in KEYS], at_lb, at_ub, dims)
    loss = (_t(gws) * ws).sum()
    if gvs is not None:
        loss = loss + (_t(gvs) * (rr.dense_D(t["D"], n, m, N, ncs) @ ws)).sum()
    grads = torch.autograd.grad(loss, [t[k] for k in KEYS])
    return ws.detach().numpy(), {k: gr.numpy() for k, gr in zip(KEYS, grads)}


def cpu_bound(pr, delta=1e-6):
    """The error bound of the restatement against the reference for one case,
    from the matrices alone.  Both sides are dense LU solves.  The reference's
    matrix is the KKT matrix K_a of the active set: relative error up to eps
    cond(K_a), times 100 for the sums that form the gradients.  The
    restatement solves with the penalised matrix K_p = K + delta I + D_a^T D_a /
    delta, whose backward error eps |K_p| acts on the solution through K_a^-1.
    On the u-box rows D_a^T D_a / delta is diagonal and an input it penalises is
    eliminated by an exact scaling, so that error stays in the penalised
    directions, which D_a v = 0 removes: the first term alone.  Dense rows
    spread it over the stage: 10 eps |K_p| |K_a^-1| there."""
    n, m, N, ncs = pr["dims"]
    t = [_t(pr[k]) for k in KEYS]
    K, _, nw = rr.kkt_system(*t[:5])
    Df = rr.dense_D(t[5], n, m, N, ncs)
    A = Df[torch.tensor(np.flatnonzero(pr["at_lb"] | pr["at_ub"]), dtype=torch.long)]
    dim, na = K.shape[0], A.shape[0]
    Ka = torch.zeros(dim + na, dim + na, dtype=F64)
    Ka[:dim, :dim] = K
    Ka[dim:, :nw] = A
    Ka[:nw, dim:] = A.t()
    sv = torch.linalg.svdvals(Ka)
    eps = float(np.finfo(float).eps)
    bound = 100.0 * eps * float(sv[0] / sv[-1])
    ubox = bool(((Df != 0).sum(dim=1) == 1).all())
    if not ubox:
        Kp = K.clone()
        Kp[:nw, :nw] += delta * torch.eye(nw, dtype=F64) + A.t() @ A / delta
        bound = max(bound, 10.0 * eps * float(torch.linalg.svdvals(Kp)[0]) / float(sv[-1]))
    return bound


def relmax(a, b):
    """Max-norm error of a against b relative to b's max-norm."""
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)) if b.size else 0.0


# ---- the ragged problem ----------------------------------------------------------

RAGGED_DIMS = (4, 2, 5, (2, 0, 3, 1, 2, 2))
# per row: "lo" / "up" pushed 0.3 past the unconstrained value (active on that
# side, the other bound infinite), "eq" lb == ub 0.2 away from it, "in" loose on
# both sides, "free" both bounds infinite.  At most m = 2 rows of a stage are
# active: the active rows of a stage stay independent on the inputs.
RAGGED_KINDS = ("up", "in",  "lo", "free", "up",  "eq",  "in", "lo",  "up", "in")


def ragged_problem(seed):
    """One (4, 2, 5) problem with ncs = (2, 0, 3, 1, 2, 2): dense standard-normal
    rows over states and inputs (the terminal's over the state), bounds placed
    around the rows' values at the unconstrained solution by RAGGED_KINDS."""
    n, m, N, ncs = RAGGED_DIMS
    E, c, H, h, x0, g = adjoint_ref.random_problem(n, m, N, 1, seed)
    rng = np.random.default_rng(seed + 177)
    d_off, y_off = rr.offsets(n, m, N, ncs)
    D = rng.standard_normal(d_off[-1])
    w0 = adjoint_ref.dense_kkt_solution(*[_t(a[0]) for a in (E, c, H, h, x0)])
    v0 = (rr.dense_D(_t(D), n, m, N, ncs) @ w0).numpy()
    lb, ub = np.full(y_off[-1], -INF), np.full(y_off[-1], INF)
    for i, kind in enumerate(RAGGED_KINDS):
        if kind == "up":
            ub[i] = v0[i] - 0.3
        elif kind == "lo":
            lb[i] = v0[i] + 0.3
        elif kind == "eq":
            lb[i] = ub[i] = v0[i] + 0.2
        elif kind == "in":
            lb[i], ub[i] = v0[i] - 2.0, v0[i] + 2.0
    return dict(E=E[0], c=c[0], H=H[0], h=h[0], x0=x0[0], D=D, lb=lb, ub=ub, gws=g[0]), RAGGED_DIMS


def _active_set(p, y, z):
    """(at_lb, at_ub, margin) from a fixed point: a row is active by the sign of
    its multiplier, an equality row always (lower); the margin is the least
    |y| over the active inequality rows and the least slack over the rest."""
    eq = p["lb"] == p["ub"]
    at_lb, at_ub = (y < -1e-9) | eq, (y > 1e-9) & ~eq
    act = at_lb | at_ub
    ineq = act & ~eq
    slack = np.minimum(z - p["lb"], p["ub"] - z)
    margin = min(np.abs(y[ineq]).min() if ineq.any() else np.inf, slack[~act].min() if (~act).any() else np.inf)
    return at_lb, at_ub, float(margin)


@functools.lru_cache(maxsize=None)
def problem(n, m, N, seed, ragged=False):
    """One case, computed once per session (callers must not modify the arrays):
    the arrays of BOX_KEYS, dims, gws, gvs, the fixed point (w, y, z) of the
    dense ADMM (rho = 10, sigma = 1e-6, alpha = 1.6, iterate change <= 1e-14), its
    active set and strict-complementarity margin."""
    if ragged:
        p, dims = ragged_problem(seed)
        assert dims[:3] == (n, m, N)
    else:
        p, dims = rr.box_problem(n, m, N, seed)
    ny = p["lb"].size
    t = [_t(p[k]) for k in KEYS]
    w, y, z, iters = rr.admm_solve(*t, torch.full((ny,), 10.0, dtype=F64), 1e-6, 1.6, dims)
    w, y, z = w.numpy(), y.numpy(), z.numpy()
    at_lb, at_ub, margin = _active_set(p, y, z)
    gvs = np.random.default_rng(seed + 991).standard_normal(ny)
    return dict(p, dims=dims, w=w, y=y, z=z, iters=iters, at_lb=at_lb, at_ub=at_ub, margin=margin, gvs=gvs,
                n_active=int((at_lb | at_ub).sum()))


@functools.lru_cache(maxsize=None)
def graded(n, m, N, seed, ragged=False, with_gvs=False, refine_iter=3):
    """problem() with the autograd reference, the restatement and the
    restatement's own error per array (max-norm, relative to the array's)."""
    pr = problem(n, m, N, seed, ragged)
    gvs = pr["gvs"] if with_gvs else None
    ws, ref = reference(pr, pr["dims"], pr["at_lb"], pr["at_ub"], pr["gws"], gvs)
    mine, steps, wt = restate(pr, pr["dims"], pr["at_lb"], pr["at_ub"], pr["w"], pr["y"], pr["gws"], gvs,
                              refine_iter=refine_iter)
    return dict(ws=ws, ref=ref, mine=mine, steps=steps, wt=wt, err={k: relmax(mine[k], ref[k]) for k in KEYS})


# (n, m, N, seeds, ragged): the cases of the issue; the GPU test takes one batch of three per line
CASES = [
    (3, 2, 6, (4, 5, 7), False),
    (12, 4, 4, (1, 2, 5), False),
    (3, 2, 18, (1, 4, 5), False),
    (24, 12, 3, (1, 5, 6), False),
    (4, 2, 5, None, True),  # seeds: RAGGED_SEEDS
]
# seeds of the ragged problem whose margin is >= 1e-2 (asserted in tests/test_admm_adjoint_cpu.py)
RAGGED_SEEDS = (2, 6, 7)
