"""CPU restatement of the ADMM loop with second-order cone rows (csrc/admm.hip,
csrc/kernels_cone.hip; DESIGN.md section 5.5 "Second-order cones").

It is ``oracle.oracle.admm_solve``'s loop -- the same x-update protocol on the
oracle's solvers, the same termination test, the same adaptive-rho rule -- with
the clamp replaced by the projection onto the mixed set: rows in no cone clamp
to [lb, ub]; the rows of a cone, with p = v - lb = (t, x), give lb + P_K(p),

    |x| <= t   ->  p
    |x| <= -t  ->  0
    otherwise  ->  a = (1 + t / |x|) / 2,  (a |x|, a x)

evaluated in that order, |x| the square root of the squares summed in row
order.  A cone counts as an active row of the adaptive rule when its
projection's argument had |x| >= t.

TEST INFRASTRUCTURE: also the problem constructions the CPU and GPU tests share.
"""
import math

import numpy as np

from oracle.oracle import OracleParallel, OracleSerial


def cone_norm(x):
    """sqrt of the squares summed in order (the kernels' |x|)."""
    ss = 0.0
    for e in x:
        ss = ss + float(e) * float(e)
    return math.sqrt(ss)


def proj_cone(p):
    """(P_K(p), case) for p = (t, x): case 0 kept, 1 zero, 2 the boundary point."""
    p = np.asarray(p, dtype=np.float64)
    t = float(p[0])
    nx = cone_norm(p[1:])
    if nx <= t:
        return p.copy(), 0
    if nx <= -t:
        return np.zeros_like(p), 1
    a = (1.0 + t / nx) / 2.0
    out = a * p
    out[0] = a * nx
    return out, 2


def stage_offsets(ncs):
    return np.concatenate([[0], np.cumsum(np.asarray(ncs, dtype=np.int64))]).astype(int)


def cone_rows(ncs, cones):
    """[(first row within the problem's ny rows, dim)] of every cone."""
    yo = stage_offsets(ncs)
    return [(int(yo[k] + r), int(d)) for (k, r, d) in cones]


def project(v, lb, ub, ncs, cones):
    """The projection of one problem's v [ny] onto the mixed set; also the list
    of (case, |x| >= t) per cone."""
    out = np.minimum(np.maximum(v, lb), ub)
    info = []
    for (q, d) in cone_rows(ncs, cones):
        p = v[q:q + d] - lb[q:q + d]
        pk, case = proj_cone(p)
        out[q:q + d] = lb[q:q + d] + pk
        info.append((case, cone_norm(p[1:]) >= float(p[0])))
    return out, info


def in_set_violation(z, lb, ub, ncs, cones):
    """How far z is outside the mixed set (0 inside): box violation, |x| - t on cones."""
    box = np.ones(z.size, dtype=bool)
    viol = 0.0
    for (q, d) in cone_rows(ncs, cones):
        box[q:q + d] = False
        p = z[q:q + d] - lb[q:q + d]
        viol = max(viol, cone_norm(p[1:]) - float(p[0]))
    if box.any():
        viol = max(viol, float(np.max(np.maximum(lb - z, z - ub)[box])))
    return max(viol, 0.0)


def admm_cone_solve(pm, x0, lb, ub, rho, cones, ws=None, ys=None, zs=None, solver="serial", sigma=1e-6, alpha=1.6,
                    max_iter=4000, check_every=25, eps_abs=1e-3, eps_rel=1e-3, adaptive_rho=True,
                    adaptive_rho_tolerance=5.0, **solver_kw):
    """One problem.  Returns (w, y, z, info); info adds to oracle.admm_solve's
    keys `cone_case` (the case of every cone at the last z-update), `margin`
    (over all termination tests, the least relative distance of the residuals
    from the thresholds that would have changed the test's outcome) and
    `est_margin` (the least relative distance of an adaptive-rho estimate e from
    the rule's limits tol and 1 / tol)."""
    n, m, N = pm.n, pm.m, pm.N
    s = n + m
    ncs = [int(x) for x in pm.ncs]
    ny = sum(ncs)
    w = np.zeros(N * s + n) if ws is None else np.array(ws, dtype=np.float64)
    y = np.zeros(ny) if ys is None else np.array(ys, dtype=np.float64)
    z = np.zeros(ny) if zs is None else np.array(zs, dtype=np.float64)
    lb = np.asarray(lb, dtype=np.float64)
    ub = np.asarray(ub, dtype=np.float64)
    rho = np.array(rho, dtype=np.float64)
    irho = 1.0 / rho
    solv = {"serial": OracleSerial, "parallel": OracleParallel}[solver](pm, **solver_kw)
    blocks = []
    doff = yoff = 0
    for k in range(N + 1):
        nc, dim = ncs[k], (s if k < N else n)
        Dk = pm.D[doff:doff + nc * dim].reshape(nc, dim, order="F") if nc else np.zeros((0, dim))
        blocks.append((k * s, dim, yoff, nc, Dk))
        doff += nc * dim
        yoff += nc
    it = 0
    conv = False
    rp = rd = 0.0
    refactor = True
    rho_updates = 0
    cone_case, margin, est_margin = [], None, np.inf
    for it in range(1, max_iter + 1):
        solv.update_problem_data(w, y, z, irho, sigma)
        if refactor:
            solv.backward(rho)
            refactor = False
        else:
            solv.backward_without_factorization(rho)
        wt = solv.forward(x0)
        check = it == max_iter or it % check_every == 0
        wn = alpha * wt + (1.0 - alpha) * w
        v = np.concatenate([Dk @ wt[wo:wo + dim] for (wo, dim, yo, nc, Dk) in blocks if nc])
        vrel = alpha * v + (1.0 - alpha) * z
        zn, cinfo = project(vrel + irho * y, lb, ub, ncs, cones)
        yn = y + rho * (vrel - zn)
        cone_case = [c for (c, _) in cinfo]
        if check:
            rp = dwm = zm = rd = dty = 0.0
            inbox = np.ones(ny, dtype=bool)
            for (q, d) in cone_rows(ncs, cones):
                inbox[q:q + d] = False
            act = bool(np.any(((zn <= lb) | (zn >= ub)) & inbox)) or any(a for (_, a) in cinfo)
            for (wo, dim, yo, nc, Dk) in blocks:
                if nc == 0:
                    continue
                sl = slice(yo, yo + nc)
                dwn = alpha * v[sl] + (1.0 - alpha) * (Dk @ w[wo:wo + dim])
                rp = max(rp, float(np.max(np.abs(dwn - zn[sl]))))
                dwm = max(dwm, float(np.max(np.abs(dwn))))
                zm = max(zm, float(np.max(np.abs(zn[sl]))))
                rd = max(rd, float(np.max(np.abs(Dk.T @ (rho[sl] * (zn[sl] - z[sl]))))))
                dty = max(dty, float(np.max(np.abs(Dk.T @ yn[sl]))))
        w, y, z = wn, yn, zn
        if check:
            tp, td = eps_abs + eps_rel * max(dwm, zm), eps_abs + eps_rel * dty
            if tp > 0 and td > 0:
                # how far this test was from the other outcome: passed -- the closer residual;
                # failed -- the farther of the residuals that failed
                fl = min(1.0 - rp / tp, 1.0 - rd / td) if (rp <= tp and rd <= td) else \
                    max(rp / tp - 1.0, rd / td - 1.0)
                margin = fl if margin is None else min(margin, fl)
            if rp <= tp and rd <= td:
                conv = True
                break
            if adaptive_rho and it < max_iter and act and dty > 1e-30:
                e = np.sqrt((rp / (max(dwm, zm) + 1e-30)) / (rd / (dty + 1e-30) + 1e-30))
                tol = adaptive_rho_tolerance
                est_margin = min(est_margin, abs(e / tol - 1.0), abs(e * tol - 1.0))
                if e > adaptive_rho_tolerance or e < 1.0 / adaptive_rho_tolerance:
                    rho = np.minimum(np.maximum(rho * e, 1e-6), 1e6)
                    irho = 1.0 / rho
                    refactor = True
                    rho_updates += 1
    return w, y, z, {"iters": it, "converged": conv, "prim_res": rp, "dual_res": rd, "rho": rho,
                     "rho_updates": rho_updates, "cone_case": cone_case, "margin": margin,
                     "est_margin": est_margin}


# ---------------------------------------------------------------------------
# problem constructions shared by the CPU and GPU tests
# ---------------------------------------------------------------------------
def build_problem(n, m, N, layout, seed):
    """(pm, x0, lb, ub, cones) from a per-stage list of row groups (N + 1 entries,
    each a list of groups, in row order):
        ("box", cols, bound)   one row e_c per column c, |w_c| <= bound
        ("ball", cols, r)      the cone |w_cols| <= r: rows [0; e_c ...], lb = (-r, 0, ..)
    Columns index the stage's w_k = (u_k, x_k) (the terminal stage: x_N).  ub of
    a cone row is lb (not read)."""
    from admm_infeas_ref import random_packed

    s = n + m
    ncs, cones, Ds, lbs, ubs = [], [], [], [], []
    for k, groups in enumerate(layout):
        dim = s if k < N else n
        rows, lo, hi = [], [], []
        for (kind, cols, val) in groups:
            cols = list(cols)
            if kind == "box":
                for c in cols:
                    e = np.zeros(dim)
                    e[c] = 1.0
                    rows.append(e)
                    lo.append(-val)
                    hi.append(val)
            else:
                cones.append((k, len(rows), len(cols) + 1))
                rows.append(np.zeros(dim))
                lo.append(-val)
                hi.append(-val)
                for c in cols:
                    e = np.zeros(dim)
                    e[c] = 1.0
                    rows.append(e)
                    lo.append(0.0)
                    hi.append(0.0)
        ncs.append(len(rows))
        if rows:
            Ds.append(np.array(rows).reshape(len(rows), dim).reshape(-1, order="F"))
        lbs += lo
        ubs += hi
    pm = random_packed(n, m, N, ncs, seed)
    pm.D = np.concatenate(Ds) if Ds else np.zeros(0)
    x0 = np.random.default_rng(seed + 7919).standard_normal(n)
    return pm, x0, np.array(lbs), np.array(ubs), cones


def build_batch(n, m, N, layout, seeds, warm_seed=None):
    """The problems of `seeds` stacked into the boundary's batch-major arrays:
    a dict with pms, x0, lb, ub, cones, ncs, the model arrays E c H h D and the
    warm start ws, ys, zs (0.1 N(0, 1) from `warm_seed`, zeros when None)."""
    ps = [build_problem(n, m, N, layout, sd) for sd in seeds]
    out = {"pms": [p[0] for p in ps], "cones": ps[0][4], "ncs": [int(x) for x in ps[0][0].ncs]}
    for k in "E c H h D".split():
        out[k] = np.ascontiguousarray(np.stack([getattr(p[0], k) for p in ps]))
    out["x0"] = np.ascontiguousarray(np.stack([p[1] for p in ps]))
    out["lb"] = np.ascontiguousarray(np.stack([p[2] for p in ps]))
    out["ub"] = np.ascontiguousarray(np.stack([p[3] for p in ps]))
    B, W, Y = len(ps), out["h"].shape[1], out["lb"].shape[1]
    if warm_seed is None:
        out["ws"], out["ys"], out["zs"] = np.zeros((B, W)), np.zeros((B, Y)), np.zeros((B, Y))
    else:
        g = np.random.default_rng(warm_seed)
        out["ws"], out["ys"], out["zs"] = (0.1 * g.standard_normal((B, W)), 0.1 * g.standard_normal((B, Y)),
                                           0.1 * g.standard_normal((B, Y)))
    return out


def standard_layout(n, m, N, ubox=0.2, ucone=0.3, xcone=1.0):
    """Two box rows on u (|u_i| <= ubox), a cone |u_k| <= ucone at every stage
    and a terminal cone |x_N| <= xcone."""
    return [[("box", (0, 1), ubox), ("ball", range(m), ucone)] for _ in range(N)] + [[("ball", range(n), xcone)]]


def ragged_layout(n=6, m=3, N=7):
    """6/3: a stage with no rows; one with box rows, a cone, box rows, a second
    cone; a cone of dimension s + 1 over the whole w_k (its first D row is
    zero); box-only stages; a terminal cone of width n + 1."""
    s = n + m
    lay = [[("box", (0, 1), 0.2), ("ball", range(m), 0.3)] for _ in range(N)] + [[("ball", range(n), 1.0)]]
    lay[1] = []
    lay[2] = [("box", (0,), 0.2), ("ball", (0, 1), 0.25), ("box", (1, 2), 0.2), ("ball", range(m), 0.3)]
    lay[3] = [("ball", range(s), 2.5)]
    lay[4] = [("box", range(m), 0.2)]
    return lay
