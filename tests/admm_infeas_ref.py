"""numpy restatement of the ADMM infeasibility certificates (DESIGN.md section
5.5; OSQP: Stellato et al. 2020 section 3.4, Banjac et al. 2019) and of the
ADMM loop of csrc/admm.hip with both tests, dense throughout.

The x-update solves the dynamics exactly, so the certificates are OSQP's in the
coordinates of the dynamics' affine set:

* primal: dy certifies that {w : dynamics, lb <= D w <= ub} is empty.  One
  backward costate recursion gives the reduced gradient g = Z^T D^T dy over the
  inputs and beta = (D w_p)^T dy for the zero-input rollout w_p;
* dual: dw certifies a cost unbounded below; every term is stage-local.

Only the packed layouts of pdplqr.model.PackedModel are used (no oracle).
"""
import numpy as np

INF_BOUND = 1e20  # |bound| >= this counts as infinite (tests/test_gpu_admm.py clips to it)

# order of the 8 measures (include/pdplqr.h: pdplqr_admm_check_certificates)
M_DY, M_G, M_SUPPORT, M_INFFLAG, M_DW, M_HDW, M_HTDW, M_VIOL = range(8)


def stage_views(pm):
    """Per-stage (E_k, c_k, H_k, h_k, D_k) of a packed model; the terminal stage
    has E = c = None."""
    n, m, N = pm.n, pm.m, pm.N
    s = n + m
    out, doff = [], 0
    for k in range(N + 1):
        dim = s if k < N else n
        nc = int(pm.ncs[k])
        D = pm.D[doff:doff + nc * dim].reshape(nc, dim, order="F")
        doff += nc * dim
        if k < N:
            out.append((pm.E[k * n * s:(k + 1) * n * s].reshape(n, s, order="F"), pm.c[k * n:(k + 1) * n],
                        pm.H[k * s * s:(k + 1) * s * s].reshape(s, s, order="F"), pm.h[k * s:(k + 1) * s], D))
        else:
            out.append((None, None, pm.H[N * s * s:].reshape(n, n, order="F"), pm.h[N * s:], D))
    return out


def costate_recursion(pm, x0, dy):
    """(g, beta): g[k] = the input part of q_k + E_k^T nu_{k+1} (k < N), and
    beta = sum_k nu_{k+1}^T c_k + nu_0^T x0, with q_k = D_k^T dy_k, nu_N = q_N."""
    n, m, N = pm.n, pm.m, pm.N
    st = stage_views(pm)
    yo = np.concatenate([[0], np.cumsum(pm.ncs)]).astype(int)
    nu = st[N][4].T @ dy[yo[N]:yo[N + 1]] if pm.ncs[N] else np.zeros(n)
    g = np.zeros((N, m))
    beta = 0.0
    for k in range(N - 1, -1, -1):
        E, c, _, _, D = st[k]
        beta += nu @ c
        v = E.T @ nu
        if pm.ncs[k]:
            v = D.T @ dy[yo[k]:yo[k + 1]] + v
        g[k] = v[:m]
        nu = v[m:]
    beta += nu @ x0
    return g, beta


def certificate_measures(pm, x0, lb, ub, dy, dw, eps_prim_inf=1e-4, eps_dual_inf=1e-4):
    """The 8 measures and the verdict (bit 0 primal, bit 1 dual) for one problem.
    dy or dw None skips that half (its measures stay 0)."""
    n, m, N = pm.n, pm.m, pm.N
    s = n + m
    st = stage_views(pm)
    yo = np.concatenate([[0], np.cumsum(pm.ncs)]).astype(int)
    meas = np.zeros(8)
    verdict = 0
    if dy is not None:
        nrm = np.max(np.abs(dy)) if dy.size else 0.0
        g, beta = costate_recursion(pm, x0, dy)
        thr = eps_prim_inf * nrm
        ub_inf, lb_inf = ub >= INF_BOUND, lb <= -INF_BOUND
        flag = bool(np.any((dy > thr) & ub_inf) or np.any((dy < -thr) & lb_inf))
        sup = np.sum(np.where(ub_inf, 0.0, ub) * np.maximum(dy, 0.0)) + \
            np.sum(np.where(lb_inf, 0.0, lb) * np.minimum(dy, 0.0)) - beta
        gmax = np.max(np.abs(g)) if g.size else 0.0
        meas[M_DY], meas[M_G], meas[M_SUPPORT], meas[M_INFFLAG] = nrm, gmax, sup, float(flag)
        if eps_prim_inf > 0 and nrm > 0 and gmax <= thr and not flag and sup < -thr:
            verdict |= 1
    if dw is not None:
        nrm = np.max(np.abs(dw))
        hdw = htdw = viol = 0.0
        viol = np.max(np.abs(dw[m:s]))  # dx_0
        for k in range(N + 1):
            E, _, H, h, D = st[k]
            wk = dw[k * s:(k + 1) * s] if k < N else dw[N * s:]
            hdw = max(hdw, np.max(np.abs(H @ wk)))
            htdw += h @ wk
            if k < N:
                xn = dw[(k + 1) * s + m:(k + 2) * s] if k + 1 < N else dw[N * s:]
                viol = max(viol, np.max(np.abs(xn - E @ wk)))
            if pm.ncs[k]:
                v = D @ wk
                l, u = lb[yo[k]:yo[k + 1]], ub[yo[k]:yo[k + 1]]
                viol = max(viol, np.max(np.where(u < INF_BOUND, v, 0.0)), np.max(np.where(l > -INF_BOUND, -v, 0.0)))
        meas[M_DW], meas[M_HDW], meas[M_HTDW], meas[M_VIOL] = nrm, hdw, htdw, viol
        thr = eps_dual_inf * nrm
        if eps_dual_inf > 0 and nrm > 0 and hdw <= thr and htdw < -thr and viol <= thr:
            verdict |= 2
    return meas, verdict


def dense_problem(pm, x0):
    """(Hd, hd, Dd, Ad, bd): the problem over the stacked w with A w = b the
    dynamics (x_0 = x0, x_{k+1} - E_k w_k = c_k)."""
    n, m, N = pm.n, pm.m, pm.N
    s = n + m
    nw, ny = N * s + n, int(np.sum(pm.ncs))
    st = stage_views(pm)
    Hd, Dd, Ad, bd = np.zeros((nw, nw)), np.zeros((ny, nw)), np.zeros((n * (N + 1), nw)), np.zeros(n * (N + 1))
    Ad[:n, m:s] = np.eye(n)
    bd[:n] = x0
    r = 0
    for k in range(N + 1):
        E, c, H, _, D = st[k]
        o, dim = k * s, (s if k < N else n)
        Hd[o:o + dim, o:o + dim] = H
        Dd[r:r + D.shape[0], o:o + dim] = D
        r += D.shape[0]
        if k < N:
            xo = (k + 1) * s + m if k + 1 < N else N * s
            Ad[n * (k + 1):n * (k + 2), xo:xo + n] = np.eye(n)
            Ad[n * (k + 1):n * (k + 2), o:o + s] -= E
            bd[n * (k + 1):n * (k + 2)] = c
    return Hd, pm.h.copy(), Dd, Ad, bd


def admm_loop(pm, x0, lb, ub, rho, w=None, y=None, z=None, sigma=1e-6, alpha=1.6, max_iter=4000, check_every=25,
              eps_abs=1e-3, eps_rel=1e-3, detect=True, eps_prim_inf=1e-4, eps_dual_inf=1e-4):
    """The loop of csrc/admm.hip (fixed rho) with a dense KKT x-update and both
    certificates at every termination test.  Returns a dict: status (0 unsolved,
    1 solved, 2 primal infeasible, 3 dual infeasible), iters, w, y, z, dy, dw,
    and `history`: (iteration, measures) of every test that ran the certificates."""
    Hd, hd, Dd, Ad, bd = dense_problem(pm, x0)
    nw, ny, na = Hd.shape[0], Dd.shape[0], Ad.shape[0]
    w = np.zeros(nw) if w is None else w.copy()
    y = np.zeros(ny) if y is None else y.copy()
    z = np.zeros(ny) if z is None else z.copy()
    K = np.zeros((nw + na, nw + na))
    K[:nw, :nw] = Hd + sigma * np.eye(nw) + Dd.T @ (rho[:, None] * Dd)
    K[:nw, nw:] = Ad.T
    K[nw:, :nw] = Ad
    Kinv = np.linalg.inv(K)
    out = {"status": 0, "history": []}
    for it in range(1, max_iter + 1):
        g = z - y / rho
        wt = (Kinv @ np.concatenate([-(hd - sigma * w - Dd.T @ (rho * g)), bd]))[:nw]
        last = it >= max_iter
        check = last or it % check_every == 0
        w0, y0, z0 = w, y, z
        v = Dd @ wt
        vrel = alpha * v + (1 - alpha) * z
        w = alpha * wt + (1 - alpha) * w
        z = np.clip(vrel + y / rho, lb, ub)
        y = y + rho * (vrel - z)
        if check:
            dwn = Dd @ w
            rp, rd = np.max(np.abs(dwn - z)), np.max(np.abs(Dd.T @ (rho * (z - z0))))
            dty = np.max(np.abs(Dd.T @ y))
            out["iters"] = it
            if rp <= eps_abs + eps_rel * max(np.max(np.abs(dwn)), np.max(np.abs(z))) and rd <= eps_abs + eps_rel * dty:
                out["status"] = 1
                break
            if detect:
                meas, verdict = certificate_measures(pm, x0, lb, ub, y - y0, w - w0, eps_prim_inf, eps_dual_inf)
                out["history"].append((it, meas))
                if verdict:
                    out["status"] = 2 if verdict & 1 else 3
                    out["dy"], out["dw"] = y - y0, w - w0
                    break
    out.update(w=w, y=y, z=z)
    return out


# ---------------------------------------------------------------------------
# problem constructions shared by the CPU and GPU tests
# ---------------------------------------------------------------------------
def random_packed(n, m, N, ncs, seed, radius=0.9):
    """A random strictly convex problem with |eig(A)| <= radius, random rows."""
    from pdplqr.model import PackedModel

    g = np.random.default_rng(seed)
    s = n + m
    A = g.standard_normal((n, n))
    A *= radius / np.max(np.abs(np.linalg.eigvals(A)))
    E = np.empty(N * n * s)
    H = np.empty(N * s * s + n * n)
    for k in range(N):
        Ek = np.hstack([g.standard_normal((n, m)) / np.sqrt(n), A + 0.02 * g.standard_normal((n, n))])
        E[k * n * s:(k + 1) * n * s] = Ek.reshape(-1, order="F")
        M = g.standard_normal((s, s))
        H[k * s * s:(k + 1) * s * s] = (M @ M.T / s + 0.5 * np.eye(s)).reshape(-1, order="F")
    M = g.standard_normal((n, n))
    H[N * s * s:] = (M @ M.T / n + 0.5 * np.eye(n)).reshape(-1, order="F")
    ncs = np.asarray(ncs, dtype=np.int32)
    nd = int(sum(int(nc) * (s if k < N else n) for k, nc in enumerate(ncs)))
    return PackedModel(n, m, N, ncs, E, 0.1 * g.standard_normal(N * n), H, g.standard_normal(N * s + n),
                       g.standard_normal(nd))


def rollout(pm, x0, us):
    """The stacked w of the inputs us [N][m] from x0."""
    n, m, N = pm.n, pm.m, pm.N
    s = n + m
    st = stage_views(pm)
    w = np.zeros(N * s + n)
    x = x0
    for k in range(N):
        w[k * s:k * s + m] = us[k]
        w[k * s + m:(k + 1) * s] = x
        x = st[k][0] @ w[k * s:(k + 1) * s] + st[k][1]
    w[N * s:] = x
    return w


def rows_of(pm, w):
    """D w, stacked."""
    n, m, N = pm.n, pm.m, pm.N
    s = n + m
    return np.concatenate([st[4] @ (w[k * s:(k + 1) * s] if k < N else w[N * s:])
                           for k, st in enumerate(stage_views(pm))])


def box_problem(n, m, N, kind, seed, margin=0.2, terminal_row=True):
    """(pm, x0, lb, ub) with rows u_k (k < N) and x_N[0]: ncs = [m] * N + [1].
    kind 'feasible': the bounds are D w_feas +- margin around a rolled-out
    trajectory (feasible by construction); 'contradictory': the same, but rows
    0 and 1 of stage 0 both read u_0[0], one asking >= 1, the other <= -1;
    'dynamics': |u| <= 0.01 and x_N[0] in [1e3, 2e3] (out of reach).
    terminal_row=False drops the row on x_N (ncs = [m] * N + [0]: with m = 4 the
    uniform layout of the fused update); 'dynamics' needs it."""
    s = n + m
    tr = 1 if terminal_row else 0
    assert tr or kind != "dynamics"
    pm = random_packed(n, m, N, [m] * N + [tr], seed)
    D = np.zeros(pm.D.size)
    for k in range(N):
        Dk = np.hstack([np.eye(m), np.zeros((m, n))])
        if kind == "contradictory" and k == 0:
            Dk[1] = Dk[0]
        D[k * m * s:(k + 1) * m * s] = Dk.reshape(-1, order="F")
    if tr:
        D[N * m * s] = 1.0
    pm.D = D
    g = np.random.default_rng(seed + 7919)
    x0 = g.standard_normal(n)
    if kind == "dynamics":
        lb, ub = np.full(N * m + 1, -0.01), np.full(N * m + 1, 0.01)
        lb[-1], ub[-1] = 1e3, 2e3
        return pm, x0, lb, ub
    v = rows_of(pm, rollout(pm, x0, 0.3 * g.standard_normal((N, m))))
    lb, ub = v - margin, v + margin
    if kind == "contradictory":
        lb[0], ub[0] = 1.0, INF_BOUND
        lb[1], ub[1] = -INF_BOUND, -1.0
    return pm, x0, lb, ub


def unbounded_problem(n, m, N, seed, margin=0.5):
    """R = 0, S = 0, B = 0, r = 1: the inputs do not move the state and have a
    linear cost and no bound, so the cost is unbounded below.  Two random rows
    on the state per stage (one at the terminal), boxed around a rollout."""
    s = n + m
    pm = random_packed(n, m, N, [2] * N + [1], seed)
    for k in range(N):
        E = pm.E[k * n * s:(k + 1) * n * s].reshape(n, s, order="F")
        E[:, :m] = 0.0
        pm.E[k * n * s:(k + 1) * n * s] = E.reshape(-1, order="F")
        H = pm.H[k * s * s:(k + 1) * s * s].reshape(s, s, order="F")
        H[:m, :] = 0.0
        H[:, :m] = 0.0
        pm.H[k * s * s:(k + 1) * s * s] = H.reshape(-1, order="F")
        pm.h[k * s:k * s + m] = 1.0
        D = pm.D[k * 2 * s:(k + 1) * 2 * s].reshape(2, s, order="F")
        D[:, :m] = 0.0
        pm.D[k * 2 * s:(k + 1) * 2 * s] = D.reshape(-1, order="F")
    g = np.random.default_rng(seed + 7919)
    x0 = g.standard_normal(n)
    v = rows_of(pm, rollout(pm, x0, np.zeros((N, m))))
    return pm, x0, v - margin, v + margin
