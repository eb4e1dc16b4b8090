"""numpy restatement of the ADMM polish (csrc/kernels_polish.hip, csrc/admm.hip;
DESIGN.md section 5.8; OSQP: Stellato et al. 2020 section 4), dense throughout,
on the layouts and the loop of tests/admm_infeas_ref.py.

The polish guesses the active rows from the ADMM (y, z), solves the
equality-constrained problem on them regularised by delta, and refines.  With
the dynamics kept as hard constraints and the active rows' multipliers
eliminated, one refinement step (K + dK) t+ = g + dK t is

    w+ = argmin 1/2 w^T H w + h^T w + delta/2 |w - w_j|^2
                + 1/(2 delta) |D_a w - (b_a - delta y_j)|^2     s.t. dynamics
    y+ = y_j + (D_a w+ - b_a) / delta   on the active rows, 0 elsewhere

which is the solver's own penalised x-update with sigma = delta, rho = 1/delta
on the active rows and 0 on the rest.
"""
import numpy as np

from admm_infeas_ref import INF_BOUND, dense_problem, stage_views

# order of the 4 KKT measures (include/pdplqr.h: pdplqr_admm_kkt_residuals)
K_ROW, K_DYN, K_GRAD, K_OBJ = range(4)

# OSQP's polish defaults and the threshold of its acceptance rule
DELTA, REFINE_ITER, ACCEPT_TINY = 1e-6, 3, 1e-10


def _y_off(pm):
    return np.concatenate([[0], np.cumsum(pm.ncs)]).astype(int)


def kkt_measures(pm, x0, lb, ub, w, y):
    """[row residual, dynamics residual, reduced gradient, objective] of (w, y).

    The row residual is the natural map max |v - clamp(v + y, lb, ub)|, v = D w:
    zero iff v is within the bounds and y in their normal cone.  The reduced
    gradient is max_k |g_k| of nu_N = q_N, [g_k; nu_k] = q_k + E_k^T nu_{k+1},
    q_k = H_k w_k + h_k + D_k^T y_k."""
    n, m, N = pm.n, pm.m, pm.N
    s = n + m
    st, yo = stage_views(pm), _y_off(pm)
    lo = np.where(lb <= -INF_BOUND, -np.inf, lb)
    hi = np.where(ub >= INF_BOUND, np.inf, ub)
    wk = [w[k * s:(k + 1) * s] if k < N else w[N * s:] for k in range(N + 1)]
    row, obj = 0.0, 0.0
    dyn = np.max(np.abs(wk[0][m:] - x0))
    q = []
    for k in range(N + 1):
        E, c, H, h, D = st[k]
        yk = y[yo[k]:yo[k + 1]]
        obj += 0.5 * wk[k] @ (H @ wk[k]) + h @ wk[k]
        qk = H @ wk[k] + h
        if pm.ncs[k]:
            v = D @ wk[k]
            row = max(row, np.max(np.abs(v - np.clip(v + yk, lo[yo[k]:yo[k + 1]], hi[yo[k]:yo[k + 1]]))))
            qk = qk + D.T @ yk
        q.append(qk)
        if k < N:
            xn = wk[k + 1][m:] if k + 1 < N else wk[N]
            dyn = max(dyn, np.max(np.abs(xn - E @ wk[k] - c)))
    nu, grad = q[N], 0.0
    for k in range(N - 1, -1, -1):
        v = q[k] + st[k][0].T @ nu
        grad = max(grad, np.max(np.abs(v[:m])))
        nu = v[m:]
    return np.array([row, dyn, grad, obj])


def classify(y, z, lb, ub):
    """OSQP's active-set guess: (lower, upper, b, y0, n_active).  An equality
    row counts as lower-active."""
    lower = (lb == ub) | (z - lb < -y)
    upper = ~lower & (ub - z < y)
    act = lower | upper
    b = np.where(lower, lb, np.where(upper, ub, 0.0))
    return lower, upper, b, np.where(act, y, 0.0), int(np.count_nonzero(act))


def classification_margin(y, z, lb, ub):
    """The least distance of a row's two tests from their thresholds."""
    return float(np.min(np.minimum(np.abs(z - lb + y), np.abs(ub - z - y))))


def prox_step(Hd, hd, Dd, Ad, bd, act, b, wj, yj, delta):
    """One refinement step in the proximal form (module docstring)."""
    nw, na = Hd.shape[0], Ad.shape[0]
    Da = Dd[act]
    K = np.zeros((nw + na, nw + na))
    K[:nw, :nw] = Hd + delta * np.eye(nw) + Da.T @ Da / delta
    K[:nw, nw:] = Ad.T
    K[nw:, :nw] = Ad
    rhs = np.concatenate([-hd + delta * wj + Da.T @ ((b[act] - delta * yj[act]) / delta), bd])
    w = np.linalg.solve(K, rhs)[:nw]
    y = np.zeros_like(yj)
    y[act] = yj[act] + (Da @ w - b[act]) / delta
    return w, y


def refinement_step(Hd, hd, Dd, Ad, bd, act, b, wj, yj, nuj, delta):
    """The same step as iterative refinement on the dense regularised KKT matrix
    with the dynamics multipliers kept: (K + dK) t+ = g + dK t, t = (w, y_a, nu),
    dK = diag(delta I, -delta I, 0)."""
    nw, na = Hd.shape[0], Ad.shape[0]
    Da = Dd[act]
    ma = Da.shape[0]
    K = np.zeros((nw + ma + na, nw + ma + na))
    K[:nw, :nw] = Hd + delta * np.eye(nw)
    K[:nw, nw:nw + ma] = Da.T
    K[nw:nw + ma, :nw] = Da
    K[nw:nw + ma, nw:nw + ma] = -delta * np.eye(ma)
    K[:nw, nw + ma:] = Ad.T
    K[nw + ma:, :nw] = Ad
    rhs = np.concatenate([-hd + delta * wj, b[act] - delta * yj[act], bd])
    t = np.linalg.solve(K, rhs)
    y = np.zeros_like(yj)
    y[act] = t[nw:nw + ma]
    return t[:nw], y, t[nw + ma:]


def polish(pm, x0, lb, ub, w, y, z, delta=DELTA, refine_iter=REFINE_ITER):
    """Classify, then refine_iter + 1 steps from (w, y0).  Returns a dict: w, y,
    z = clamp(D w), act, b, n_active."""
    Hd, hd, Dd, Ad, bd = dense_problem(pm, x0)
    lower, upper, b, yj, n_act = classify(y, z, lb, ub)
    act = lower | upper
    wj = w.copy()
    for _ in range(refine_iter + 1):
        wj, yj = prox_step(Hd, hd, Dd, Ad, bd, act, b, wj, yj, delta)
    return {"w": wj, "y": yj, "z": np.clip(Dd @ wj, lb, ub), "act": act, "b": b, "n_active": n_act}


def accept(before, after):
    """OSQP's acceptance rule on the KKT measures of the ADMM iterate and of the
    polished pair: pri = max(row, dynamics), dua = reduced gradient."""
    pri, dua = max(before[K_ROW], before[K_DYN]), before[K_GRAD]
    pri_p, dua_p = max(after[K_ROW], after[K_DYN]), after[K_GRAD]
    return bool((pri_p < pri and dua_p < dua) or (pri_p < pri and dua < ACCEPT_TINY)
                or (dua_p < dua and pri < ACCEPT_TINY))


def active_set_solution(pm, x0, act, b):
    """The exact solution of the equality-constrained problem on the active set
    `act` (no regularisation): a dense solve of [H Da^T A^T; Da 0 0; A 0 0]."""
    Hd, hd, Dd, Ad, bd = dense_problem(pm, x0)
    nw, na = Hd.shape[0], Ad.shape[0]
    Da = Dd[act]
    ma = Da.shape[0]
    K = np.zeros((nw + ma + na, nw + ma + na))
    K[:nw, :nw] = Hd
    K[:nw, nw:nw + ma] = Da.T
    K[nw:nw + ma, :nw] = Da
    K[:nw, nw + ma:] = Ad.T
    K[nw + ma:, :nw] = Ad
    t = np.linalg.solve(K, np.concatenate([-hd, b[act], bd]))
    y = np.zeros(Dd.shape[0])
    y[act] = t[nw:nw + ma]
    return t[:nw], y
