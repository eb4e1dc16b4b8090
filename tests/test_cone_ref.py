"""The CPU restatement of the ADMM loop with second-order cones
(tests/admm_cone_ref.py) checked without the device code: the projection's
defining properties, and converged runs against dense KKT algebra
(admm_infeas_ref.dense_problem) -- z in the set, the natural-map residual
max|z - Pi(z + y)| and the reduced gradient of H w + h + D^T y on the dynamics'
null space.  No GPU."""
import numpy as np
import pytest

import admm_cone_ref as R
from admm_infeas_ref import dense_problem

EPS = 2.0 ** -52


def _vectors():
    g = np.random.default_rng(11)
    out = []
    for d in (2, 3, 5, 10, 65):
        for scale in (1e-100, 1e-3, 1.0, 1e3, 1e100):
            for _ in range(6):
                p = g.standard_normal(d)
                p[0] *= g.choice([0.1, 1.0, 3.0])
                out.append(scale * p)
    return out


def test_projection_is_idempotent_and_lands_in_the_cone():
    for p in _vectors():
        q, _ = R.proj_cone(p)
        m = np.max(np.abs(p))
        assert R.cone_norm(q[1:]) <= q[0] + 8 * EPS * m
        q2, _ = R.proj_cone(q)
        assert np.max(np.abs(q2 - q)) <= 8 * EPS * m


def test_moreau_identity_and_orthogonality():
    """p = P_K(p) - P_K(-p) (K is self-dual, so -P_K(-p) is the projection onto
    the polar cone) and the two parts are orthogonal."""
    seen = set()
    for p in _vectors():
        a, ca = R.proj_cone(p)
        b, _ = R.proj_cone(-p)
        m = np.max(np.abs(p))
        assert np.max(np.abs(p - (a - b))) <= (p.size + 5) * EPS * m * 6
        assert abs(float(a @ b)) <= (p.size + 5) * EPS * 6 * float(np.linalg.norm(a) * np.linalg.norm(b)) + 1e-300
        seen.add(ca)
    assert seen == {0, 1, 2}


def test_the_three_cases_and_their_boundaries():
    x = np.array([3.0, 4.0])  # |x| = 5 exactly
    q, c = R.proj_cone(np.concatenate([[6.0], x]))
    assert c == 0 and np.array_equal(q, [6.0, 3.0, 4.0])
    q, c = R.proj_cone(np.concatenate([[5.0], x]))  # |x| = t: kept
    assert c == 0 and np.array_equal(q, [5.0, 3.0, 4.0])
    q, c = R.proj_cone(np.concatenate([[-5.0], x]))  # |x| = -t: zero
    assert c == 1 and not q.any()
    q, c = R.proj_cone(np.concatenate([[-7.0], x]))
    assert c == 1 and not q.any()
    q, c = R.proj_cone(np.concatenate([[1.0], x]))  # a = (1 + 1/5) / 2 = 0.6
    assert c == 2 and np.allclose(q, [3.0, 1.8, 2.4], rtol=4 * EPS, atol=0)
    q, c = R.proj_cone(np.concatenate([[0.0], x]))  # t = 0: half of x
    assert c == 2 and np.allclose(q, [2.5, 1.5, 2.0], rtol=4 * EPS, atol=0)
    # x = 0 never reaches the division
    q, c = R.proj_cone(np.array([2.0, 0.0, 0.0]))
    assert c == 0 and np.array_equal(q, [2.0, 0.0, 0.0])
    q, c = R.proj_cone(np.array([-2.0, 0.0, 0.0]))
    assert c == 1 and not q.any()
    q, c = R.proj_cone(np.array([0.0, 0.0, 0.0]))
    assert c == 0 and not q.any()


def test_mixed_set_projection_leaves_box_rows_to_the_clamp():
    n, m, N = 6, 3, 7
    bt = R.build_batch(n, m, N, R.ragged_layout(), [0])
    ncs, cones, lb, ub = bt["ncs"], bt["cones"], bt["lb"][0], bt["ub"][0]
    assert ncs[1] == 0 and (3, 0, 10) in cones and (N, 0, n + 1) in cones
    assert [c for c in cones if c[0] == 2] == [(2, 1, 3), (2, 6, 4)]
    v = np.random.default_rng(3).standard_normal(lb.size)
    out, info = R.project(v, lb, ub, ncs, cones)
    box = np.ones(lb.size, dtype=bool)
    for (q, d) in R.cone_rows(ncs, cones):
        box[q:q + d] = False
    assert box.any() and np.array_equal(out[box], np.clip(v, lb, ub)[box])
    assert R.in_set_violation(out, lb, ub, ncs, cones) <= 16 * EPS
    assert len(info) == len(cones)


CASES = [("6/3", 6, 3, 20, {}, 0), ("6/3", 6, 3, 20, {}, 5), ("20/12", 20, 12, 8, {}, 2),
         ("28/12", 28, 12, 5, dict(ucone=0.5, xcone=4.0), 1), ("ragged", 6, 3, 7, None, 2)]


@pytest.mark.parametrize("name,n,m,N,kw,seed", CASES)
@pytest.mark.parametrize("rho0,adaptive", [(1.0, False), (0.1, True)])
def test_converged_runs_satisfy_the_dense_kkt_conditions(name, n, m, N, kw, seed, rho0, adaptive):
    eps = 1e-4
    lay = R.ragged_layout() if kw is None else R.standard_layout(n, m, N, **kw)
    pm, x0, lb, ub, cones = R.build_problem(n, m, N, lay, seed)
    ncs = [int(x) for x in pm.ncs]
    w, y, z, info = R.admm_cone_solve(pm, x0, lb, ub, np.full(lb.size, rho0), cones, eps_abs=eps, eps_rel=eps,
                                      adaptive_rho=adaptive)
    assert info["converged"] and info["iters"] < 4000
    assert (info["rho_updates"] >= 1) == adaptive
    assert 2 in info["cone_case"], "vacuous: no cone on its boundary"
    Hd, hd, Dd, Ad, bd = dense_problem(pm, x0)
    # z is in the set, (z, y) a fixed point of the natural map: y in the normal cone at z
    assert R.in_set_violation(z, lb, ub, ncs, cones) <= 64 * EPS * max(1.0, np.max(np.abs(z)))
    zz, _ = R.project(z + y, lb, ub, ncs, cones)
    assert np.max(np.abs(z - zz)) <= 1e-13 * max(1.0, np.max(np.abs(z + y)))
    # the dynamics hold (the x-update solves them exactly; w is an affine mix of such solutions)
    assert np.max(np.abs(Ad @ w - bd)) <= 1e-9 * max(1.0, np.max(np.abs(w)))
    # stationarity on the dynamics' null space, and D w = z, at the scale of eps
    _, sv, Vt = np.linalg.svd(Ad)
    Z = Vt[Ad.shape[0]:].T
    assert sv.min() > 1e-8
    grad = Hd @ w + hd + Dd.T @ y
    scale = max(1.0, np.max(np.abs(Dd.T @ y)), np.max(np.abs(Hd @ w)), np.max(np.abs(hd)))
    assert np.max(np.abs(Z.T @ grad)) <= 20 * eps * scale * np.sqrt(Z.shape[0])
    assert np.max(np.abs(Dd @ w - z)) <= eps * (1.0 + max(np.max(np.abs(Dd @ w)), np.max(np.abs(z))))
