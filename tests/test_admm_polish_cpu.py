"""CPU checks of the mathematics behind the ADMM polish
on the dense numpy restatement tests/admm_polish_ref.py:

(a) one step of the proximal form (the penalised x-update the device runs)
    equals one step of iterative refinement on the dense regularised KKT matrix
    with the dynamics multipliers kept;
(b) the reduced gradient of kkt_measures is |Z^T (H w + h + D^T y)| for the
    null-space basis Z of the dynamics in input coordinates;
(c) the table of cases tests/test_gpu_polish.py runs on the device: the accepted
    ones land on the optimum, the two rejected ones are rejected by the row
    residual.
"""
import numpy as np
import pytest

import admm_infeas_ref as ref
import admm_polish_ref as pol

# (n, m, N, seed, margin, terminal_row, eps_abs) of ref.box_problem(..., "feasible", ...); the loop
# settings are those of the GPU tests
LOOP = dict(sigma=1e-6, alpha=1.6, check_every=5, eps_rel=0.0, detect=False)
ACCEPTED = [(3, 2, 6, 1, .05, True, 1e-3), (4, 2, 9, 2, .05, True, 1e-3), (12, 4, 8, 3, .05, True, 1e-3),
            (24, 8, 5, 7, .05, True, 1e-3), (6, 3, 20, 8, .05, True, 1e-3), (12, 4, 8, 3, .05, False, 1e-3),
            (5, 3, 7, 6, .1, True, 1e-2)]
REJECTED = [(5, 3, 7, 4, .1, True, 1e-2), (3, 2, 6, 5, .02, True, 1e-3)]


def _case(n, m, N, seed, margin, tr, eps):
    pm, x0, lb, ub = ref.box_problem(n, m, N, "feasible", seed, margin, terminal_row=tr)
    r = ref.admm_loop(pm, x0, lb, ub, np.ones(lb.size), eps_abs=eps, **LOOP)
    assert r["status"] == 1
    p = pol.polish(pm, x0, lb, ub, r["w"], r["y"], r["z"])
    before = pol.kkt_measures(pm, x0, lb, ub, r["w"], r["y"])
    after = pol.kkt_measures(pm, x0, lb, ub, p["w"], p["y"])
    return pm, x0, lb, ub, r, p, before, after


@pytest.mark.parametrize("n,m,N,seed", [(3, 2, 6, 1), (6, 3, 9, 2)])
def test_proximal_step_is_iterative_refinement(n, m, N, seed):
    pm, x0, lb, ub = ref.box_problem(n, m, N, "feasible", seed, .05)
    r = ref.admm_loop(pm, x0, lb, ub, np.ones(lb.size), eps_abs=1e-3, **LOOP)
    Hd, hd, Dd, Ad, bd = ref.dense_problem(pm, x0)
    lower, upper, b, y0, n_act = pol.classify(r["y"], r["z"], lb, ub)
    act = lower | upper
    assert 0 < n_act < lb.size
    wj, yj = r["w"].copy(), y0
    for step in range(3):
        wp, yp = pol.prox_step(Hd, hd, Dd, Ad, bd, act, b, wj, yj, pol.DELTA)
        # nu does not enter the step: (K + dK) t+ = g + dK t has dK = 0 on the dynamics block
        wr, yr, _ = pol.refinement_step(Hd, hd, Dd, Ad, bd, act, b, wj, yj, None, pol.DELTA)
        ew = np.max(np.abs(wp - wr)) / np.max(np.abs(wr))
        ey = np.max(np.abs(yp - yr)) / np.max(np.abs(yr))
        print((n, m, N), "step", step, "w", ew, "y", ey)
        assert ew < 1e-9 and ey < 1e-9
        assert not yp[~act].any()
        wj, yj = wp, yp


@pytest.mark.parametrize("n,m,N,ncs", [(3, 2, 6, [2, 0, 3, 1, 0, 2, 1]), (6, 3, 9, [2] * 9 + [0])])
def test_reduced_gradient_is_null_space_projection(n, m, N, ncs):
    g = np.random.default_rng(n + N)
    pm = ref.random_packed(n, m, N, ncs, 11)
    x0 = g.standard_normal(n)
    ny, nw, s = int(sum(ncs)), N * (n + m) + n, n + m
    w, y = g.standard_normal(nw), g.standard_normal(ny)
    lb, ub = -np.ones(ny), np.ones(ny)
    Hd, hd, Dd, Ad, bd = ref.dense_problem(pm, x0)
    iu = np.concatenate([np.arange(k * s, k * s + m) for k in range(N)])
    ix = np.setdiff1d(np.arange(nw), iu)
    # A [w_u; w_x] = b with A_x square and invertible: Z = [I; -A_x^{-1} A_u]
    Z = np.zeros((nw, iu.size))
    Z[iu] = np.eye(iu.size)
    Z[ix] = -np.linalg.solve(Ad[:, ix], Ad[:, iu])
    assert np.max(np.abs(Ad @ Z)) < 1e-12
    want = np.max(np.abs(Z.T @ (Hd @ w + hd + Dd.T @ y)))
    got = pol.kkt_measures(pm, x0, lb, ub, w, y)[pol.K_GRAD]
    assert abs(got - want) <= 1e-12 * want
    # the other measures, dense
    meas = pol.kkt_measures(pm, x0, lb, ub, w, y)
    v = Dd @ w
    assert abs(meas[pol.K_ROW] - np.max(np.abs(v - np.clip(v + y, lb, ub)))) <= 1e-14
    assert abs(meas[pol.K_DYN] - np.max(np.abs(Ad @ w - bd))) <= 1e-13
    assert abs(meas[pol.K_OBJ] - (0.5 * w @ Hd @ w + hd @ w)) <= 1e-12 * abs(meas[pol.K_OBJ])


def test_row_residual_sees_sign_and_complementarity():
    pm = ref.random_packed(2, 1, 2, [1, 1, 0], 3)
    x0 = np.zeros(2)
    w = np.zeros(2 * 3 + 2)
    lb, ub = np.array([-1.0, -ref.INF_BOUND]), np.array([1.0, ref.INF_BOUND])
    row = lambda y: pol.kkt_measures(pm, x0, lb, ub, w, np.array(y))[pol.K_ROW]  # noqa: E731
    assert row([0.0, 0.0]) == 0.0
    assert row([0.3, 0.0]) == 0.3   # a multiplier on an inactive row (v = 0 inside [-1, 1])
    assert row([0.0, -0.2]) == 0.2  # a free row takes no multiplier of either sign
    assert row([5.0, 0.0]) == 1.0   # ... capped by the distance to the bound


@pytest.mark.parametrize("case", ACCEPTED, ids=str)
def test_table_accepted(case):
    pm, x0, lb, ub, r, p, before, after = _case(*case)
    margin = pol.classification_margin(r["y"], r["z"], lb, ub)
    print(case, "iters", r["iters"], "margin", margin, "before", before, "after", after)
    assert pol.accept(before, after)
    assert margin > 1e-3
    tight = ref.admm_loop(pm, x0, lb, ub, np.full(lb.size, 10.0), sigma=1e-6, alpha=1.6, check_every=25,
                          eps_abs=1e-13, eps_rel=0.0, detect=False, max_iter=20000)
    assert tight["status"] == 1
    err = np.max(np.abs(p["w"] - tight["w"]))
    we, _ = pol.active_set_solution(pm, x0, p["act"], p["b"])
    print(case, "polish - tight ADMM", err, "polish - exact", np.max(np.abs(p["w"] - we)), "ADMM - exact",
          np.max(np.abs(r["w"] - we)))
    assert err < 1e-10
    assert np.max(np.abs(p["w"] - we)) < 1e-11
    assert np.max(np.abs(p["z"] - ref.rows_of(pm, p["w"]))) < 1e-12  # within the bounds: the clamp moves nothing


@pytest.mark.parametrize("case", REJECTED, ids=str)
def test_table_rejected_by_row_residual(case):
    pm, x0, lb, ub, r, p, before, after = _case(*case)
    print(case, "before", before, "after", after)
    assert not pol.accept(before, after)
    # the equality-constrained solve is fine (gradient and dynamics improve): the guess was wrong,
    # and only the row residual (a wrong-signed multiplier or a violated bound) shows it
    assert after[pol.K_GRAD] < before[pol.K_GRAD] and after[pol.K_DYN] < 1e-10
    assert after[pol.K_ROW] > 2 * before[pol.K_ROW]
