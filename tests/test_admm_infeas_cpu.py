"""CPU-side checks of the ADMM infeasibility detection:

* the costate recursion of tests/admm_infeas_ref.py (the statement
  k_infeas_primal implements) against a dense null-space computation;
* the numpy loop certifies the constructions the GPU tests use, and solves
  the problems that are feasible by construction;
* the C ABI declares and exports the new calls, and the argument checks that
  need no device.
No GPU call is made here.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import admm_infeas_ref as ref
from conftest import ROOT

SHAPES = [
    (2, 1, 3, [1, 2, 1, 1]),
    (3, 2, 6, [2, 0, 3, 1, 0, 2, 1]),  # ragged: stages without rows, rows at the terminal
    (3, 2, 6, [0, 0, 3, 1, 0, 2, 0]),
    (12, 4, 4, [4, 4, 4, 4, 3]),
]


@pytest.mark.parametrize("n,m,N,ncs", SHAPES)
def test_recursion_matches_dense_null_space(n, m, N, ncs):
    """g = Z_u^T D^T dy and beta = (D w_p)^T dy, with Z an orthonormal null-space
    basis of the dynamics matrix from its SVD, re-based so that its input rows
    are the identity (Z_u = Z Z[U]^-1: the parametrisation by the inputs), and
    w_p the zero-input rollout.  1e-12 relative."""
    s = n + m
    for seed in range(3):
        pm = ref.random_packed(n, m, N, ncs, seed, radius=1.0)
        g = np.random.default_rng(100 + seed)
        x0, dy = g.standard_normal(n), g.standard_normal(int(sum(ncs)))
        _, _, Dd, Ad, bd = ref.dense_problem(pm, x0)
        _, sv, Vt = np.linalg.svd(Ad)
        assert sv.min() > 1e-8  # full row rank: the null space has N m dimensions
        Z = Vt[Ad.shape[0]:].T
        U = np.concatenate([np.arange(k * s, k * s + m) for k in range(N)])
        Zu = Z @ np.linalg.inv(Z[U])
        assert np.max(np.abs(Ad @ Zu)) < 1e-10
        q = Dd.T @ dy
        g_ref = (Zu.T @ q).reshape(N, m)
        w_p = ref.rollout(pm, x0, np.zeros((N, m)))
        assert np.max(np.abs(Ad @ w_p - bd)) < 1e-12
        beta_ref = (Dd @ w_p) @ dy
        g_rec, beta = ref.costate_recursion(pm, x0, dy)
        assert np.max(np.abs(g_rec - g_ref)) <= 1e-12 * np.max(np.abs(g_ref))
        # (beta is a sum that may cancel: relative to the sum of its terms' magnitudes)
        assert abs(beta - beta_ref) <= 1e-12 * (np.abs(Dd @ w_p) @ np.abs(dy))


def test_measures_skip_halves_and_zero_dy():
    pm, x0, lb, ub = ref.box_problem(3, 2, 6, "feasible", 1)
    g = np.random.default_rng(0)
    dw = g.standard_normal(pm.h.size)
    meas, verdict = ref.certificate_measures(pm, x0, lb, ub, np.zeros(lb.size), None)
    assert verdict == 0 and not meas.any()  # |dy| = 0 never certifies
    meas, verdict = ref.certificate_measures(pm, x0, lb, ub, None, dw)
    assert not meas[:4].any() and meas[ref.M_DW] == np.max(np.abs(dw)) and verdict == 0


@pytest.mark.parametrize("n,m,N", [(3, 2, 6), (12, 4, 8)])
def test_numpy_loop_on_the_constructions(n, m, N):
    """The problems the GPU tests use: the infeasible ones are certified, the
    ones feasible by construction are solved (rho = 10, zero start)."""
    for kind, want in (("feasible", 1), ("contradictory", 2), ("dynamics", 2)):
        pm, x0, lb, ub = ref.box_problem(n, m, N, kind, 2)
        r = ref.admm_loop(pm, x0, lb, ub, np.full(lb.size, 10.0), eps_abs=1e-6, eps_rel=0.0, max_iter=1000)
        assert r["status"] == want, (kind, r["status"], r["iters"])
        if want == 2:
            # the certificate on its own: a Farkas-type statement about the stacked problem.
            # For every w with A w = b: dy^T D w = beta + g^T u, so with g ~ 0 the value
            # dy^T D w is beta for all feasible w, while the box allows at most the support sum
            meas, verdict = ref.certificate_measures(pm, x0, lb, ub, r["dy"], None)
            assert verdict == 1 and meas[ref.M_SUPPORT] < 0


@pytest.mark.parametrize("n,m,N", [(2, 1, 5), (6, 3, 8)])
def test_numpy_loop_unbounded(n, m, N):
    pm, x0, lb, ub = ref.unbounded_problem(n, m, N, 1)
    r = ref.admm_loop(pm, x0, lb, ub, np.full(lb.size, 10.0), eps_abs=1e-6, eps_rel=0.0, max_iter=200)
    assert r["status"] == 3 and r["iters"] == 25
    _, verdict = ref.certificate_measures(pm, x0, lb, ub, None, r["dw"])
    assert verdict == 2


NEW_CALLS = ["pdplqr_admm_set_infeasibility_detection", "pdplqr_admm_status", "pdplqr_admm_certificate",
             "pdplqr_admm_check_certificates"]


def test_abi_declares_and_exports_the_new_calls():
    from pdplqr import _lib

    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pdplqr.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pdplqr_[a-z_]+)\s*\(", txt))
    L = _lib.lib()
    for nm in NEW_CALLS:
        assert nm in declared, nm
        assert hasattr(L, nm), nm
        assert nm in _lib.EXPORTS, nm
    for nm, val in (("UNSOLVED", 0), ("SOLVED", 1), ("PRIMAL_INFEASIBLE", 2), ("DUAL_INFEASIBLE", 3)):
        assert re.search(rf"#define PDPLQR_ADMM_{nm} {val}\b", txt)
        assert getattr(_lib, "PDPLQR_ADMM_" + nm) == val


def test_null_handle_is_invalid_without_a_device():
    from pdplqr import _lib

    L = _lib.lib()
    st = (C.c_int32 * 1)()
    assert L.pdplqr_admm_set_infeasibility_detection(None, 1, 1e-4, 1e-4) == -1
    assert L.pdplqr_admm_status(None, st) == -1
    assert L.pdplqr_admm_certificate(None, None, None, 0) == -1
    assert L.pdplqr_admm_check_certificates(None, None, None, None, None, None, 1e-4, 1e-4, None, None, 0) == -1
