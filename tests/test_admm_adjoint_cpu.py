"""CPU checks of the mathematics of pdplqr_admm_adjoint (no GPU; DESIGN.md
section 5.9): the dense restatement of the call's four steps
(tests/admm_adjoint_ref.py: restate) against autograd through the KKT solve on
the active set (adjoint_rows_ref.active_set_solution), with and without a
cotangent on D w.

Measured here (float64, delta = 1e-6, refine_iter = 3, four solves): the worst
error over the eight gradient arrays, max-norm relative to the array's, is
2e-15 .. 9e-14 on the u-box problems and 2e-11 .. 3e-10 on the ragged problem
with dense rows (there the dense active-set solve of the reference is itself the
less accurate side: |D_a v| of the restatement is at 1e-16 after three solves);
max|D_a v| falls by 4 to 5 orders per solve: 1e-5, 1e-9, 1e-13, 1e-17.  With one
solve (refine_iter = 0) the error is 1e-6 .. 2e-4.  The bound per case is
admm_adjoint_ref.cpu_bound, computed from the two matrices alone: 1e-12 ..
1e-10 on the u-box problems, 2e-6 on the ragged one (an a-priori bound of a
solve with the 1/delta penalty on dense rows; loose by four digits there).
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import admm_adjoint_ref as ar
from conftest import ROOT

ALL = [(n, m, N, seed, rg) for n, m, N, seeds, rg in ar.CASES for seed in (seeds or ar.RAGGED_SEEDS)]


def _id(cse):
    return "-".join(map(str, cse[:4])) + ("-ragged" if cse[4] else "")


@pytest.mark.parametrize("cse", ALL, ids=_id)
def test_premise_strict_complementarity(cse):
    """The reference alone: every case has a margin >= 1e-2 between its active and
    inactive rows, so rounding cannot move a row across."""
    pr = ar.problem(*cse)
    act = pr["at_lb"] | pr["at_ub"]
    print(_id(cse), "margin", pr["margin"], "active", pr["n_active"], "of", act.size, "admm iters", pr["iters"])
    assert pr["margin"] >= 1e-2
    assert 0 < pr["n_active"] < act.size
    if cse[4]:  # the ragged problem: an equality row, infinite bounds, at most m active rows per stage
        n, m, N, ncs = pr["dims"]
        assert ncs == (2, 0, 3, 1, 2, 2)
        assert (pr["lb"] == pr["ub"]).sum() == 1 and pr["at_lb"][pr["lb"] == pr["ub"]].all()
        assert (pr["lb"] <= -ar.INF).any() and (pr["ub"] >= ar.INF).any()
        off = np.cumsum((0,) + ncs)
        assert all(act[off[k]:off[k + 1]].sum() <= m for k in range(N + 1))
        assert pr["at_lb"].sum() >= 2 and pr["at_ub"].sum() >= 1


@pytest.mark.parametrize("with_gvs", [False, True], ids=["gws", "gws+gvs"])
@pytest.mark.parametrize("cse", ALL, ids=_id)
def test_restatement_matches_autograd(cse, with_gvs):
    g = ar.graded(*cse, with_gvs)
    pr = ar.problem(*cse)
    print(_id(cse), with_gvs, "errors", g["err"], "|D_a v| per step", [st[0] for st in g["steps"]])
    tol = ar.cpu_bound(pr)
    assert ar.relmax(g["wt"], g["ws"]) < tol  # w~ is the active-set optimum
    for k in ar.KEYS:
        assert g["err"][k] < tol, (k, g["err"][k], tol)
    # the sides: an inactive row has no bound gradient, an active one exactly one
    assert not g["mine"]["lb"][~pr["at_lb"]].any() and not g["mine"]["ub"][~pr["at_ub"]].any()
    assert g["mine"]["lb"][pr["at_lb"]].all() and g["mine"]["ub"][pr["at_ub"]].all()


@pytest.mark.parametrize("cse", ALL, ids=_id)
def test_refinement_contracts(cse):
    """max|D_a v| falls by at least three orders per solve until it reaches
    rounding (1e-13 of max|v|)."""
    steps = ar.graded(*cse, True)["steps"]
    assert len(steps) == 4
    for (a, _), (b, vmax) in zip(steps, steps[1:]):
        assert b <= max(1e-3 * a, 1e-13 * vmax), steps
    assert steps[-1][0] <= 1e-13 * steps[-1][1]


@pytest.mark.parametrize("cse", [ALL[0], ALL[5], ALL[-1]], ids=_id)
def test_one_solve_is_not_enough(cse):
    """refine_iter = 0 is the plain regularised adjoint: it misses by more than 1e-6."""
    g = ar.graded(*cse, False, 0)
    print(_id(cse), g["err"])
    assert max(g["err"].values()) > 1e-6
    assert max(g["err"].values()) < 1e-2  # (but it is the right quantity)


def test_abi_declares_and_exports_admm_adjoint():
    from pdplqr import _lib

    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pdplqr.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+pdplqr_admm_adjoint\s*\(", txt)
    assert re.search(r"\bint\s+pdplqr_admm_adjoint_info\s*\(", txt)
    for nm, val in (("EXACT", 1), ("APPROX", 2), ("FAILED", 3)):
        assert re.search(rf"#define\s+PDPLQR_ADMM_ADJOINT_{nm}\s+{val}\b", txt)
        assert getattr(_lib, f"PDPLQR_ADMM_ADJOINT_{nm}") == val
    assert "pdplqr_admm_adjoint" in _lib.EXPORTS and "pdplqr_admm_adjoint_info" in _lib.EXPORTS
    L = _lib.lib()
    buf = np.zeros(4)
    p = C.c_void_p(buf.ctypes.data)
    assert L.pdplqr_admm_adjoint(None, p, None, None, None, None, None, None, None, None, None, 0) == -1
    assert L.pdplqr_last_error()
    assert L.pdplqr_admm_adjoint_info(None, None, None) == -1


def test_layer_mode_argument():
    """backward_mode is checked before any handle is made."""
    from pdplqr import BoxLQRLayer

    with pytest.raises(ValueError, match="requires polish"):
        BoxLQRLayer(3, 2, 6, 1, [2] * 6 + [0], rho=10.0, backward_mode="active_set")
    with pytest.raises(ValueError, match="backward_mode"):
        BoxLQRLayer(3, 2, 6, 1, [2] * 6 + [0], rho=10.0, polish=True, backward_mode="exact")
