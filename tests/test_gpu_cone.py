"""Second-order cone rows of the ADMM loop on the GPU (pdplqr_admm_set_cones,
pdplqr_admm_project, csrc/kernels_cone.hip) against the
CPU restatement tests/admm_cone_ref.py, which tests/test_cone_ref.py checks on
its own.  Shapes: 6/3 N = 20 (16 lanes per stage: four stages per wave, two
block trips, the second partial), 20/12 N = 8 (32 lanes), 28/12 N = 5 (a wave
per stage, fewer stages than waves) and a ragged 6/3 layout (a stage without
rows; box rows, a cone, box rows, a second cone; a cone of dimension s + 1 whose
first D row is zero; a terminal cone of width n + 1).  Every restatement run
is computed once per module and shared.  All calls go through the C ABI."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import admm_cone_ref as R
from conftest import ROOT, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-9  # tests/test_gpu_admm.py: the same comparison against the same x-update

# name: (n, m, N, layout keywords (None: the ragged layout), seeds -- chosen on the CPU, see the tests)
SHAPES = {
    "6/3": (6, 3, 20, {}, (0, 2, 5, 9)),
    "20/12": (20, 12, 8, {}, (1, 2, 3, 6)),
    "28/12": (28, 12, 5, dict(ucone=0.5, xcone=4.0), (0, 1, 2, 3)),
    "ragged": (6, 3, 7, None, (1, 2, 4, 9)),
}
SOLVERS = [("serial", True), ("serial", False), ("parallel-LU", True), ("parallel-CHOLESKY", True)]
FIXED = dict(max_iter=40, eps_abs=0.0, eps_rel=0.0)
CONV = dict(max_iter=4000, check_every=25, eps_abs=1e-4, eps_rel=1e-4)


@pytest.fixture(scope="module", autouse=True)
def _device():
    from pdplqr import device_count

    assert device_count() > 0, "no HIP device visible: GPU tests must run on an MI355X"


@functools.lru_cache(maxsize=None)
def _batch(name, warm):
    n, m, N, kw, seeds = SHAPES[name]
    lay = R.ragged_layout() if kw is None else R.standard_layout(n, m, N, **kw)
    return R.build_batch(n, m, N, lay, seeds, warm_seed=1 if warm else None)


def _okw(solver):
    return {"num_segments": 4, "condensed": solver.split("-")[1]} if solver.startswith("parallel") else {}


@functools.lru_cache(maxsize=None)
def _ref(name, solver, warm, rho0, adaptive, fixed):
    """The restatement's runs of a batch (computed once, never modified)."""
    bt = _batch(name, warm)
    out = []
    for b, pm in enumerate(bt["pms"]):
        rho = np.full(bt["lb"].shape[1], rho0)
        out.append(R.admm_cone_solve(pm, bt["x0"][b], bt["lb"][b], bt["ub"][b], rho, bt["cones"], bt["ws"][b],
                                     bt["ys"][b], bt["zs"][b], solver=solver.split("-")[0], adaptive_rho=adaptive,
                                     **(FIXED if fixed else CONV), **_okw(solver)))
    return out


def _handle(bt, solver="serial", keep=True, cones="own", tensors=None):
    from pdplqr import BatchedLQRSolver

    p = bt["pms"][0]
    bs = BatchedLQRSolver(p.n, p.m, p.N, len(bt["pms"]), solver=solver.split("-")[0], keep_factors=keep,
                          ncs=bt["ncs"], **_okw(solver))
    A = tensors or bt
    bs.set_model(A["E"], A["c"], A["H"], A["h"], A["D"])
    if cones is not None:
        bs.set_cones(bt["cones"] if cones == "own" else cones)
    return bs


def _solve(bs, bt, rho0, **st):
    w, y, z = bt["ws"].copy(), bt["ys"].copy(), bt["zs"].copy()
    info = bs.admm_solve(bt["x0"], bt["lb"], bt["ub"], np.full(bt["lb"].shape, rho0), w, y, z, **st)
    assert np.count_nonzero(bs.status()) == 0
    return w, y, z, info


# ---------------------------------------------------------------------------
# 1. pdplqr_admm_project against the restatement
# ---------------------------------------------------------------------------
def _crafted(ncs, cones, seed):
    """[batch][ny] vectors: every cone of problem b gets pattern b % 8 at
    magnitude 1e-100 / 1e-3 / 1 / 1e100; lb is zero on the first half of the
    batch (the boundaries |x| = t, |x| = -t are then hit exactly), random on the
    second; box rows get values inside, outside and on their bounds."""
    g = np.random.default_rng(seed)
    ny = int(sum(ncs))
    scales = [1e-100, 1e-3, 1.0, 1e100]
    B = 8 * len(scales) * 2
    v, lb, ub = np.zeros((B, ny)), np.zeros((B, ny)), np.zeros((B, ny))
    rows = R.cone_rows(ncs, cones)
    for b in range(B):
        pat, sc, rnd = b % 8, scales[(b // 8) % 4], b >= B // 2
        lb[b] = -sc * g.uniform(0.5, 1.5, ny)
        ub[b] = sc * g.uniform(0.5, 1.5, ny)
        v[b] = sc * g.choice([0.0, 0.3, -0.7, 3.0, -3.0], ny)  # box rows: inside and outside
        v[b, ::5] = ub[b, ::5]
        v[b, 1::7] = lb[b, 1::7]
        for (q, d) in rows:
            x = np.zeros(d - 1)
            x[0] = 3.0
            if d > 2:
                x[-1] = 4.0
            nx = 5.0 if d > 2 else 3.0
            if pat in (5, 6, 7):
                x[:] = 0.0  # x = 0 with t > 0, t < 0, t = 0
            t = {0: 2 * nx, 1: nx, 2: -nx, 3: -2 * nx, 4: 0.25 * nx, 5: 1.0, 6: -1.0, 7: 0.0}[pat]
            if pat == 4:
                x = g.standard_normal(d - 1)  # a generic boundary point
            l = sc * g.standard_normal(d) if rnd else np.zeros(d)
            lb[b, q:q + d] = ub[b, q:q + d] = l
            v[b, q:q + d] = l + sc * np.concatenate([[t], x])
    return v, lb, ub


def _check_projection(out, v, lb, ub, ncs, cones):
    rows = R.cone_rows(ncs, cones)
    box = np.ones(v.shape[1], dtype=bool)
    for (q, d) in rows:
        box[q:q + d] = False
    seen = set()
    for b in range(v.shape[0]):
        ref, info = R.project(v[b], lb[b], ub[b], ncs, cones)
        assert np.array_equal(out[b][box], ref[box]), b  # box rows: to the bit
        for (q, d), (case, _) in zip(rows, info):
            pmax = np.max(np.abs(v[b, q:q + d] - lb[b, q:q + d]))
            err = np.max(np.abs(out[b, q:q + d] - ref[q:q + d]))
            # (q + 5) 2^-52 <= 1.6e-14 relative for q <= 65 squares, a root, a division, two products: six times that
            assert err <= 1e-13 * pmax, (b, q, d, case, err, pmax)
            seen.add(case)
    assert seen == {0, 1, 2}


@pytest.mark.parametrize("n,m,N,ncs,cones", [
    # 6/3: box rows, a cone of dimension 2, a cone of dimension s + 1; a stage without rows; a terminal cone
    (6, 3, 3, [14, 0, 11, 9], [(0, 2, 2), (0, 4, 10), (2, 0, 10), (3, 1, 7)]),
    # n + m = 64: the widest cone the handle takes (65 rows), a terminal cone of dimension 2
    (40, 24, 1, [66, 3], [(0, 1, 65), (1, 0, 2)]),
])
def test_project_matches_restatement(n, m, N, ncs, cones):
    import torch
    from pdplqr import BatchedLQRSolver

    v, lb, ub = _crafted(ncs, cones, seed=5)
    bs = BatchedLQRSolver(n, m, N, v.shape[0], ncs=ncs)
    bs.set_cones(cones)
    out = bs.project(v, lb, ub)
    _check_projection(out, v, lb, ub, ncs, cones)
    dev = torch.device("cuda", 0)
    dout = bs.project(*[torch.from_numpy(a).to(dev) for a in (v, lb, ub)])
    torch.cuda.synchronize()
    assert np.array_equal(dout.cpu().numpy(), out)
    bs.set_cones([])  # cleared: every row a box row
    assert np.array_equal(bs.project(v, lb, ub), np.minimum(np.maximum(v, lb), ub))
    bs.close()


# ---------------------------------------------------------------------------
# 2. fixed iterations
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("solver,keep", SOLVERS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_fixed_iterations_match_restatement(name, solver, keep):
    """eps = 0, 40 iterations from random warm starts at rho = 10: w, y, z within
    1e-9 relative of the restatement, prim_res as test_gpu_admm.py's
    test_fixed_iterations_match_oracle.  Not vacuous: over the batch, at the last
    iteration, the restatement has a cone strictly inside (case 0 with its
    argument's |x| < t) and one on its boundary."""
    bt = _batch(name, True)
    ref = _ref(name, solver, True, 10.0, True, True)
    cases = np.concatenate([r[3]["cone_case"] for r in ref])
    assert (cases == 2).any(), "vacuous: no cone on its boundary"
    interior = False
    for b, (ow, oy, oz, oi) in enumerate(ref):
        for (q, d), c in zip(R.cone_rows(bt["ncs"], bt["cones"]), oi["cone_case"]):
            p = oz[q:q + d] - bt["lb"][b, q:q + d]
            interior |= c == 0 and R.cone_norm(p[1:]) < p[0] * (1 - 1e-6)
    assert interior, "vacuous: no cone strictly interior"
    bs = _handle(bt, solver, keep)
    w, y, z, info = _solve(bs, bt, 10.0, **FIXED)
    bs.close()
    assert info["iterations"] == 40 and np.all(info["iters"] == 40) and not info["converged"].any()
    for b, (ow, oy, oz, oi) in enumerate(ref):
        errs = (rel_err(w[b], ow), rel_err(y[b], oy), rel_err(z[b], oz))
        print(name, solver, keep, b, "rel err w y z", errs, "prim", info["prim_res"][b], oi["prim_res"])
        assert max(errs) < TOL, (b, errs)
        assert abs(info["prim_res"][b] - oi["prim_res"]) <= 1e-9 * max(oi["prim_res"], 1e-300) + 1e-15


# ---------------------------------------------------------------------------
# 3. converged runs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("rho0,adaptive", [(1.0, False), (0.1, True)])
@pytest.mark.parametrize("name", list(SHAPES))
def test_converged_runs_match_restatement(name, rho0, adaptive):
    """eps_abs = eps_rel = 1e-4, a test every 25 iterations: per problem the
    iteration count, the convergence flag and the final rho (the device keeps
    the number of rescales per batch only; a problem's rho is 0.1 times the
    product of its rescale factors) equal the restatement's, the iterates agree
    at 1e-6 relative (the tolerance's scale), the batch does not converge all at
    once, and a frozen problem keeps its bits (the first problem to freeze has the
    same bits after a solve that stops 25 iterations later as after the full one).
    The seeds were picked on the CPU: over all termination tests of every
    problem, the restatement's residuals stay at least 6 % (relative) away
    from the threshold that would change the test's outcome, and every adaptive
    estimate at least 7 % away from the rule's limits 5 and 1/5; the
    assertions on `margin` / `est_margin` below repeat that check at 1 %."""
    bt = _batch(name, False)
    ref = _ref(name, "serial", False, rho0, adaptive, False)
    for (_, _, _, oi) in ref:
        assert oi["converged"] and oi["margin"] > 0.01 and oi["est_margin"] > 0.01, oi
        assert (oi["rho_updates"] >= 1) == adaptive
    bs = _handle(bt, "serial", True)
    w, y, z, info = _solve(bs, bt, rho0, adaptive_rho=adaptive, **CONV)
    assert info["converged"].all()
    assert len(set(info["iters"].tolist())) > 1, "vacuous: all problems converged together"
    for b, (ow, oy, oz, oi) in enumerate(ref):
        assert info["iters"][b] == oi["iters"], (b, info["iters"][b], oi["iters"])
        errs = (rel_err(w[b], ow), rel_err(y[b], oy), rel_err(z[b], oz), rel_err(info["rho"][b], oi["rho"]))
        print(name, rho0, adaptive, b, "iters", info["iters"][b], "rel err w y z rho", errs)
        assert max(errs) < 1e-6, (b, errs)
    # the first problem to freeze: however long the rest of the batch goes on, its bits stay
    first = int(np.argmin(info["iters"]))
    cap = int(info["iters"][first]) + 25
    assert cap <= info["iterations"]  # (the batch does not converge at one test)
    w2, y2, z2, info2 = _solve(bs, bt, rho0, adaptive_rho=adaptive, **dict(CONV, max_iter=cap))
    bs.close()
    assert info2["iterations"] == cap and info2["iters"][first] == info["iters"][first]
    assert np.array_equal(w2[first], w[first]) and np.array_equal(y2[first], y[first])
    assert np.array_equal(z2[first], z[first])


# ---------------------------------------------------------------------------
# 4. cones off is the old code
# ---------------------------------------------------------------------------
def _box_batch():
    """6/3, N = 20: three box rows on u per stage, one on x_N."""
    n, m, N = 6, 3, 20
    lay = [[("box", range(m), 0.2)] for _ in range(N)] + [[("box", (0,), 1.0)]]
    return R.build_batch(n, m, N, lay, (0, 2, 5), warm_seed=4)


def test_no_cones_set_cleared_or_refused_give_the_same_bits():
    """A handle never given cones, one given cones and then cleared, and one
    given a list that covers no row of its stage (a cone needs two rows of its
    stage, so such a list leaves the stage's rows: set_cones refuses it and
    leaves the handle as it was) return identical bits."""
    from pdplqr import PdplqrError

    bt = _box_batch()
    st = dict(max_iter=60, check_every=10, eps_abs=1e-7, eps_rel=1e-7)
    res = []
    for mode in ("never", "cleared", "refused"):
        bs = _handle(bt, cones=None)
        if mode == "cleared":
            bs.set_cones([(0, 0, 3), (5, 1, 2)])
            bs.set_cones([])
        elif mode == "refused":
            with pytest.raises(PdplqrError) as e:
                bs.set_cones([(0, 3, 2)])
            assert e.value.code == -1
        res.append(_solve(bs, bt, 10.0, **st))
        bs.close()
    for (w, y, z, info) in res[1:]:
        assert np.array_equal(w, res[0][0]) and np.array_equal(y, res[0][1]) and np.array_equal(z, res[0][2])
        assert np.array_equal(info["iters"], res[0][3]["iters"])


_CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [{root!r}, {root!r} + "/pdp-lqr_amd", {root!r} + "/tests"]
import admm_cone_ref as R
from pdplqr import BatchedLQRSolver

n, m, N = 12, 4, 8
lay = [[("box", range(m), 0.2)] for _ in range(N)] + [[]]
bt = R.build_batch(n, m, N, lay, (0, 1, 2), warm_seed=6)
lb, ub = bt["lb"].copy(), bt["ub"].copy()
lb[:, :4] = np.array([-0.3, 0.0, 0.0, 0.0])
ub[:, :4] = lb[:, :4]
out = []
for cones in (None, [(0, 0, 4)]):
    bs = BatchedLQRSolver(n, m, N, 3, keep_factors=True, ncs=bt["ncs"])
    bs.set_model(bt["E"], bt["c"], bt["H"], bt["h"], bt["D"])
    if cones:
        bs.set_cones(cones)
    w, y, z = bt["ws"].copy(), bt["ys"].copy(), bt["zs"].copy()
    bs.admm_solve(bt["x0"], lb, ub, np.full(lb.shape, 10.0), w, y, z, max_iter=1)
    bs.close()
    out.append((w, y, z))
(w0, y0, z0), (w1, y1, z1) = out
assert np.array_equal(w0, w1), "w"
assert np.array_equal(y0[:, 4:], y1[:, 4:]), "y of the other stages"
assert np.array_equal(z0[:, 4:], z1[:, 4:]), "z of the other stages"
assert not np.array_equal(z0[:, :4], z1[:, :4]), "vacuous: the cone changed nothing on stage 0"
print("child ok")
"""


def test_cones_on_stage_0_leave_the_other_stages_bits():
    """PDPLQR_NO_ADMM_FUSE=1, a fresh process, 12/4 with four box rows per stage
    (the layout whose update otherwise runs inside the streamed backward): after
    one iteration a handle with one cone on stage 0 reproduces the never-set
    handle's bits on w and on every other stage's rows of y and z -- the cone
    kernel's box rows are k_admm_update's arithmetic."""
    env = dict(os.environ, PDPLQR_NO_ADMM_FUSE="1")
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT)], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------------------
# 5. device buffers equal host buffers
# ---------------------------------------------------------------------------
def test_device_buffers_equal_host_buffers():
    import torch

    bt = _batch("ragged", True)
    st = dict(max_iter=60, check_every=10, eps_abs=1e-7, eps_rel=1e-7)
    bs = _handle(bt)
    hw, hy, hz, hi = _solve(bs, bt, 10.0, **st)
    bs.close()
    dev = torch.device("cuda", 0)
    T = {k: torch.from_numpy(bt[k]).to(dev) for k in "E c H h D x0 lb ub ws ys zs".split()}
    rho = torch.full_like(T["lb"], 10.0)
    bs = _handle(bt, tensors=T)
    di = bs.admm_solve(T["x0"], T["lb"], T["ub"], rho, T["ws"], T["ys"], T["zs"], **st)
    torch.cuda.synchronize()
    bs.close()
    assert np.array_equal(T["ws"].cpu().numpy(), hw) and np.array_equal(T["ys"].cpu().numpy(), hy)
    assert np.array_equal(T["zs"].cpu().numpy(), hz) and np.array_equal(di["iters"], hi["iters"])


# ---------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------
INVALID, UNSUPPORTED = -1, -5


def _raises(code, fn, *a, **k):
    from pdplqr import PdplqrError

    with pytest.raises(PdplqrError) as e:
        fn(*a, **k)
    assert e.value.code == code, e.value


def test_set_cones_refusals():
    from pdplqr import BatchedLQRSolver

    bt = _batch("ragged", True)
    n, m, N = 6, 3, 7
    bs = _handle(bt)
    for bad in ([(0, 2, 1)],              # cone_dim < 2
                [(N + 1, 0, 2)], [(-1, 0, 2)],  # a stage outside 0..N
                [(1, 0, 2)],              # a stage without rows
                [(0, 3, 4)], [(0, -1, 2)],  # leaves its stage's rows
                [(0, 0, 3), (0, 2, 2)],   # overlap
                [(2, 6, 4), (2, 1, 3)], [(3, 0, 10), (0, 2, 4)]):  # unsorted: row, stage
        _raises(INVALID, bs.set_cones, bad)
    # a refused call leaves the previous cones in place: the solve still is the cone solve
    ref = _ref("ragged", "serial", True, 10.0, True, True)
    w, y, z, _ = _solve(bs, bt, 10.0, **FIXED)
    assert rel_err(z[0], ref[0][2]) < TOL
    bs.close()
    # cone_dim > the stage's variables + 1 (the terminal stage: nx + 1)
    ncs = [12] * N + [9]
    bs = BatchedLQRSolver(n, m, N, 2, ncs=ncs)
    _raises(UNSUPPORTED, bs.set_cones, [(0, 0, 11)])
    _raises(UNSUPPORTED, bs.set_cones, [(N, 0, 8)])
    bs.set_cones([(0, 0, 10), (N, 0, 7)])
    bs.close()
    bs = BatchedLQRSolver(n, m, N, 2, solver="kkt", ncs=ncs)
    _raises(UNSUPPORTED, bs.set_cones, [(0, 0, 3)])
    bs.close()
    bs = BatchedLQRSolver(n, m, N, 2, solver="parallel", num_segments=4, ncs=ncs, devices=[0])  # non-NULL `devices`
    _raises(UNSUPPORTED, bs.set_cones, [(0, 0, 3)])
    bs.close()
    bs = BatchedLQRSolver(40, 25, 2, 1, ncs=[3, 3, 0])  # nx + nu = 65
    _raises(UNSUPPORTED, bs.set_cones, [(0, 0, 3)])
    bs.close()


def test_solve_refusals_leave_the_iterates_untouched():
    bt = _batch("ragged", True)
    bs = _handle(bt)
    q, d = R.cone_rows(bt["ncs"], bt["cones"])[1]
    rho = np.full(bt["lb"].shape, 10.0)

    def attempt(code, lb=bt["lb"], ub=bt["ub"], rho=rho, **kw):
        w, y, z = bt["ws"].copy(), bt["ys"].copy(), bt["zs"].copy()
        _raises(code, bs.admm_solve, bt["x0"], lb, ub, rho, w, y, z, **FIXED, **kw)
        assert np.array_equal(w, bt["ws"]) and np.array_equal(y, bt["ys"]) and np.array_equal(z, bt["zs"])

    r2 = rho.copy()
    r2[1, q + 1] = 11.0  # rho not constant within a cone
    attempt(INVALID, rho=r2)
    for val in (np.inf, -np.inf, 1e20, -1e20):  # a cone row's lb not finite
        l2, u2 = bt["lb"].copy(), bt["ub"].copy()
        l2[2, q] = val
        u2[2, q] = max(val, u2[2, q])  # (lb <= ub still holds: the cone check is the one that refuses)
        attempt(INVALID, lb=l2, ub=u2)
    # rho differing between cones, and on box rows, is fine
    r3 = rho.copy()
    r3[:, q:q + d] = 7.0
    w, y, z = bt["ws"].copy(), bt["ys"].copy(), bt["zs"].copy()
    bs.admm_solve(bt["x0"], bt["lb"], bt["ub"], r3, w, y, z, **FIXED)
    # polish, detection: box statements
    bs.set_polish(True)
    attempt(UNSUPPORTED)
    bs.set_polish(False)
    attempt(UNSUPPORTED, detect_infeasibility=True)
    # the evaluators would read cone rows as boxes
    _raises(UNSUPPORTED, bs.kkt_residuals, bt["x0"], bt["lb"], bt["ub"], bt["ws"], bt["ys"])
    _raises(UNSUPPORTED, bs.check_certificates, bt["x0"], bt["lb"], bt["ub"], bt["ys"], bt["ws"])
    _raises(UNSUPPORTED, bs.admm_adjoint, bt["ws"])
    # cleared: they serve the handle again
    bs.set_cones([])
    assert bs.kkt_residuals(bt["x0"], bt["lb"], bt["ub"], bt["ws"], bt["ys"]).shape == (len(bt["pms"]), 4)
    bs.close()
