"""The ADMM polish on the GPU (csrc/kernels_polish.hip, csrc/admm.hip; DESIGN.md
section 5.8) against the numpy restatement tests/admm_polish_ref.py:

* the KKT measures alone (pdplqr_admm_kkt_residuals): within 1e-9 relative of
  kkt_measures at the five shapes of tests/test_gpu_infeas.py's PARITY;
* the loop: the table of tests/test_admm_polish_cpu.py.  Accepted problems land
  on the exact solution of their active set; rejected and unsolved ones keep
  their ADMM iterate bit for bit;
* off means off, arguments and limits, BoxLQRLayer(polish=True).

The bound on the polished w.  The reference polish's own error against the exact
active-set solution (a dense solve, no regularisation) is 5e-14 .. 1e-12 over
the table; the device may be 1000 times that far away: it eliminates the
1/delta penalty through the stage recursion of the Riccati factorisation, not
through a dense inverse.  Per case the bound is 1000 * max(reference error of the
case, 5e-14) -- the floor is the low end of that range, so that a case the dense
solve happens to get to 3e-15 is not held to 3e-12.
Every input is valid data.
"""
import numpy as np
import pytest

import admm_infeas_ref as ref
import admm_polish_ref as pol

pytestmark = pytest.mark.gpu

REF_ERR_FLOOR = 5e-14


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from pdplqr import device_count

    assert device_count() > 0, "no HIP device visible: GPU tests must run on an MI355X"


def _arrays(pms):
    return {k: np.ascontiguousarray(np.stack([getattr(p, k) for p in pms])) for k in "E c H h D".split()}


def _solver(pms, solver="serial", keep=True, **kw):
    from pdplqr import BatchedLQRSolver

    p = pms[0]
    if solver == "parallel":
        kw.update(num_segments=4, condensed="CHOLESKY")
    bs = BatchedLQRSolver(p.n, p.m, p.N, len(pms), solver=solver, keep_factors=keep, ncs=[int(x) for x in p.ncs], **kw)
    A = _arrays(pms)
    bs.set_model(A["E"], A["c"], A["H"], A["h"], A["D"] if A["D"].size else None)
    return bs


def _close(a, b, tol):
    return abs(a - b) <= tol * max(abs(a), abs(b))


def _code(fn, *a):
    from pdplqr._lib import PdplqrError

    with pytest.raises(PdplqrError) as e:
        fn(*a)
    return e.value.code


# ---------------------------------------------------------------------------
# the evaluator alone
# ---------------------------------------------------------------------------
PARITY = [
    (3, 2, 6, [2, 0, 3, 1, 0, 2, 1]),                 # ragged, rows at the terminal
    (12, 4, 9, [4] * 9 + [0]),                        # the uniform layout (uni = 4)
    (6, 3, 65, [k % 7 for k in range(65)] + [2]),     # more stages than one block pass; up to 6 rows
    (24, 8, 5, [3, 5, 0, 6, 2, 4]),                   # 32 lanes per stage
    (40, 24, 3, [4, 7, 2, 3]),                        # s = 64: the instance that keeps no column
]


def _parity_inputs(n, m, N, ncs):
    g = np.random.default_rng(n * 1000 + N + 1)
    pms = [ref.random_packed(n, m, N, ncs, 50 + b, radius=0.95) for b in range(3)]
    ny, nw = int(sum(ncs)), N * (n + m) + n
    x0 = g.standard_normal((3, n))
    w, y = g.standard_normal((3, nw)), g.standard_normal((3, ny))
    lb, ub = -1.0 - g.random((3, ny)), 1.0 + g.random((3, ny))
    ub[g.random((3, ny)) < 0.3] = 1e20
    lb[g.random((3, ny)) < 0.3] = -1e20
    w[2, m:n + m] = x0[2]  # problem 2 starts at x0: its dynamics residual comes from the stages alone
    return pms, x0, lb, ub, w, y


@pytest.mark.parametrize("n,m,N,ncs", PARITY, ids=lambda v: str(v) if isinstance(v, int) else "ncs")
def test_kkt_residuals_match_numpy(n, m, N, ncs):
    pms, x0, lb, ub, w, y = _parity_inputs(n, m, N, ncs)
    bs = _solver(pms)
    meas = bs.kkt_residuals(x0, lb, ub, w, y)
    again = bs.kkt_residuals(x0, lb, ub, w, y)
    bs.close()
    assert meas.shape == (3, 4) and np.array_equal(meas, again)
    for b in range(3):
        want = pol.kkt_measures(pms[b], x0[b], lb[b], ub[b], w[b], y[b])
        print((n, m, N), b, "device", meas[b], "numpy", want)
        for i in range(4):
            assert _close(meas[b, i], want[i], 1e-9), (b, i, meas[b, i], want[i])
        assert want[pol.K_ROW] > 0 and want[pol.K_GRAD] > 0


def test_kkt_residuals_device_buffers_same_bits():
    import torch

    n, m, N, ncs = PARITY[0]
    pms, x0, lb, ub, w, y = _parity_inputs(n, m, N, ncs)
    bs = _solver(pms)
    meas = bs.kkt_residuals(x0, lb, ub, w, y)
    dmeas = bs.kkt_residuals(*[torch.tensor(a, device="cuda") for a in (x0, lb, ub, w, y)])
    bs.close()
    assert np.array_equal(dmeas.cpu().numpy(), meas)


# ---------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------
LOOP = dict(sigma=1e-6, alpha=1.6, max_iter=4000, check_every=5, eps_rel=0.0, adaptive_rho=False)
_REF = {}


def _reference(n, m, N, kind, seed, margin, tr, eps):
    """The problem, the numpy loop's outcome, its polish and measures (computed once)."""
    key = (n, m, N, kind, seed, margin, tr, eps)
    if key not in _REF:
        pm, x0, lb, ub = ref.box_problem(n, m, N, kind, seed, margin, terminal_row=tr)
        r = ref.admm_loop(pm, x0, lb, ub, np.ones(lb.size), sigma=1e-6, alpha=1.6, max_iter=4000, check_every=5,
                          eps_abs=eps, eps_rel=0.0, detect=(kind != "feasible"))
        out = dict(pm=pm, x0=x0, lb=lb, ub=ub, admm=r)
        if r["status"] == 1:
            p = pol.polish(pm, x0, lb, ub, r["w"], r["y"], r["z"])
            out.update(polish=p, before=pol.kkt_measures(pm, x0, lb, ub, r["w"], r["y"]),
                       after=pol.kkt_measures(pm, x0, lb, ub, p["w"], p["y"]),
                       margin=pol.classification_margin(r["y"], r["z"], lb, ub),
                       exact=pol.active_set_solution(pm, x0, p["act"], p["b"])[0])
            out["accept"] = pol.accept(out["before"], out["after"])
        _REF[key] = out
    return _REF[key]


def _run(bs, refs, eps, polish, detect=False):
    x0, lb, ub = (np.ascontiguousarray(np.stack([c[k] for c in refs])) for k in ("x0", "lb", "ub"))
    B, nw = len(refs), refs[0]["pm"].h.size
    w, y, z = np.zeros((B, nw)), np.zeros(lb.shape), np.zeros(lb.shape)
    bs.set_polish(polish)
    info = bs.admm_solve(x0, lb, ub, np.ones(lb.shape), w, y, z, eps_abs=eps, detect_infeasibility=detect, **LOOP)
    return w, y, z, info


ACCEPTED = [(3, 2, 6, 1, .05, True), (4, 2, 9, 2, .05, True), (12, 4, 8, 3, .05, True), (24, 8, 5, 7, .05, True),
            (6, 3, 20, 8, .05, True), (12, 4, 8, 3, .05, False)]  # the last: the uniform layout of the fused update


@pytest.mark.parametrize("solver,keep", [("serial", True), ("serial", False), ("parallel", True)])
@pytest.mark.parametrize("case", ACCEPTED, ids=str)
def test_loop_accepted(case, solver, keep):
    n, m, N, seed, margin, tr = case
    c = _reference(n, m, N, "feasible", seed, margin, tr, 1e-3)
    assert c["admm"]["status"] == 1 and c["accept"]  # the reference itself
    assert c["margin"] > 1e-6, c["margin"]           # device rounding cannot flip a row
    bs = _solver([c["pm"]], solver, keep)
    w, y, z, info = _run(bs, [c], 1e-3, True)
    pi = bs.polish_info()
    bs.close()
    err_ref = np.max(np.abs(c["polish"]["w"] - c["exact"]))
    err_dev = np.max(np.abs(w[0] - c["exact"]))
    err_admm = np.max(np.abs(c["admm"]["w"] - c["exact"]))
    print(case, solver, keep, "status", pi["status"], "n_active", pi["n_active"], "iters", info["iters"], "numpy",
          c["admm"]["iters"], "measures", pi["measures"][0], "numpy", c["before"], c["after"])
    print(case, solver, keep, "w error: device", err_dev, "reference", err_ref, "ADMM iterate", err_admm)
    assert list(pi["status"]) == [1] and list(info["polish_status"]) == [1]
    assert info["status"][0] == 1 and info["iters"][0] == c["admm"]["iters"]
    assert pi["n_active"][0] == c["polish"]["n_active"]
    for i in range(4):  # the ADMM iterate's measures: the iterates match to rounding
        assert _close(pi["measures"][0, i], c["before"][i], 1e-6) or abs(pi["measures"][0, i] - c["before"][i]) < 1e-12
    assert err_dev <= 1000 * max(err_ref, REF_ERR_FLOOR), (err_dev, err_ref)
    assert err_dev <= 1e-3 * err_admm, (err_dev, err_admm)
    # y and z of the polished point: z = clamp(D w), y zero off the active set
    assert not y[0][~c["polish"]["act"]].any()
    assert np.max(np.abs(z[0] - np.clip(ref.rows_of(c["pm"], w[0]), c["lb"], c["ub"]))) < 1e-13
    assert np.max(np.abs(y[0] - c["polish"]["y"])) <= 1e-6 * np.max(np.abs(c["polish"]["y"]))


def _mixed():
    return [_reference(5, 3, 7, "feasible", 6, .1, True, 1e-2), _reference(5, 3, 7, "feasible", 4, .1, True, 1e-2),
            _reference(5, 3, 7, "contradictory", 3, .05, True, 1e-2)]


@pytest.mark.parametrize("solver,keep", [("serial", True), ("serial", False), ("parallel", True)])
def test_loop_mixed_batch(solver, keep):
    cs = _mixed()
    assert [c["admm"]["status"] for c in cs] == [1, 1, 2]  # the reference itself
    assert cs[0]["accept"] and not cs[1]["accept"]
    assert cs[1]["after"][pol.K_ROW] > 10 * cs[1]["before"][pol.K_ROW]  # rejected by the row residual, clearly
    assert min(cs[0]["margin"], cs[1]["margin"]) > 1e-6
    bs = _solver([c["pm"] for c in cs], solver, keep)
    w1, y1, z1, i1 = _run(bs, cs, 1e-2, True, detect=True)
    pi = bs.polish_info()
    w0, y0, z0, i0 = _run(bs, cs, 1e-2, False, detect=True)
    assert "polish_status" not in i0 and _code(bs.polish_info) == -4
    bs.close()
    print(solver, keep, "polish", pi["status"], "n_active", pi["n_active"], "admm", i1["status"], "measures",
          pi["measures"])
    assert list(pi["status"]) == [1, 2, 0]
    assert list(i1["status"]) == [1, 1, 2] and np.array_equal(i1["status"], i0["status"])
    assert np.array_equal(i1["iters"], i0["iters"])
    for b in (1, 2):  # rejected, not attempted: the ADMM iterate, bit for bit
        assert np.array_equal(w1[b], w0[b]) and np.array_equal(y1[b], y0[b]) and np.array_equal(z1[b], z0[b])
    assert not np.array_equal(w1[0], w0[0])
    assert np.max(np.abs(w1[0] - cs[0]["exact"])) <= 1000 * max(np.max(np.abs(cs[0]["polish"]["w"] - cs[0]["exact"])),
                                                               REF_ERR_FLOOR)
    assert pi["n_active"][1] == cs[1]["polish"]["n_active"]
    assert _close(pi["measures"][1, 4], cs[1]["after"][pol.K_ROW], 1e-6)


def test_loop_rejected_alone():
    c = _reference(3, 2, 6, "feasible", 5, .02, True, 1e-3)
    assert c["admm"]["status"] == 1 and not c["accept"] and c["margin"] > 1e-6
    bs = _solver([c["pm"]])
    w1, y1, z1, i1 = _run(bs, [c], 1e-3, True)
    pi = bs.polish_info()
    w0, y0, z0, i0 = _run(bs, [c], 1e-3, False)
    bs.close()
    print("polish", pi["status"], pi["n_active"], pi["measures"], "numpy", c["before"], c["after"])
    assert list(pi["status"]) == [2] and pi["n_active"][0] == c["polish"]["n_active"]
    assert np.array_equal(w1, w0) and np.array_equal(y1, y0) and np.array_equal(z1, z0)


def test_off_means_off():
    cs = [_reference(3, 2, 6, "feasible", 1, .05, True, 1e-3), _reference(3, 2, 6, "feasible", 5, .02, True, 1e-3)]
    bs = _solver([c["pm"] for c in cs])
    bs.set_polish(True, 1e-6, 3)
    bs.set_polish(False)
    a = _run(bs, cs, 1e-3, False)
    assert _code(bs.polish_info) == -4 and "polish_status" not in a[3]
    bs.close()
    fresh = _solver([c["pm"] for c in cs])
    x0, lb, ub = (np.ascontiguousarray(np.stack([c[k] for c in cs])) for k in ("x0", "lb", "ub"))
    w, y, z = np.zeros_like(a[0]), np.zeros_like(a[1]), np.zeros_like(a[2])
    info = fresh.admm_solve(x0, lb, ub, np.ones(lb.shape), w, y, z, eps_abs=1e-3, **LOOP)  # set_polish never called
    fresh.close()
    assert np.array_equal(a[0], w) and np.array_equal(a[1], y) and np.array_equal(a[2], z)
    assert np.array_equal(a[3]["iters"], info["iters"]) and np.array_equal(a[3]["prim_res"], info["prim_res"])


def test_refine_iter_zero_is_one_solve():
    """refine_iter = 0 is the plain regularised solve: accepted, and not as close as with three steps."""
    c = _reference(3, 2, 6, "feasible", 1, .05, True, 1e-3)
    errs = []
    for it in (0, 3):
        bs = _solver([c["pm"]])
        bs.set_polish(True, 1e-6, it)
        x0, lb, ub = c["x0"][None], c["lb"][None], c["ub"][None]
        w, y, z = np.zeros((1, c["pm"].h.size)), np.zeros(lb.shape), np.zeros(lb.shape)
        info = bs.admm_solve(x0, lb, ub, np.ones(lb.shape), w, y, z, eps_abs=1e-3, **LOOP)
        bs.close()
        assert list(info["polish_status"]) == [1]
        errs.append(np.max(np.abs(w[0] - c["exact"])))
    print("w error with refine_iter 0 / 3:", errs)
    assert errs[1] < errs[0] < np.max(np.abs(c["admm"]["w"] - c["exact"]))


# ---------------------------------------------------------------------------
# arguments and limits
# ---------------------------------------------------------------------------
def test_unsupported_and_argument_checks():
    from pdplqr import BatchedLQRSolver

    kkt = BatchedLQRSolver(4, 2, 6, 1, solver="kkt", ncs=[2] * 6 + [0])
    assert _code(kkt.set_polish, True) == -5
    kkt.set_polish(False)  # switching off is always fine
    z = np.zeros
    assert _code(kkt.kkt_residuals, z((1, 4)), z((1, 12)), z((1, 12)), z((1, 40)), z((1, 12))) == -5
    kkt.close()
    md = BatchedLQRSolver(4, 2, 8, 1, solver="parallel", num_segments=2, ncs=[2] * 8 + [0], devices=[0])
    assert _code(md.set_polish, True) == -5
    md.close()
    xl = BatchedLQRSolver(60, 8, 2, 1, ncs=[1, 1, 0])  # nx + nu = 68
    assert _code(xl.set_polish, True) == -5
    xl.close()
    bs = BatchedLQRSolver(4, 2, 6, 1, ncs=[2] * 6 + [0])
    assert _code(bs.set_polish, True, 0.0, 3) == -1
    assert _code(bs.set_polish, True, -1e-6, 3) == -1
    assert _code(bs.set_polish, True, float("nan"), 3) == -1
    assert _code(bs.set_polish, True, 1e-6, -1) == -1
    bs.set_polish(True, 1e-6, 0)
    assert _code(bs.polish_info) == -4  # before any admm_solve
    assert _code(bs.kkt_residuals, z((1, 4)), z((1, 12)), z((1, 12)), z((1, 40)), z((1, 12))) == -4  # before set_model
    bs.close()


# ---------------------------------------------------------------------------
# BoxLQRLayer
# ---------------------------------------------------------------------------
def test_layer_polish_reaches_the_tight_solution():
    """The layer's CPU-checked (3, 2, 6) problems (tests/test_gpu_box_layer.py): with
    polish, eps = 1e-4 returns the w the unpolished layer returns at eps = 1e-9,
    and gradients within that test's bound."""
    import torch

    import adjoint_ref
    import adjoint_rows_ref as rr
    from pdplqr import BoxLQRLayer
    from test_adjoint_rows_cpu import BOX_CASES, LAYER

    n, m, N, seeds = BOX_CASES[0]
    bcs = [rr.box_case(n, m, N, seed) for seed in seeds]
    ncs = bcs[0]["dims"][3]
    gws = torch.tensor(np.stack([bc["gws"] for bc in bcs]), device="cuda")
    res = {}
    for polish, eps in ((False, LAYER["eps_abs"]), (True, 1e-4)):
        layer = BoxLQRLayer(n, m, N, len(seeds), ncs, rho=10.0, sigma=1e-6, alpha=1.6, eps=eps,
                            max_iter=LAYER["max_iter"], adj_tol=LAYER["adj_tol"], adj_max_iter=LAYER["adj_max_iter"],
                            check_every=LAYER["check_every"], polish=polish)
        leaves = [torch.tensor(np.stack([bc[k] for bc in bcs]), device="cuda", requires_grad=True) for k in rr.BOX_KEYS]
        ws = layer(*leaves)
        info = layer.admm_info
        assert info["converged"].all()
        if polish:
            assert list(info["polish_status"]) == [1] * len(seeds)
        else:
            assert "polish_status" not in info
        (gws * ws).sum().backward()
        res[polish] = (ws.detach().cpu().numpy(), [t.grad.cpu().numpy() for t in leaves], info["iters"].copy())
        layer.close()
    print("admm iters: eps 1e-9", res[False][2], "eps 1e-4 + polish", res[True][2])
    assert (res[True][2] < res[False][2]).all()
    dw = np.max(np.abs(res[True][0] - res[False][0]))
    print("polished (eps 1e-4) against unpolished (eps 1e-9) w:", dw)
    assert dw <= 1000 * REF_ERR_FLOOR
    tol = 10 * rr.LAYER_CPU_ERR[(n, m, N)]
    worst = 0.0
    for b, bc in enumerate(bcs):
        assert adjoint_ref.rel(res[True][0][b], bc["ws"]) < 10 * rr.LAYER_CPU_WS_ERR[(n, m, N)]
        for k, gr in zip(rr.BOX_KEYS, res[True][1]):
            worst = max(worst, adjoint_ref.rel(gr[b].ravel(), bc["grads"][k]))
    print("worst gradient error with polish:", worst, "bound", tol)
    assert worst < tol, (worst, tol)
