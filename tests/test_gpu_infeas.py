"""Infeasibility detection of the ADMM loop on the GPU (csrc/kernels_infeas.hip,
csrc/admm.hip) against the numpy restatement
tests/admm_infeas_ref.py:

* the certificate kernels alone (pdplqr_admm_check_certificates): every
  measure within 1e-9 relative of certificate_measures, verdicts equal where the
  reference is a factor 2 away from its thresholds;
* the loop: problems infeasible by construction are certified at the
  reference's iteration, their neighbours (feasible by construction) are
  untouched bit for bit, the device's certificates pass the numpy checker;
* unsupported handles, call order, adaptive rho, BoxLQRLayer.
Every input is valid data.
"""
import numpy as np
import pytest

import admm_infeas_ref as ref

pytestmark = pytest.mark.gpu

EPS = 1e-4


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


def _close(a, b, tol=1e-9):
    return abs(a - b) <= tol * max(abs(a), abs(b))


# ---------------------------------------------------------------------------
# the kernels alone
# ---------------------------------------------------------------------------
PARITY = [
    (3, 2, 6, [2, 0, 3, 1, 0, 2, 1]),                 # ragged, rows at the terminal
    (12, 4, 9, [4] * 9 + [0]),                        # the uniform layout (uni = 4)
    (6, 3, 65, [k % 7 for k in range(65)] + [2]),     # more stages than one block pass; up to 6 rows
    (24, 8, 5, [3, 5, 0, 6, 2, 4]),                   # 32 lanes per stage
    (40, 24, 3, [4, 7, 2, 3]),                        # s = 64: the single-buffered primal instance
]


def _parity_inputs(n, m, N, ncs):
    g = np.random.default_rng(n * 1000 + N)
    pms = [ref.random_packed(n, m, N, ncs, 50 + b, radius=0.95) for b in range(3)]
    ny, nw = int(sum(ncs)), N * (n + m) + n
    x0 = g.standard_normal((3, n))
    dy, dw = g.standard_normal((3, ny)), g.standard_normal((3, nw))
    dy[2] = 0.0  # |dy| = 0: never a certificate
    lb, ub = -1.0 - g.random((3, ny)), 1.0 + g.random((3, ny))
    # problem 0: infinite bounds at random rows; problem 1: only where dy has the admissible sign
    inf_u, inf_l = g.random((3, ny)) < 0.3, g.random((3, ny)) < 0.3
    inf_u[1] &= dy[1] < 0
    inf_l[1] &= dy[1] > 0
    ub[inf_u], lb[inf_l] = 1e20, -1e20
    return pms, x0, lb, ub, dy, dw


@pytest.mark.parametrize("n,m,N,ncs", PARITY, ids=lambda v: str(v) if isinstance(v, int) else "ncs")
def test_check_certificates_matches_numpy(n, m, N, ncs):
    pms, x0, lb, ub, dy, dw = _parity_inputs(n, m, N, ncs)
    bs = _solver(pms)
    meas, verdict = bs.check_certificates(x0, lb, ub, dy, dw, EPS, EPS)
    only_p, vp = bs.check_certificates(x0, lb, ub, dy, None, EPS, EPS)
    only_d, vd = bs.check_certificates(x0, lb, ub, None, dw, EPS, EPS)
    bs.close()
    # a value does not depend on which half was asked for; a skipped half is zero
    assert np.array_equal(only_p[:, :4], meas[:, :4]) and not only_p[:, 4:].any()
    assert np.array_equal(only_d[:, 4:], meas[:, 4:]) and not only_d[:, :4].any()
    assert np.array_equal(vp | vd, verdict)
    flags = []
    for b in range(3):
        want, wv = ref.certificate_measures(pms[b], x0[b], lb[b], ub[b], dy[b], dw[b], EPS, EPS)
        print((n, m, N), b, "device", meas[b], "numpy", want)
        for i in range(8):
            assert _close(meas[b, i], want[i]), (b, i, meas[b, i], want[i])
        assert verdict[b] == wv
        flags.append(want[ref.M_INFFLAG])
    assert flags[0] == 1.0 and flags[1] == 0.0 and not meas[2, :4].any()


def test_check_certificates_device_buffers_same_bits():
    import torch

    n, m, N, ncs = PARITY[0]
    pms, x0, lb, ub, dy, dw = _parity_inputs(n, m, N, ncs)
    bs = _solver(pms)
    meas, verdict = bs.check_certificates(x0, lb, ub, dy, dw, EPS, EPS)
    dev = [torch.tensor(a, device="cuda") for a in (x0, lb, ub, dy, dw)]
    dmeas, dverdict = bs.check_certificates(*dev, EPS, EPS)
    bs.close()
    assert np.array_equal(dmeas.cpu().numpy(), meas) and np.array_equal(dverdict.cpu().numpy(), verdict)


def _away_from_thresholds(meas, primal):
    """Every compared measure of the reference is a factor 2 away from its threshold."""
    if primal:
        thr = EPS * meas[ref.M_DY]
        pairs = [(meas[ref.M_G], thr), (-meas[ref.M_SUPPORT], thr)]
    else:
        thr = EPS * meas[ref.M_DW]
        pairs = [(meas[ref.M_HDW], thr), (-meas[ref.M_HTDW], thr), (meas[ref.M_VIOL], thr)]
    return all(v <= t / 2 or v >= 2 * t for v, t in pairs)


@pytest.mark.parametrize("n,m,N", [(3, 2, 6), (12, 4, 8)])
def test_verdict_primal_true_certificate_plus_noise(n, m, N):
    """dy of the numpy loop's certificate for the contradictory-rows problem:
    as it is and with 1e-7 relative noise it certifies, with 1e-2 noise the
    reduced gradient is far above the threshold."""
    pm, x0, lb, ub = ref.box_problem(n, m, N, "contradictory", 2)
    r = ref.admm_loop(pm, x0, lb, ub, np.full(lb.size, 10.0), eps_abs=1e-6, eps_rel=0.0, max_iter=1000)
    assert r["status"] == 2
    g = np.random.default_rng(5)
    scale = np.max(np.abs(r["dy"]))
    dys = np.stack([r["dy"] + lvl * scale * g.standard_normal(lb.size) for lvl in (0.0, 1e-7, 1e-2)])
    bs = _solver([pm] * 3)
    rep = lambda a: np.ascontiguousarray(np.stack([a] * 3))  # noqa: E731
    meas, verdict = bs.check_certificates(rep(x0), rep(lb), rep(ub), dys, None, EPS, EPS)
    bs.close()
    want = []
    for b in range(3):
        wm, wv = ref.certificate_measures(pm, x0, lb, ub, dys[b], None, EPS, EPS)
        assert _away_from_thresholds(wm, True), wm
        want.append(wv)
    assert want == [1, 1, 0] and list(verdict) == want


@pytest.mark.parametrize("n,m,N", [(2, 1, 5), (6, 3, 8)])
def test_verdict_dual_true_certificate_plus_noise(n, m, N):
    pm, x0, lb, ub = ref.unbounded_problem(n, m, N, 1)
    r = ref.admm_loop(pm, x0, lb, ub, np.full(lb.size, 10.0), eps_abs=1e-6, eps_rel=0.0, max_iter=200)
    assert r["status"] == 3
    g = np.random.default_rng(6)
    scale = np.max(np.abs(r["dw"]))
    dws = np.stack([r["dw"] + lvl * scale * g.standard_normal(r["dw"].size) for lvl in (0.0, 1e-7, 1e-2)])
    bs = _solver([pm] * 3)
    rep = lambda a: np.ascontiguousarray(np.stack([a] * 3))  # noqa: E731
    meas, verdict = bs.check_certificates(rep(x0), rep(lb), rep(ub), None, dws, EPS, EPS)
    bs.close()
    want = []
    for b in range(3):
        wm, wv = ref.certificate_measures(pm, x0, lb, ub, None, dws[b], EPS, EPS)
        assert _away_from_thresholds(wm, False), wm
        want.append(wv)
    assert want == [2, 2, 0] and list(verdict) == want


# ---------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------
LOOP = dict(sigma=1e-6, alpha=1.6, max_iter=400, check_every=25, eps_abs=1e-6, eps_rel=0.0, adaptive_rho=False)
KINDS = ["feasible", "contradictory", "feasible", "dynamics", "feasible"]
SEEDS = [1, 2, 3, 2, 4]
_REF = {}


def _mixed(n, m, N):
    """The mixed batch and the numpy loop's outcome per problem (computed once)."""
    if (n, m, N) not in _REF:
        probs = [ref.box_problem(n, m, N, kind, seed) for kind, seed in zip(KINDS, SEEDS)]
        kw = {k: v for k, v in LOOP.items() if k != "adaptive_rho"}
        outs = [ref.admm_loop(pm, x0, lb, ub, np.full(lb.size, 10.0), **kw) for pm, x0, lb, ub in probs]
        _REF[(n, m, N)] = (probs, outs)
    return _REF[(n, m, N)]


def _run(bs, probs, detect, **over):
    x0 = np.ascontiguousarray(np.stack([p[1] for p in probs]))
    lb = np.ascontiguousarray(np.stack([p[2] for p in probs]))
    ub = np.ascontiguousarray(np.stack([p[3] for p in probs]))
    B, nw = len(probs), probs[0][0].h.size
    w, y, z = np.zeros((B, nw)), np.zeros(lb.shape), np.zeros(lb.shape)
    info = bs.admm_solve(x0, lb, ub, np.full(lb.shape, 10.0), w, y, z, detect_infeasibility=detect,
                         eps_prim_inf=EPS, eps_dual_inf=EPS, **{**LOOP, **over})
    return w, y, z, info


def _deciding_test_is_clear(out):
    """The precondition of the iteration-count comparison: at the reference's
    deciding test every primal measure passes by a factor 2, and the test before
    it (if one ran the certificates) fails by a factor 2."""
    hist = out["history"]
    it, ms = hist[-1]
    thr = EPS * ms[ref.M_DY]
    ok = ms[ref.M_G] <= thr / 2 and ms[ref.M_SUPPORT] <= -2 * thr and ms[ref.M_INFFLAG] == 0
    if len(hist) > 1:
        _, pv = hist[-2]
        pthr = EPS * pv[ref.M_DY]
        ok = ok and (pv[ref.M_G] >= 2 * pthr or pv[ref.M_SUPPORT] >= -pthr / 2 or pv[ref.M_INFFLAG] == 1)
    return ok


@pytest.mark.parametrize("solver,keep", [("serial", True), ("serial", False), ("parallel", True)])
@pytest.mark.parametrize("n,m,N", [(3, 2, 6), (12, 4, 8)])
def test_loop_primal_mixed_batch(n, m, N, solver, keep):
    probs, outs = _mixed(n, m, N)
    want = [1, 2, 1, 2, 1]
    assert [o["status"] for o in outs] == want  # the reference itself
    bs = _solver([p[0] for p in probs], solver, keep)
    w1, y1, z1, i1 = _run(bs, probs, True)
    dy, dw = bs.admm_certificate()
    assert np.count_nonzero(bs.status()) == 0
    w0, y0, z0, i0 = _run(bs, probs, False)
    bs.close()
    print((n, m, N, solver, keep), "status", i1["status"], "iters on", i1["iters"], "off", i0["iters"], "numpy",
          [o["iters"] for o in outs])
    assert list(i1["status"]) == want
    assert list(i1["converged"]) == [s == 1 for s in want]
    assert list(i0["status"]) == [1, 0, 1, 0, 1] and np.array_equal(i0["status"], i0["converged"].astype(np.int32))
    for b, s in enumerate(want):
        if s == 1:  # a certified neighbour does not disturb a feasible problem
            assert np.array_equal(w1[b], w0[b]) and np.array_equal(y1[b], y0[b]) and np.array_equal(z1[b], z0[b])
            assert i1["iters"][b] == i0["iters"][b]
            assert not dy[b].any() and not dw[b].any()
        else:
            assert i0["iters"][b] == LOOP["max_iter"]
            assert _deciding_test_is_clear(outs[b]), outs[b]["history"][-2:]
            assert i1["iters"][b] == outs[b]["iters"]
            pm, x0, lb, ub = probs[b]
            meas, verdict = ref.certificate_measures(pm, x0, lb, ub, dy[b], None, EPS, EPS)
            print(b, "device certificate, numpy measures", meas[:4])
            assert verdict == 1


def test_loop_primal_fused_update_path():
    """12/4 with 4 rows per stage and none at the terminal, SERIAL with cached
    factors: the update runs inside the streamed backward (k_nofact_admm_dma).
    Same outcome as with the separate update pass (PDPLQR_NO_ADMM_FUSE), and the
    feasible neighbours keep their bits in either mode."""
    import os

    n, m, N = 12, 4, 8
    probs = [ref.box_problem(n, m, N, kind, seed, terminal_row=False)
             for kind, seed in (("feasible", 1), ("contradictory", 2), ("feasible", 3))]
    kw = {k: v for k, v in LOOP.items() if k != "adaptive_rho"}
    outs = [ref.admm_loop(pm, x0, lb, ub, np.full(lb.size, 10.0), **kw) for pm, x0, lb, ub in probs]
    assert [o["status"] for o in outs] == [1, 2, 1] and _deciding_test_is_clear(outs[1])
    res = {}
    for mode in ("fused", "separate"):
        if mode == "separate":
            os.environ["PDPLQR_NO_ADMM_FUSE"] = "1"
        try:
            bs = _solver([p[0] for p in probs])
            on = _run(bs, probs, True)
            dy, _ = bs.admm_certificate()
            off = _run(bs, probs, False)
            bs.close()
        finally:
            os.environ.pop("PDPLQR_NO_ADMM_FUSE", None)
        print(mode, "status", on[3]["status"], "iters", on[3]["iters"], "numpy", [o["iters"] for o in outs])
        assert list(on[3]["status"]) == [1, 2, 1] and on[3]["iters"][1] == outs[1]["iters"]
        for b in (0, 2):
            assert all(np.array_equal(on[i][b], off[i][b]) for i in range(3)) and on[3]["iters"][b] == off[3]["iters"][b]
        pm, x0, lb, ub = probs[1]
        assert ref.certificate_measures(pm, x0, lb, ub, dy[1], None, EPS, EPS)[1] == 1
        res[mode] = on
    assert np.array_equal(res["fused"][3]["iters"], res["separate"][3]["iters"])


@pytest.mark.parametrize("n,m,N", [(2, 1, 5), (6, 3, 8)])
def test_loop_dual_unbounded(n, m, N):
    probs = [ref.unbounded_problem(n, m, N, seed) for seed in (1, 2)]
    bs = _solver([p[0] for p in probs])
    w, y, z, info = _run(bs, probs, True, max_iter=200)
    dy, dw = bs.admm_certificate()
    assert np.count_nonzero(bs.status()) == 0
    bs.close()
    assert list(info["status"]) == [3, 3] and list(info["iters"]) == [25, 25] and not info["converged"].any()
    for b, (pm, x0, lb, ub) in enumerate(probs):
        meas, verdict = ref.certificate_measures(pm, x0, lb, ub, None, dw[b], EPS, EPS)
        print(b, "numpy measures of the device dw", meas[4:])
        assert verdict == 2


def test_one_test_switched_off():
    """A tolerance of 0 switches that test off: the unbounded problems are not
    recognised by the primal test alone: the test at iteration 25, which certifies
    them in test_loop_dual_unbounded, leaves them iterating."""
    probs = [ref.unbounded_problem(2, 1, 5, seed) for seed in (1, 2)]
    bs = _solver([p[0] for p in probs])
    x0, lb, ub = (np.ascontiguousarray(np.stack([p[i] for p in probs])) for i in (1, 2, 3))
    w, y, z = np.zeros((2, probs[0][0].h.size)), np.zeros(lb.shape), np.zeros(lb.shape)
    info = bs.admm_solve(x0, lb, ub, np.full(lb.shape, 10.0), w, y, z, detect_infeasibility=True, eps_prim_inf=EPS,
                         eps_dual_inf=0.0, **{**LOOP, "max_iter": 25})
    bs.close()
    assert list(info["status"]) == [0, 0] and list(info["iters"]) == [25, 25]


# ---------------------------------------------------------------------------
# unsupported handles and call order
# ---------------------------------------------------------------------------
def _code(fn, *a):
    from pdplqr._lib import PdplqrError

    with pytest.raises(PdplqrError) as e:
        fn(*a)
    return e.value.code


def test_unsupported_and_argument_checks():
    from pdplqr import BatchedLQRSolver

    kkt = BatchedLQRSolver(4, 2, 6, 1, solver="kkt", ncs=[2] * 6 + [0])
    assert _code(kkt.handle.set_infeasibility_detection, True) == -5
    kkt.handle.set_infeasibility_detection(False)  # switching off is always fine
    kkt.close()
    md = BatchedLQRSolver(4, 2, 8, 1, solver="parallel", num_segments=2, ncs=[2] * 8 + [0], devices=[0])
    assert _code(md.handle.set_infeasibility_detection, True) == -5
    md.close()
    xl = BatchedLQRSolver(60, 8, 2, 1, ncs=[1, 1, 0])  # nx + nu = 68
    assert _code(xl.handle.set_infeasibility_detection, True) == -5
    xl.close()
    bs = BatchedLQRSolver(4, 2, 6, 1, ncs=[2] * 6 + [0])
    assert _code(bs.handle.set_infeasibility_detection, True, -1e-4, 1e-4) == -1
    assert _code(bs.handle.set_infeasibility_detection, True, 1e-4, float("nan")) == -1
    bs.handle.set_infeasibility_detection(True, 0.0, 1e-4)
    assert _code(bs.handle.admm_status) == -4  # before any admm_solve
    bs.close()


def test_status_and_certificate_with_detection_off():
    probs, _ = _mixed(3, 2, 6)
    bs = _solver([p[0] for p in probs])
    _, _, _, info = _run(bs, probs, False, max_iter=100)
    assert np.array_equal(bs.handle.admm_status(), info["converged"].astype(np.int32))
    assert set(info["status"]) == {0, 1}
    assert _code(bs.admm_certificate) == -4
    bs.close()


def test_adaptive_rho_with_an_infeasible_neighbour():
    """Adaptive rho on, one infeasible problem in the batch: the others end
    with the status they have without detection; the certified one keeps the
    rho it was certified with."""
    probs, _ = _mixed(3, 2, 6)
    probs = [probs[0], probs[1], probs[2]]
    bs = _solver([p[0] for p in probs])
    _, _, _, on = _run(bs, probs, True, adaptive_rho=True)
    _, _, _, off = _run(bs, probs, False, adaptive_rho=True)
    bs.close()
    print("adaptive: on", on["status"], on["iters"], "off", off["status"], off["iters"])
    assert on["status"][1] == 2
    assert on["status"][0] == off["status"][0] == 1 and on["status"][2] == off["status"][2] == 1


# ---------------------------------------------------------------------------
# BoxLQRLayer
# ---------------------------------------------------------------------------
def _layer_leaves(probs, need=True):
    import torch

    arrs = dict(_arrays([p[0] for p in probs]), x0=np.stack([p[1] for p in probs]), lb=np.stack([p[2] for p in probs]),
                ub=np.stack([p[3] for p in probs]))
    return [torch.tensor(arrs[k], device="cuda", requires_grad=need) for k in "E c H h x0 D lb ub".split()]


def test_layer_refuses_an_infeasible_problem():
    from pdplqr import BoxLQRLayer

    n, m, N = 3, 2, 6
    probs, _ = _mixed(n, m, N)
    probs = [probs[0], probs[2], probs[1]]  # the infeasible one is problem 2
    ncs = [int(x) for x in probs[0][0].ncs]
    for allow in (False, True):
        layer = BoxLQRLayer(n, m, N, 3, ncs, rho=10.0, eps=1e-6, max_iter=400, detect_infeasible=True,
                            allow_unconverged=allow)
        ws = layer(*_layer_leaves(probs))
        assert list(layer.admm_info["status"]) == [1, 1, 2]
        with pytest.raises(RuntimeError, match=r"problem 2 .*primal infeasible"):
            ws.sum().backward()
        layer.close()
    # without detection the same batch is only "not converged"
    layer = BoxLQRLayer(n, m, N, 3, ncs, rho=10.0, eps=1e-6, max_iter=100)
    ws = layer(*_layer_leaves(probs))
    with pytest.raises(RuntimeError, match="converge"):
        ws.sum().backward()
    layer.close()


def test_layer_gradients_unchanged_when_feasible():
    import torch

    from pdplqr import BoxLQRLayer

    n, m, N = 3, 2, 6
    probs, _ = _mixed(n, m, N)
    probs = [probs[0], probs[2], probs[4]]
    ncs = [int(x) for x in probs[0][0].ncs]
    gws = torch.tensor(np.random.default_rng(3).standard_normal((3, probs[0][0].h.size)), device="cuda")
    grads = []
    for detect in (False, True):
        layer = BoxLQRLayer(n, m, N, 3, ncs, rho=10.0, eps=1e-6, max_iter=400, adj_max_iter=400,
                            detect_infeasible=detect)
        leaves = _layer_leaves(probs)
        ws = layer(*leaves)
        assert list(layer.admm_info["status"]) == [1, 1, 1]
        (gws * ws).sum().backward()
        grads.append([ws.detach().cpu().numpy()] + [t.grad.cpu().numpy() for t in leaves])
        layer.close()
    for a, b in zip(*grads):
        assert np.array_equal(a, b)
