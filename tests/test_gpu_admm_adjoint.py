"""GPU checks of pdplqr_admm_adjoint (csrc/adjoint.hip, csrc/kernels_asadj.hip;
DESIGN.md section 5.9) through the C ABI: set_model -> set_polish(True, 1e-6, 3)
-> admm_solve (rho = 10 fixed, eps_abs = 1e-6) -> every problem ACCEPTED with the
reference's active count -> admm_adjoint, against autograd through the KKT
solve on the active set (tests/admm_adjoint_ref.py).

Tolerance: the project's polish rule (tests/test_gpu_polish.py), per problem
and per gradient array: 1000 * max(e_ref, 5e-14) in max-norm relative to the
array's max-norm, e_ref being the dense CPU restatement's own error against
autograd for that problem and array (admm_adjoint_ref.graded).  The factor is
DESIGN.md section 5.8's: the 1/delta penalty through the stage recursion costs
up to two digits against a dense inverse.
"""
import numpy as np
import pytest

import admm_adjoint_ref as ar
import admm_infeas_ref as ref
from test_adjoint_rows_cpu import BOX_CASES, LAYER

pytestmark = pytest.mark.gpu

REF_ERR_FLOOR = 5e-14
OUT = ("gE", "gc", "gH", "gh", "gx", "gD", "glb", "gub")  # in the order of ar.KEYS
SOLVE = dict(sigma=1e-6, alpha=1.6, max_iter=4000, check_every=25, eps_abs=1e-6, eps_rel=0.0, adaptive_rho=False)
# (n, m, N, seeds, ragged): one batch of three per line
CASES = [(n, m, N, seeds or ar.RAGGED_SEEDS, rg) for n, m, N, seeds, rg in ar.CASES]


def _id(cse):
    return "-".join(map(str, cse[:3])) + ("-ragged" if cse[4] else "")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from pdplqr import device_count

    assert device_count() > 0, "no HIP device visible: GPU tests must run on an MI355X"


def _code(fn, *a, **kw):
    from pdplqr._lib import PdplqrError

    with pytest.raises(PdplqrError) as e:
        fn(*a, **kw)
    return e.value.code


def _problems(cse):
    n, m, N, seeds, rg = cse
    return [ar.problem(n, m, N, seed, rg) for seed in seeds]


def _stack(prs, k):
    return np.ascontiguousarray(np.stack([p[k] for p in prs]))


def _solved(prs, refine=3, polish=True, **kw):
    """A handle after admm_solve from a zero start: (solver, w, y, z, info)."""
    from pdplqr import BatchedLQRSolver

    n, m, N, ncs = prs[0]["dims"]
    kw.setdefault("keep_factors", True)
    bs = BatchedLQRSolver(n, m, N, len(prs), ncs=list(ncs), **kw)
    bs.set_model(*[_stack(prs, k) for k in ("E", "c", "H", "h", "D")])
    if polish:
        bs.set_polish(True, 1e-6, refine)
    lb = _stack(prs, "lb")
    w, y, z = np.zeros((len(prs), prs[0]["h"].size)), np.zeros(lb.shape), np.zeros(lb.shape)
    info = bs.admm_solve(_stack(prs, "x0"), lb, _stack(prs, "ub"), np.full(lb.shape, 10.0), w, y, z, **SOLVE)
    return bs, w, y, z, info


def _accepted(bs, prs, info):
    pi = bs.polish_info()
    print("admm iters", info["iters"], "polish", pi["status"], "n_active", pi["n_active"],
          "reference", [p["n_active"] for p in prs])
    assert list(info["status"]) == [1] * len(prs)
    assert list(pi["status"]) == [1] * len(prs)
    assert list(pi["n_active"]) == [p["n_active"] for p in prs]
    return pi


def _blank(prs, want=OUT):
    return {o: (np.full((len(prs), prs[0][k].size), 7.0) if o in want else None) for o, k in zip(OUT, ar.KEYS)}


def _adjoint(bs, prs, gvs=None, want=OUT):
    out = _blank(prs, want)
    bs.admm_adjoint(_stack(prs, "gws"), gvs, **out)
    return out


def _check(out, cse, with_gvs, what, only=None):
    n, m, N, seeds, rg = cse
    worst = 0.0
    for b, seed in enumerate(seeds):
        if only is not None and b not in only:
            continue
        g = ar.graded(n, m, N, seed, rg, with_gvs)
        for o, k in zip(OUT, ar.KEYS):
            err, tol = ar.relmax(out[o][b], g["ref"][k]), 1000 * max(g["err"][k], REF_ERR_FLOOR)
            print(what, seed, k, "device", err, "restatement", g["err"][k], "bound", tol)
            worst = max(worst, err / tol)
            assert err <= tol, (what, seed, k, err, tol)
    return worst


@pytest.mark.parametrize("with_gvs", [False, True], ids=["gws", "gws+gvs"])
@pytest.mark.parametrize("cse", CASES, ids=_id)
def test_gradients_match_autograd(cse, with_gvs):
    prs = _problems(cse)
    assert min(p["margin"] for p in prs) >= 1e-2
    bs, w, y, z, info = _solved(prs)
    _accepted(bs, prs, info)
    out = _adjoint(bs, prs, _stack(prs, "gvs") if with_gvs else None)
    ai = bs.admm_adjoint_info()
    bs.close()
    print(_id(cse), "status", ai["status"], "resid", ai["resid"])
    assert list(ai["status"]) == [1] * len(prs)
    _check(out, cse, with_gvs, _id(cse))
    assert (ai["resid"][:, 0] < 1e-10).all()


def test_no_active_rows_equals_adjoint():
    """Problem 1 of the batch has bounds so wide that no row is active: its
    gradients are those of the unconstrained solve (pdplqr_adjoint on the model
    without rows), and glb, gub, gD are zero exactly."""
    from pdplqr import BatchedLQRSolver

    cse = CASES[0]
    n, m, N = cse[:3]
    prs = _problems(cse)
    wide = dict(prs[1], lb=np.full(prs[1]["lb"].shape, -50.0), ub=np.full(prs[1]["ub"].shape, 50.0))
    batch = [prs[0], wide, prs[2]]
    bs, w, y, z, info = _solved(batch)
    pi = bs.polish_info()
    assert pi["n_active"][1] == 0 and info["status"][1] == 1
    out = _adjoint(bs, batch)
    ai = bs.admm_adjoint_info()
    bs.close()
    print("status", ai["status"], "resid", ai["resid"])
    assert ai["resid"][1, 0] == 0.0
    for o in ("gD", "glb", "gub"):
        assert not out[o][1].any(), o
    _check(out, cse, False, "beside the wide problem", only=(0, 2))
    plain = BatchedLQRSolver(n, m, N, 1, keep_factors=True)
    one = lambda k: np.ascontiguousarray(wide[k][None])  # noqa: E731
    plain.set_model(one("E"), one("c"), one("H"), one("h"))
    plain.update_problem_data(np.zeros((1, wide["h"].size)), sigma=0.0)
    plain.backward()
    ws = np.zeros((1, wide["h"].size))
    plain.forward(one("x0"), ws)
    want = {o: np.zeros((1, wide[k].size)) for o, k in zip(OUT[:5], ar.KEYS[:5])}
    plain.adjoint(ws, one("gws"), **want)
    plain.close()
    for o in OUT[:5]:
        err = ar.relmax(out[o][1], want[o][0])
        print("no active rows", o, err)
        assert err <= 1000 * REF_ERR_FLOOR, (o, err)


@pytest.mark.parametrize("cse", [CASES[1], CASES[4]], ids=_id)
def test_null_outputs_repeats_and_device_buffers(cse):
    """A value does not depend on which outputs were asked for, on protocol calls
    in between, or on where the buffers live."""
    import torch

    prs = _problems(cse)
    gvs = _stack(prs, "gvs")
    bs, w, y, z, info = _solved(prs)
    _accepted(bs, prs, info)
    full = _adjoint(bs, prs, gvs)
    for o in OUT:
        one = _adjoint(bs, prs, gvs, want=(o,))
        assert np.array_equal(one[o], full[o]), o
    bs.admm_adjoint(_stack(prs, "gws"), gvs)  # nothing requested: OK
    # protocol calls in between: another x-update, another factor
    g = np.random.default_rng(3)
    bs.update_problem_data(g.standard_normal(w.shape), g.standard_normal(y.shape), g.standard_normal(y.shape),
                           np.full(y.shape, 0.5), sigma=0.3)
    bs.backward(np.full(y.shape, 2.0))
    again = _adjoint(bs, prs, gvs)
    t = lambda a: torch.tensor(a, device="cuda")  # noqa: E731
    dev = {o: torch.full(full[o].shape, 7.0, dtype=torch.float64, device="cuda") for o in OUT}
    bs.admm_adjoint(t(_stack(prs, "gws")), t(gvs), **dev)
    torch.cuda.synchronize()
    bs.close()
    for o in OUT:
        assert np.array_equal(again[o], full[o]), o
        assert np.array_equal(dev[o].cpu().numpy(), full[o]), o


def test_resid_falls_with_the_refinement():
    """refine_iter = 0 .. 3 on one solve (the call takes the handle's setting):
    max|D_a v| / max|v| falls by at least two orders per solve to below 1e-10,
    and one solve alone misses the reference by more than 1e-6."""
    cse = CASES[1]
    prs = _problems(cse)
    bs, w, y, z, info = _solved(prs)
    _accepted(bs, prs, info)
    resid, outs = [], []
    for r in range(4):
        bs.set_polish(True, 1e-6, r)
        outs.append(_adjoint(bs, prs))
        resid.append(bs.admm_adjoint_info()["resid"].copy())
    bs.close()
    print("resid per refine_iter", [x.tolist() for x in resid])
    for a, b in zip(resid, resid[1:]):
        assert (b[:, 0] <= np.maximum(1e-2 * a[:, 0], 1e-13)).all()
    assert (resid[3][:, 0] < 1e-10).all() and (resid[0][:, 0] > 1e-8).all()
    assert (resid[3][:, 1] < resid[1][:, 1]).all()  # the steps themselves shrink
    assert (resid[0][:, 1] == 1.0).all()  # the first step's change is v itself
    g = ar.graded(*cse[:3], cse[3][0], cse[4], False)
    miss = max(ar.relmax(outs[0][o][0], g["ref"][k]) for o, k in zip(OUT, ar.KEYS))
    print("refine_iter = 0 misses by", miss)
    assert miss > 1e-6
    _check(outs[3], cse, False, "refine_iter 3")


def test_handle_state_after_the_call():
    """forward returns w~ (the optimum, to the bound of the polished w); the
    outcome of the solve is untouched."""
    cse = CASES[4]
    prs = _problems(cse)
    bs, w, y, z, info = _solved(prs)
    pi = _accepted(bs, prs, info)
    _adjoint(bs, prs)
    wt = np.zeros_like(w)
    bs.forward(_stack(prs, "x0"), wt)
    pi2, info2 = bs.polish_info(), bs.admm_info()
    _adjoint(bs, prs, want=("gh",))
    wt2 = np.zeros_like(w)
    bs.forward(_stack(prs, "x0"), wt2)
    bs.close()
    assert np.array_equal(wt, wt2)
    for k in pi:
        assert np.array_equal(pi[k], pi2[k]), k
    for k in ("iters", "converged", "prim_res", "dual_res", "status", "polish_status"):
        assert np.array_equal(info[k], info2[k]), k
    for b, seed in enumerate(cse[3]):
        g = ar.graded(*cse[:3], seed, cse[4], False)
        e_ref = ar.relmax(g["wt"], g["ws"])
        err, was = ar.relmax(wt[b], g["ws"]), ar.relmax(w[b], g["ws"])
        print("w~", seed, err, "the solve's w", was, "restatement", e_ref)
        assert err <= 1000 * max(e_ref, REF_ERR_FLOOR)


def test_mixed_batch_status():
    """tests/test_gpu_polish.py's mixed batch (accepted / rejected / certified
    infeasible): EXACT / APPROX / APPROX."""
    from pdplqr import BatchedLQRSolver

    cs = [ref.box_problem(5, 3, 7, "feasible", 6, .1, True), ref.box_problem(5, 3, 7, "feasible", 4, .1, True),
          ref.box_problem(5, 3, 7, "contradictory", 3, .05, True)]
    pm = cs[0][0]
    bs = BatchedLQRSolver(pm.n, pm.m, pm.N, 3, keep_factors=True, ncs=[int(x) for x in pm.ncs])
    bs.set_model(*[np.ascontiguousarray(np.stack([getattr(c[0], k) for c in cs])) for k in "E c H h D".split()])
    bs.set_polish(True, 1e-6, 3)
    x0, lb, ub = (np.ascontiguousarray(np.stack([c[i] for c in cs])) for i in (1, 2, 3))
    w, y, z = np.zeros((3, pm.h.size)), np.zeros(lb.shape), np.zeros(lb.shape)
    info = bs.admm_solve(x0, lb, ub, np.ones(lb.shape), w, y, z, sigma=1e-6, alpha=1.6, max_iter=4000, check_every=5,
                         eps_abs=1e-2, eps_rel=0.0, adaptive_rho=False, detect_infeasibility=True)
    pi = bs.polish_info()
    assert list(info["status"]) == [1, 1, 2] and list(pi["status"]) == [1, 2, 0]  # that test's outcome
    gh = np.zeros_like(w)
    bs.admm_adjoint(np.ones_like(w), None, gh=gh)
    ai = bs.admm_adjoint_info()
    bs.close()
    print("status", ai["status"], "resid", ai["resid"])
    assert list(ai["status"]) == [1, 2, 2]
    assert np.isfinite(gh).all() and gh[0].any()


def test_refusals():
    from pdplqr import BatchedLQRSolver, _lib

    cse = CASES[0]
    prs = _problems(cse)
    n, m, N, ncs = prs[0]["dims"]

    def refused(bs, code):
        out = _blank(prs)
        assert _code(bs.admm_adjoint, _stack(prs, "gws"), None, **out) == code
        assert _lib.lib().pdplqr_last_error()
        assert all(np.all(v == 7.0) for v in out.values())  # nothing was written

    bs, *_ = _solved(prs, solver="parallel", num_segments=2)
    refused(bs, -5)
    bs.close()
    bs = BatchedLQRSolver(n, m, N, len(prs), solver="kkt", ncs=list(ncs))
    refused(bs, -5)
    bs.close()
    bs, w, y, z, info = _solved(prs, keep_factors=False)
    refused(bs, -4)
    bs.close()
    bs, w, y, z, info = _solved(prs, polish=False)  # no polish in the last solve
    refused(bs, -4)
    assert _code(bs.admm_adjoint_info) == -4  # no admm_adjoint has run
    bs.close()
    bs = BatchedLQRSolver(n, m, N, len(prs), keep_factors=True, ncs=list(ncs))  # before any solve
    bs.set_model(*[_stack(prs, k) for k in ("E", "c", "H", "h", "D")])
    bs.set_polish(True, 1e-6, 3)
    refused(bs, -4)
    bs.close()
    # polish on, then a solve with it off: the classification of the earlier solve is stale
    bs, w, y, z, info = _solved(prs)
    _adjoint(bs, prs)
    bs.set_polish(False)
    lb = _stack(prs, "lb")
    bs.admm_solve(_stack(prs, "x0"), lb, _stack(prs, "ub"), np.full(lb.shape, 10.0), w, y, z, **SOLVE)
    refused(bs, -4)
    bs.close()


# ---------------------------------------------------------------------------
# BoxLQRLayer(backward_mode="active_set")
# ---------------------------------------------------------------------------
def _layer(n, m, N, batch, ncs, **kw):
    from pdplqr import BoxLQRLayer

    cfg = dict(rho=10.0, sigma=1e-6, alpha=1.6, eps=1e-6, max_iter=LAYER["max_iter"], adj_tol=LAYER["adj_tol"],
               adj_max_iter=LAYER["adj_max_iter"], check_every=LAYER["check_every"], polish=True,
               backward_mode="active_set")
    cfg.update(kw)
    return BoxLQRLayer(n, m, N, batch, ncs, **cfg)


def _leaves(prs, need=ar.KEYS):
    import torch

    return [torch.tensor(_stack(prs, k), device="cuda", requires_grad=(k in need)) for k in ar.KEYS]


@pytest.mark.parametrize("case", BOX_CASES, ids=lambda cse: "-".join(map(str, cse[:3])))
def test_layer_active_set_mode(case):
    """Against autograd (this file's bound) and against the default mode at the
    settings of tests/test_gpu_box_layer.py (that test's bound for the default
    mode's own error, 10 * LAYER_CPU_ERR, plus this mode's)."""
    import torch

    import adjoint_rows_ref as rr

    n, m, N, seeds = case
    cse = (n, m, N, seeds, False)
    prs = _problems(cse)
    ncs = prs[0]["dims"][3]
    gws = torch.tensor(_stack(prs, "gws"), device="cuda")
    grads = {}
    for mode in ("active_set", "fixed_point"):
        layer = _layer(n, m, N, len(seeds), ncs, backward_mode=mode,
                       **({} if mode == "active_set" else dict(eps=LAYER["eps_abs"], polish=False)))
        leaves = _leaves(prs)
        ws = layer(*leaves)
        assert layer.admm_info["converged"].all()
        (gws * ws).sum().backward()
        print(case, mode, "admm iters", layer.admm_info["iters"], "adjoint iterations", layer.adjoint_iterations)
        grads[mode] = [t.grad.cpu().numpy().reshape(len(seeds), -1) for t in leaves]
        if mode == "active_set":
            assert layer.adjoint_iterations == 4
            assert list(layer.adjoint_info["status"]) == [1] * len(seeds)
        layer.close()
    _check(dict(zip(OUT, grads["active_set"])), cse, False, "layer " + str(case))
    for b, seed in enumerate(seeds):
        g = ar.graded(n, m, N, seed, False, False)
        for i, k in enumerate(ar.KEYS):
            a, f = grads["active_set"][i][b], grads["fixed_point"][i][b]
            diff = float(np.linalg.norm(a - f) / max(np.linalg.norm(g["ref"][k]), 1e-300))
            tol = 10 * rr.LAYER_CPU_ERR[(n, m, N)] + 1000 * max(g["err"][k], REF_ERR_FLOOR) * np.sqrt(a.size)
            print(case, seed, k, "active_set against fixed_point", diff, "bound", tol)
            assert diff <= tol, (k, diff, tol)


def test_layer_guards_and_partial_gradients():
    import torch

    cse = CASES[0]
    n, m, N = cse[:3]
    prs = _problems(cse)
    ncs = prs[0]["dims"][3]
    # a solve that did not converge has no exact gradient ...
    layer = _layer(n, m, N, len(prs), ncs, max_iter=2)
    leaves = _leaves(prs)
    ws = layer(*leaves)
    assert not layer.admm_info["converged"].all()
    with pytest.raises(RuntimeError, match="problem 0 .* no exact active-set gradient"):
        ws.sum().backward()
    assert list(layer.adjoint_info["status"]) == [2] * len(prs)
    layer.close()
    # ... unless asked for
    layer = _layer(n, m, N, len(prs), ncs, max_iter=2, allow_unconverged=True)
    leaves = _leaves(prs)
    layer(*leaves).sum().backward()
    assert leaves[3].grad is not None and torch.isfinite(leaves[3].grad).all()
    layer.close()
    # a stale factor
    layer = _layer(n, m, N, len(prs), ncs)
    leaves = _leaves(prs)
    first = layer(*leaves)
    layer(*leaves)
    with pytest.raises(RuntimeError, match="factorization"):
        first.sum().backward()
    # only h and ub need gradients: one call, nothing else requested
    leaves = _leaves(prs, need=("h", "ub"))
    ws = layer(*leaves)
    hd, asked = layer.handle, []
    inner = hd.admm_adjoint

    def recording(gws_, gvs_=None, *outs):
        asked.append({o for o, v in zip(OUT, outs) if v is not None})
        return inner(gws_, gvs_, *outs)

    hd.admm_adjoint = recording
    try:
        (torch.tensor(_stack(prs, "gws"), device="cuda") * ws).sum().backward()
    finally:
        del hd.admm_adjoint
    layer.close()
    assert asked == [{"gh", "gub"}]
    got = {k: t.grad for k, t in zip(ar.KEYS, leaves)}
    assert all(got[k] is None for k in ar.KEYS if k not in ("h", "ub"))
    for b, seed in enumerate(cse[3]):
        g = ar.graded(n, m, N, seed, False, False)
        for k in ("h", "ub"):
            err = ar.relmax(got[k][b].cpu().numpy(), g["ref"][k])
            assert err <= 1000 * max(g["err"][k], REF_ERR_FLOOR), (k, err)
