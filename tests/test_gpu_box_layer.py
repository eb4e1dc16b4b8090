"""GPU checks of pdplqr.BoxLQRLayer (pdplqr/diff.py): the box-constrained
solve by pdplqr_admm_solve and its fixed-point adjoint over
pdplqr_adjoint_rows, against autograd through the active-set KKT solve
(tests/adjoint_rows_ref.py) on strictly complementary problems.

The cases, seeds and stopping rules are those of
tests/test_adjoint_rows_cpu.py::test_recursion_at_layer_settings (LAYER there:
eps = 1e-9, adj_tol = 1e-10, tests every 25 iterations, caps 2000), where the
dense CPU restatement of the same two iterations reaches a worst gradient
error of 2.2e-12 at (3, 2, 6) and 3.0e-10 at (12, 4, 4)
(adjoint_rows_ref.LAYER_CPU_ERR: truncation of the iterations, not rounding).
The tolerance here is 10 times that, for the device's summation order:
2.3e-11 and 3.0e-9, on every gradient array of every problem.  The solution
itself is held the same way against the active-set optimum: the restatement
reaches 3.9e-13 and 2.8e-10 (adjoint_rows_ref.LAYER_CPU_WS_ERR), the bound is
10 times that.
"""
import numpy as np
import pytest

import adjoint_ref
import adjoint_rows_ref as rr
from test_adjoint_rows_cpu import BOX_CASES, LAYER

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    from pdplqr import device_count

    assert device_count() > 0, "no HIP device visible: GPU tests must run on an MI355X"


def _layer(n, m, N, batch, ncs, **kw):
    from pdplqr import BoxLQRLayer

    cfg = dict(rho=10.0, sigma=1e-6, alpha=1.6, eps=LAYER["eps_abs"], max_iter=LAYER["max_iter"],
               adj_tol=LAYER["adj_tol"], adj_max_iter=LAYER["adj_max_iter"], check_every=LAYER["check_every"])
    cfg.update(kw)
    return BoxLQRLayer(n, m, N, batch, ncs, **cfg)


def _leaves(bcs, need=rr.BOX_KEYS):
    import torch

    return [torch.tensor(np.stack([bc[k] for bc in bcs]), device="cuda", requires_grad=(k in need)) for k in rr.BOX_KEYS]


@pytest.mark.parametrize("case", BOX_CASES, ids=lambda cse: "-".join(map(str, cse[:3])))
def test_box_layer_matches_active_set(case):
    import torch

    n, m, N, seeds = case
    bcs = [rr.box_case(n, m, N, seed) for seed in seeds]
    ncs = bcs[0]["dims"][3]
    layer = _layer(n, m, N, len(seeds), ncs)
    leaves = _leaves(bcs)
    ws = layer(*leaves)
    info = layer.admm_info
    print(case, "admm iters", info["iters"], "converged", info["converged"])
    assert info["converged"].all()
    gws = torch.tensor(np.stack([bc["gws"] for bc in bcs]), device="cuda")
    (gws * ws).sum().backward()
    print(case, "adjoint iterations", layer.adjoint_iterations)
    assert layer.adjoint_iterations < LAYER["adj_max_iter"]
    w = ws.detach().cpu().numpy()
    tol = 10 * rr.LAYER_CPU_ERR[(n, m, N)]
    worst = 0.0
    for b, bc in enumerate(bcs):
        err = adjoint_ref.rel(w[b], bc["ws"])
        print(case, seeds[b], "ws", err)
        assert err < 10 * rr.LAYER_CPU_WS_ERR[(n, m, N)]
        for k, t in zip(rr.BOX_KEYS, leaves):
            err = adjoint_ref.rel(t.grad[b].cpu().numpy().ravel(), bc["grads"][k])
            worst = max(worst, err)
            print(case, seeds[b], k, err)
    assert worst < tol, (worst, tol)


def test_box_layer_guards_and_partial_gradients():
    n, m, N, seeds = BOX_CASES[0]
    bcs = [rr.box_case(n, m, N, seed) for seed in seeds]
    ncs = bcs[0]["dims"][3]
    # an unconverged solve cannot be differentiated ...
    layer = _layer(n, m, N, len(seeds), ncs, max_iter=2)
    leaves = _leaves(bcs)
    ws = layer(*leaves)
    assert not layer.admm_info["converged"].all()
    with pytest.raises(RuntimeError, match="converge"):
        ws.sum().backward()
    # ... unless asked for
    layer = _layer(n, m, N, len(seeds), ncs, max_iter=2, allow_unconverged=True, adj_max_iter=3)
    layer(*leaves).sum().backward()
    assert leaves[3].grad is not None
    # a stale factor
    layer = _layer(n, m, N, len(seeds), ncs)
    leaves = _leaves(bcs)
    first = layer(*leaves)
    second = layer(*leaves)
    with pytest.raises(RuntimeError, match="factorization"):
        first.sum().backward()
    # only h and lb need gradients: nothing else is written
    leaves = _leaves(bcs, need=("h", "lb"))
    import torch

    gws = torch.tensor(np.stack([bc["gws"] for bc in bcs]), device="cuda")
    ws = layer(*leaves)
    # record the output arguments of every adjoint_rows call of the backward pass
    names = ("gE", "gc", "gH", "gh", "gx", "gD", "gg", "grho")
    hd, asked = layer.handle, []
    inner = hd.adjoint_rows

    def recording(ws_, rho_, gws_, gvs_=None, *outs, **kw):
        kw.update(zip(names, outs))
        asked.append({k for k in names if kw.get(k) is not None})
        return inner(ws_, rho_, gws_, gvs_, **kw)

    hd.adjoint_rows = recording
    try:
        (gws * ws).sum().backward()
    finally:
        del hd.adjoint_rows
    assert len(asked) == layer.adjoint_iterations + 1
    assert all(a == {"gh", "gg"} for a in asked[:-1])  # the iteration
    assert asked[-1] == {"gh"}                          # the final call: h only (lb's term is elementwise)
    tol = 10 * rr.LAYER_CPU_ERR[(n, m, N)]
    for k, t in zip(rr.BOX_KEYS, leaves):
        if k in ("h", "lb"):
            for b, bc in enumerate(bcs):
                assert adjoint_ref.rel(t.grad[b].cpu().numpy().ravel(), bc["grads"][k]) < tol, k
        else:
            assert t.grad is None, k
