#!/usr/bin/env python3
"""Cost of differentiating the box-constrained solve, both ways, at the conic
configuration: N = 512, nx = 12, nu = 4, batch 1024, 4 constraint rows per stage
(a box on the inputs, none at the terminal), SERIAL, keep_factors = 1, device
buffers, rho fixed.

Prints ONE JSON line (and writes it to --out):
  fixed_point_ms     BoxLQRLayer.backward in the default mode (the fixed-point
                     iteration over pdplqr_adjoint_rows), all eight gradients;
                     fixed_point_iters its iteration count
  active_set_ms      the same with backward_mode="active_set" (one
                     pdplqr_admm_adjoint call and one status read)
  call_all_ms        pdplqr_admm_adjoint alone, all outputs
  call_gh_ms         ... asking for gh only
  step_ms, rows_ms   k_asadj_step and k_asadj_rows alone; step_copy_ms,
                     rows_copy_ms a device copy_ of their compulsory bytes
  *_err              the worst gradient error of each mode over (c, h, x0, lb, ub),
                     max-norm relative to the array's, against the default mode
                     at a tight solve (eps = --tight-eps, adj_tol = 1e-12)
Each time is the median of --reps event-timed calls after --warmup calls, the
calls of the measurements interleaved.  One process, one device; run it under
`timeout`.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pdp-lqr_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from adjoint_bench import HBM_PEAK_GBS  # noqa: E402
from polish_bench import gen  # noqa: E402

KEYS = ("E", "c", "H", "h", "x0", "D", "lb", "ub")
SMALL = ("c", "h", "x0", "lb", "ub")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=512)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--n", type=int, default=12)
    ap.add_argument("--m", type=int, default=4)
    ap.add_argument("--rho", type=float, default=1.0)
    ap.add_argument("--eps", type=float, default=1e-6)
    ap.add_argument("--tight-eps", type=float, default=1e-10)
    ap.add_argument("--max-iter", type=int, default=8000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("admm_adjoint_bench: no GPU (this measurement has no CPU form)")
    from pdplqr import BatchedLQRSolver, BoxLQRLayer, _lib

    n, m, N, batch, nc = a.n, a.m, a.N, a.batch, a.m
    s = n + m
    f64 = torch.float64
    dev = torch.device("cuda", 0)
    E, c, H, h, x0 = gen(n, m, N, batch, dev)
    ncs = [nc] * N + [0]
    ny, nw = N * nc, N * s + n
    Dk = torch.zeros(nc, s, dtype=f64, device=dev)
    Dk[:, :m] = torch.eye(m, dtype=f64, device=dev)
    D = Dk.t().reshape(-1).repeat(N).expand(batch, -1).contiguous()  # column-major per stage
    # the box: half the mean |u| of the unconstrained optimum, so that a good part of the rows is active
    plain = BatchedLQRSolver(n, m, N, batch, keep_factors=True)
    plain.set_model(E, c, H, h, None)
    w_unc = torch.zeros(batch, nw, dtype=f64, device=dev)
    plain.update_problem_data(w_unc, sigma=1e-6)
    plain.backward()
    plain.forward(x0, w_unc)
    torch.cuda.synchronize()
    plain.close()
    width = 0.5 * float(w_unc[:, :N * s].reshape(batch, N, s)[:, :, :m].abs().mean())
    del w_unc
    lb = torch.full((batch, ny), -width, dtype=f64, device=dev)
    ub = torch.full((batch, ny), width, dtype=f64, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    gws = torch.randn(batch, nw, dtype=f64, device=dev, generator=g)
    data = dict(E=E, c=c, H=H, h=h, x0=x0, D=D, lb=lb, ub=ub)

    def layer(mode, eps, need=KEYS, **kw):
        cfg = dict(rho=a.rho, sigma=1e-6, alpha=1.6, eps=eps, max_iter=a.max_iter, allow_unconverged=True,
                   polish=(mode == "active_set"), backward_mode=mode)
        cfg.update(kw)
        ly = BoxLQRLayer(n, m, N, batch, ncs, **cfg)
        leaves = [data[k].clone().requires_grad_(k in need) for k in KEYS]
        return ly, leaves, ly(*leaves)

    def grads_of(leaves):
        return {k: t.grad.clone() for k, t in zip(KEYS, leaves) if t.grad is not None}

    res = {"config": {"n": n, "m": m, "N": N, "batch": batch, "nc": nc, "rho": a.rho, "eps": a.eps,
                      "tight_eps": a.tight_eps, "width": width, "keep_factors": 1, "reps": a.reps},
           "device": torch.cuda.get_device_name(dev)}
    # the reference: the default mode at a tight solve, the small gradients only
    ly, leaves, ws = layer("fixed_point", a.tight_eps, need=SMALL, adj_tol=1e-12, adj_max_iter=a.max_iter)
    (gws * ws).sum().backward()
    ref = grads_of(leaves)
    res["ref_admm_iters_max"] = int(ly.admm_info["iters"].max())
    res["ref_converged"] = int(ly.admm_info["converged"].sum())
    res["ref_adjoint_iters"] = int(ly.adjoint_iterations)
    ly.close()
    del ly, leaves, ws

    modes = {}
    for mode in ("fixed_point", "active_set"):
        ly, leaves, ws = layer(mode, a.eps)
        modes[mode] = (ly, leaves, (gws * ws).sum())
        res[mode + "_admm_iters_max"] = int(ly.admm_info["iters"].max())
        res[mode + "_converged"] = int(ly.admm_info["converged"].sum())
    pst = modes["active_set"][0].admm_info["polish_status"]
    res["polish_status"] = {str(v): int((pst == v).sum()) for v in (0, 1, 2)}

    def backward(mode):
        ly, leaves, loss = modes[mode]
        for t in leaves:
            t.grad = None
        loss.backward(retain_graph=True)

    hd = modes["active_set"][0].handle
    outs = [torch.empty(batch, data[k].numel() // batch, dtype=f64, device=dev) for k in KEYS]
    L = _lib.lib()
    L.pdplqr_debug_asadj_step.argtypes = [C.c_void_p]
    L.pdplqr_debug_asadj_rows.argtypes = [C.c_void_p] * 4
    L.pdplqr_debug_asadj_step.restype = L.pdplqr_debug_asadj_rows.restype = C.c_int
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def kernel(fn, *args):
        cur = hd._enter(outs[5])
        _lib.check(fn(hd.h, *args))
        hd._leave(cur)

    step_bytes = 8 * batch * N * (nc * s + 3 * nc + 3 * s)
    rows_bytes = 8 * batch * N * (2 * s + 7 * nc + nc * s)
    src = torch.randn(max(step_bytes, rows_bytes) // 2 // 8, dtype=f64, device=dev)
    dst = torch.empty_like(src)
    runs = {
        "fixed_point_ms": lambda: backward("fixed_point"),
        "active_set_ms": lambda: backward("active_set"),
        "call_all_ms": lambda: hd.admm_adjoint(gws, None, *outs),
        "call_gh_ms": lambda: hd.admm_adjoint(gws, None, gh=outs[3]),
        "step_ms": lambda: kernel(L.pdplqr_debug_asadj_step),
        "rows_ms": lambda: kernel(L.pdplqr_debug_asadj_rows, p(outs[5]), p(outs[6]), p(outs[7])),
        "step_copy_ms": lambda: dst[:step_bytes // 16].copy_(src[:step_bytes // 16]),
        "rows_copy_ms": lambda: dst[:rows_bytes // 16].copy_(src[:rows_bytes // 16]),
    }
    times = {k: [] for k in runs}
    for it in range(a.warmup + a.reps):
        for k, fn in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                times[k].append(e0.elapsed_time(e1))
            if it == 0 and k in ("fixed_point_ms", "active_set_ms"):
                mode = k[:-3]
                got = grads_of(modes[mode][1])
                errs = {q: float((got[q] - ref[q]).abs().max() / ref[q].abs().max()) for q in SMALL}
                res[mode + "_err"] = max(errs.values())
                res[mode + "_errs"] = errs
                res[mode + "_iters"] = int(modes[mode][0].adjoint_iterations)
                if mode == "active_set":
                    ai = modes[mode][0].adjoint_info
                    res["adjoint_status"] = {str(v): int((ai["status"] == v).sum()) for v in (1, 2, 3)}
                    res["adjoint_resid_max"] = [float(ai["resid"][:, 0].max()), float(ai["resid"][:, 1].max())]
    torch.cuda.synchronize()
    for ly, _, _ in modes.values():
        ly.close()
    for k, v in times.items():
        res[k] = round(statistics.median(v), 4)
        res[k.replace("_ms", "_min_ms")] = round(min(v), 4)
        res[k.replace("_ms", "_max_ms")] = round(max(v), 4)
    res["speedup"] = round(res["fixed_point_ms"] / res["active_set_ms"], 2)
    for nm, nbytes in (("step", step_bytes), ("rows", rows_bytes)):
        res[nm + "_bytes"] = nbytes
        res[nm + "_gbs"] = round(nbytes / res[nm + "_ms"] / 1e6, 1)
        res[nm + "_hbm_fraction"] = round(res[nm + "_gbs"] / HBM_PEAK_GBS, 3)
        res[nm + "_over_copy"] = round(res[nm + "_ms"] / res[nm + "_copy_ms"], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
