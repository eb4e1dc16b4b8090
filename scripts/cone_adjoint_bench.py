#!/usr/bin/env python3
"""Cost of the fixed-point adjoint on the device (pdplqr_admm_adjoint_fixed_point)
against BoxLQRLayer's torch loop, at the conic configuration: N = 512, nx = 12,
nu = 4, batch 1024, SERIAL, keep_factors = 1, device buffers, rho = 1 fixed,
eps = 1e-6, adj_tol = 1e-8, tests every 25 iterations.

Variants:
  a   BoxLQRLayer.backward in its default mode (the torch loop over
      pdplqr_adjoint_rows), a box |u_i| <= width on the 4 inputs, all eight
      gradients
  b   pdplqr_admm_adjoint_fixed_point on the same problem (no cones), all
      eight gradients
  c   the same with 5 rows per stage (a zero row and one row per input) as
      one cone |u_k| <= --radius
Each measurement is one event-timed call in a fresh process (after the forward
solve and one short call that loads the code objects); the driver interleaves
the variants, --reps processes each, and reports medians, the spread
(min .. max), ms per adjoint iteration, b against a.  Variants b and c also
time k_fpadj_step alone (a middle step on the state the call left) against a device
copy_ of its compulsory bytes.  Prints ONE JSON line (and writes it to --out).
Needs a GPU; run it under `timeout`.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pdp-lqr_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E (bench.py)
KEYS = ("E", "c", "H", "h", "x0", "D", "lb", "ub")


def step_bytes(n, m, N, batch, nc):
    """Compulsory bytes of one k_fpadj_step over nc rows per stage k < N: reads
    v, a_w, gws (3 s), D (nc s), rho, a_y, a_z, P^T q, ys, zs, lb, ub (8 nc);
    writes a_w, rhs (2 s) and a_y, a_z, P^T q (3 nc)."""
    s = n + m
    return 8 * batch * (N * (5 * s + nc * s + 11 * nc) + 5 * n)


def child(a):
    import torch

    from pdplqr import BatchedLQRSolver, BoxLQRLayer, ConeLQRLayer, _lib
    from polish_bench import gen

    n, m, N, batch = a.n, a.m, a.N, a.batch
    cone = a.child == "c"
    nc = m + 1 if cone else m
    s = n + m
    f64 = torch.float64
    dev = torch.device("cuda", 0)
    E, c, H, h, x0 = gen(n, m, N, batch, dev)
    ncs = [nc] * N + [0]
    ny, nw = N * nc, N * s + n
    Dk = torch.zeros(nc, s, dtype=f64, device=dev)
    Dk[nc - m:, :m] = torch.eye(m, dtype=f64, device=dev)
    D = Dk.t().reshape(-1).repeat(N).expand(batch, -1).contiguous()  # column-major per stage
    if cone:  # D w - lb = (r, u): |u| <= r
        lb = torch.tensor([-a.radius] + [0.0] * m, dtype=f64, device=dev).repeat(N).expand(batch, -1).contiguous()
        ub = lb.clone()
    else:
        # the box of scripts/admm_adjoint_bench.py: half the mean |u| of the unconstrained optimum
        plain = BatchedLQRSolver(n, m, N, batch, keep_factors=True)
        plain.set_model(E, c, H, h, None)
        w_unc = torch.zeros(batch, nw, dtype=f64, device=dev)
        plain.update_problem_data(w_unc, sigma=1e-6)
        plain.backward()
        plain.forward(x0, w_unc)
        torch.cuda.synchronize()
        plain.close()
        width = 0.5 * float(w_unc[:, :N * s].reshape(batch, N, s)[:, :, :m].abs().mean())
        lb = torch.full((batch, ny), -width, dtype=f64, device=dev)
        ub = torch.full((batch, ny), width, dtype=f64, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    gws = torch.randn(batch, nw, dtype=f64, device=dev, generator=g)
    data = dict(E=E, c=c, H=H, h=h, x0=x0, D=D, lb=lb, ub=ub)
    cfg = dict(rho=a.rho, sigma=1e-6, alpha=1.6, eps=a.eps, max_iter=a.max_iter, adj_tol=a.adj_tol,
               adj_max_iter=a.max_iter, check_every=25, allow_unconverged=True)
    if a.child == "a":
        ly = BoxLQRLayer(n, m, N, batch, ncs, **cfg)
    else:
        ly = ConeLQRLayer(n, m, N, batch, ncs, cones=[(k, 0, nc) for k in range(N)] if cone else [], **cfg)
    leaves = [data[k].clone().requires_grad_(True) for k in KEYS]
    ws = ly(*leaves)
    loss = (gws * ws).sum()
    out = {"admm_iters_max": int(ly.admm_info["iters"].max()), "converged": int(ly.admm_info["converged"].sum())}
    # one short backward loads the code objects
    full = (ly.adj_max_iter, ly.check_every)
    ly.adj_max_iter, ly.check_every = 2, 1
    loss.backward(retain_graph=True)
    ly.adj_max_iter, ly.check_every = full
    for t in leaves:
        t.grad = None
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    loss.backward(retain_graph=True)
    e1.record()
    e1.synchronize()
    out["ms"] = e0.elapsed_time(e1)
    out["adjoint_iters"] = int(ly.adjoint_iterations)
    out["finite"] = bool(all(torch.isfinite(t.grad).all() for t in leaves))
    out["grad_h_norm"] = float(leaves[3].grad.norm())
    if a.child != "a":
        info = ly.adjoint_info
        out["adjoint_converged"] = int(info["converged"].sum())
        out["adjoint_iters_min"] = int(info["iters"].min())
        # k_fpadj_step alone: a middle step on what the call left, against a copy_ of its compulsory bytes
        hd = ly.handle
        L = _lib.lib()
        L.pdplqr_debug_fpadj_step.argtypes = [C.c_void_p] * 7 + [C.c_double] * 2
        L.pdplqr_debug_fpadj_step.restype = C.c_int
        nbytes = step_bytes(n, m, N, batch, nc)
        src = torch.randn(nbytes // 16, dtype=f64, device=dev)
        dst = torch.empty_like(src)

        # the vectors of the timed call: what the layer's forward saved for backward, and the loss's gws
        _, ys, zs, slb, sub = ws.grad_fn.saved_tensors
        vecs = [C.c_void_p(t.data_ptr()) for t in (ys, zs, slb, sub, ly._rho, gws)]

        def step():
            cur = hd._enter(gws)
            _lib.check(L.pdplqr_debug_fpadj_step(hd.h, *vecs, ly.sigma, ly.alpha))
            hd._leave(cur)

        times = {"step_ms": [], "step_copy_ms": []}
        for it in range(1 + a.kernel_reps):
            for k, fn in (("step_ms", step), ("step_copy_ms", lambda: dst.copy_(src))):
                k0, k1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                k0.record()
                fn()
                k1.record()
                k1.synchronize()
                if it:
                    times[k].append(k0.elapsed_time(k1))
        for k, v in times.items():
            out[k] = statistics.median(v)
        out["step_bytes"] = nbytes
    ly.close()
    print("CHILD " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=512)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--n", type=int, default=12)
    ap.add_argument("--m", type=int, default=4)
    ap.add_argument("--rho", type=float, default=1.0)
    ap.add_argument("--eps", type=float, default=1e-6)
    ap.add_argument("--adj-tol", type=float, default=1e-8)
    ap.add_argument("--max-iter", type=int, default=8000)
    ap.add_argument("--radius", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernel-reps", type=int, default=7)
    ap.add_argument("--child", default=None, choices=["a", "b", "c"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    variants = ["a", "b", "c"]
    runs = {v: [] for v in variants}
    last = {}
    for rep in range(a.reps):
        for v in variants[rep % 3:] + variants[:rep % 3]:  # interleaved, the order rotating
            env = dict(os.environ)
            env.pop("PDPLQR_LIB", None)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", v]
            for k in ("N", "batch", "n", "m", "rho", "eps", "adj_tol", "max_iter", "radius", "kernel_reps"):
                cmd += ["--" + k.replace("_", "-"), str(getattr(a, k))]
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("CHILD ")]
            if p.returncode != 0 or not lines:
                sys.exit(f"cone_adjoint_bench: variant {v} failed (rc {p.returncode}):\n{p.stdout}\n{p.stderr}")
            last[v] = json.loads(lines[-1][6:])
            runs[v].append(last[v])
            print(f"rep {rep} {v}: {last[v]['ms']:.3f} ms, {last[v]['adjoint_iters']} iterations", file=sys.stderr,
                  flush=True)
    res = {"config": {"n": a.n, "m": a.m, "N": a.N, "batch": a.batch, "rho": a.rho, "eps": a.eps,
                      "adj_tol": a.adj_tol, "check_every": 25, "radius": a.radius, "keep_factors": 1, "reps": a.reps}}
    for v in variants:
        ms = [r["ms"] for r in runs[v]]
        med = statistics.median(ms)
        res[v] = {"ms_median": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
                  "spread": round((max(ms) - min(ms)) / med, 4), "adjoint_iters": last[v]["adjoint_iters"],
                  "ms_per_iteration": round(med / (last[v]["adjoint_iters"] + 1), 5),
                  "all_ms": [round(x, 3) for x in ms], "last": last[v]}
        if v != "a":
            st = statistics.median(r["step_ms"] for r in runs[v])
            cp = statistics.median(r["step_copy_ms"] for r in runs[v])
            res[v].update(step_ms=round(st, 4), step_copy_ms=round(cp, 4), step_over_copy=round(st / cp, 3),
                          step_bytes=last[v]["step_bytes"], step_gbs=round(last[v]["step_bytes"] / st / 1e6, 1),
                          step_hbm_fraction=round(last[v]["step_bytes"] / st / 1e6 / HBM_PEAK_GBS, 3))
    res["b_over_a"] = round(res["b"]["ms_median"] / res["a"]["ms_median"], 4)
    res["c_over_b_per_iteration"] = round(res["c"]["ms_per_iteration"] / res["b"]["ms_per_iteration"], 4)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
