#!/usr/bin/env python3
"""Cost of the second-order cone rows of the ADMM loop (pdplqr_admm_set_cones)
at the conic configuration: N = 512, nx = 12, nu = 4, batch 1024, SERIAL,
keep_factors = 1, device buffers, rho = 1 fixed, 200 iterations (eps = 0), a
termination test every 25, 5 constraint rows per stage: a zero row and one row
per input (none at the terminal).

Variants (every one with PDPLQR_NO_ADMM_FUSE=1):
  a   the library given by --parent-lib (the parent commit's build), the 5 rows
      as box rows |u_i| <= r
  b   this tree's library, the same
  c   this tree's library, the 5 rows as one cone |u_k| <= r
Each measurement is one event-timed solve in a fresh process (after one
25-iteration solve that loads the code objects); the driver interleaves the
variants, --reps processes each, and reports medians, the spread (min .. max)
of every variant, b against a, and c per iteration against the compulsory
bytes of the cone update pass.  Prints ONE JSON line (and writes it to --out).
Without --parent-lib variant a is skipped.  Needs a GPU; run it under `timeout`.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pdp-lqr_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E (bench.py)


def pass_bytes(n, m, N, batch, nc):
    """Compulsory bytes of one fused cone update pass over nc cone rows per stage
    k < N: reads w~, w, h (3 s), D (nc s), z, y, rho, inv_rho, lb (5 nc); writes
    w, h~ (2 s) and z, y, g (3 nc).  The second walk over a cone re-reads D and
    the row vectors (cache hits, not counted)."""
    s = n + m
    return 8 * batch * (N * (5 * s + nc * s + 8 * nc) + 2 * n)


def child(a):
    import torch

    from pdplqr import BatchedLQRSolver
    from polish_bench import gen

    n, m, N, batch, nc = a.n, a.m, a.N, a.batch, a.m + 1
    s = n + m
    f64 = torch.float64
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)  # one stream for torch and the handle: the events bracket the handle's work
    torch.cuda.set_stream(stream)
    E, c, H, h, x0 = gen(n, m, N, batch, dev)
    ncs = [nc] * N + [0]
    ny, nw = N * nc, N * s + n
    Dk = torch.zeros(nc, s, dtype=f64, device=dev)
    Dk[1:, :m] = torch.eye(m, dtype=f64, device=dev)
    D = Dk.t().reshape(-1).repeat(N).expand(batch, -1).contiguous()  # column-major per stage
    r = a.radius
    cone = a.child == "c"
    if cone:  # D w - lb = (r, u): |u| <= r
        lb = torch.tensor([-r] + [0.0] * m, dtype=f64, device=dev).repeat(N).expand(batch, -1).contiguous()
        ub = lb.clone()
    else:
        lb = torch.full((batch, ny), -r, dtype=f64, device=dev)
        ub = torch.full((batch, ny), r, dtype=f64, device=dev)
    rho = torch.full((batch, ny), 1.0, dtype=f64, device=dev)
    bs = BatchedLQRSolver(n, m, N, batch, keep_factors=True, ncs=ncs)
    bs.handle.set_stream(stream.cuda_stream)
    bs.set_model(E, c, H, h, D)
    if cone:
        bs.set_cones([(k, 0, nc) for k in range(N)])
    w, y, z = (torch.zeros(batch, k, dtype=f64, device=dev) for k in (nw, ny, ny))
    kw = dict(sigma=1e-6, alpha=1.6, check_every=25, eps_abs=0.0, eps_rel=0.0, adaptive_rho=False)
    bs.admm_solve(x0, lb, ub, rho, w, y, z, max_iter=25, **kw)  # loads the code objects
    w.zero_(), y.zero_(), z.zero_()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    info = bs.admm_solve(x0, lb, ub, rho, w, y, z, max_iter=a.iters, **kw)
    e1.record()
    e1.synchronize()
    u = w[:, :N * s].reshape(batch, N, s)[:, :, :m]
    out = {"ms": e0.elapsed_time(e1), "iterations": int(info["iterations"]),
           "prim_res_max": float(info["prim_res"].max()), "finite": bool(torch.isfinite(w).all()), "status_nonzero": int((bs.status() != 0).sum()),
           "u_norm_max": float(u.norm(dim=2).max()), "u_abs_max": float(u.abs().max())}
    bs.close()  # while its stream is alive
    print("CHILD " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=512)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--n", type=int, default=12)
    ap.add_argument("--m", type=int, default=4)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--radius", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-lib", default=None, help="libpdplqr.so built from the parent commit (variant a)")
    ap.add_argument("--child", default=None, choices=["a", "b", "c"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    variants = (["a"] if a.parent_lib else []) + ["b", "c"]
    runs = {v: [] for v in variants}
    last = {}
    for _ in range(a.reps):
        for v in variants:
            env = dict(os.environ, PDPLQR_NO_ADMM_FUSE="1")
            env.pop("PDPLQR_LIB", None)
            if v == "a":
                env["PDPLQR_LIB"] = os.path.abspath(a.parent_lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", v, "--N", str(a.N), "--batch", str(a.batch),
                   "--n", str(a.n), "--m", str(a.m), "--iters", str(a.iters), "--radius", str(a.radius)]
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("CHILD ")]
            if p.returncode != 0 or not lines:
                sys.exit(f"cone_bench: variant {v} failed (rc {p.returncode}):\n{p.stdout}\n{p.stderr}")
            last[v] = json.loads(lines[-1][6:])
            runs[v].append(last[v]["ms"])
    nc = a.m + 1
    res = {"config": {"n": a.n, "m": a.m, "N": a.N, "batch": a.batch, "rows_per_stage": nc, "rho": 1.0,
                      "iterations": a.iters, "check_every": 25, "radius": a.radius, "keep_factors": 1,
                      "reps": a.reps, "no_admm_fuse": 1}}
    for v in variants:
        res[v] = {"ms_median": round(statistics.median(runs[v]), 3), "ms_min": round(min(runs[v]), 3),
                  "ms_max": round(max(runs[v]), 3), "ms_per_iteration": round(statistics.median(runs[v]) / a.iters, 5),
                  "all_ms": [round(x, 3) for x in runs[v]], "last": last[v]}
    if "a" in res:
        res["b_over_a"] = round(res["b"]["ms_median"] / res["a"]["ms_median"], 4)
        res["spread_a"] = round((res["a"]["ms_max"] - res["a"]["ms_min"]) / res["a"]["ms_median"], 4)
    res["spread_b"] = round((res["b"]["ms_max"] - res["b"]["ms_min"]) / res["b"]["ms_median"], 4)
    res["c_over_b"] = round(res["c"]["ms_median"] / res["b"]["ms_median"], 4)
    by = pass_bytes(a.n, a.m, a.N, a.batch, nc)
    res["cone_pass_bytes"] = by
    res["cone_pass_ms_at_hbm_peak"] = round(by / HBM_PEAK_GBS / 1e6, 4)
    res["c_minus_b_ms_per_iteration"] = round(res["c"]["ms_per_iteration"] - res["b"]["ms_per_iteration"], 5)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
