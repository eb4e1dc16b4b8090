"""Cost of the ADMM infeasibility detection at the conic configuration (N = 512,
12/4, 4 rows per stage, batch 1024, SERIAL, keep_factors = 1, device buffers,
|u| <= 0.5, rho = 1 fixed, zero start, 200 iterations with eps = 0, a
termination test every 25): DESIGN.md section 5.5, profiles/admm/bench_infeas.json.

  python scripts/infeas_bench.py [--parent-lib PATH] [--rounds 7] [--out FILE]

Every measurement is one event-timed admm_solve in a fresh process (one
warm-up solve first); the variants are interleaved round by round and the
medians reported:
  a  the library at PATH (a build of the parent commit), when given
  b  this tree, detection off
  c  this tree, detection on (8 tests: snapshot + both certificate kernels)
The worker of variant c also times each certificate kernel alone
(pdplqr_admm_check_certificates with one half, device buffers, 7 runs).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pdp-lqr_amd")]

N_ITER, CHECK = 200, 25
n, m, N, batch, nc = 12, 4, 512, 1024, 4


def worker(variant):
    import numpy as np
    import torch

    import bench
    from pdplqr import BatchedLQRSolver
    from pdplqr.solvers import admm_settings

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    s = n + m
    E, c, H, h, x0 = bench.gen_batch_device(n, m, N, batch, seed=555, device=dev)
    ncs = np.array([nc] * N + [0], dtype=np.int32)
    Dk = torch.zeros(nc, s, dtype=torch.float64, device=dev)
    Dk[:, :m] = torch.eye(m, dtype=torch.float64, device=dev)
    D = Dk.t().contiguous().reshape(-1).repeat(batch, N)
    ny = nc * N
    f = dict(dtype=torch.float64, device=dev)
    lb, ub, rho = torch.full((batch, ny), -0.5, **f), torch.full((batch, ny), 0.5, **f), torch.full((batch, ny), 1.0, **f)
    w, y, z = torch.zeros(batch, N * s + n, **f), torch.zeros(batch, ny, **f), torch.zeros(batch, ny, **f)
    bs = BatchedLQRSolver(n, m, N, batch, solver="serial", ncs=ncs, keep_factors=True, device=0)
    bs.set_model(E, c, H, h, D)
    hd = bs.handle
    st = admm_settings(max_iter=N_ITER, check_every=CHECK, eps_abs=0.0, eps_rel=0.0, adaptive_rho=False)
    if variant == "c":
        hd.set_infeasibility_detection(True, 1e-4, 1e-4)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def solve():
        w.zero_(), y.zero_(), z.zero_()
        return timed(lambda: hd.admm_solve(x0, lb, ub, rho, w, y, z, st))

    solve()
    out = {"variant": variant, "solve_ms": solve(), "finite": bool(torch.isfinite(w).all().item())}
    if variant == "c":
        out["status_counts"] = np.bincount(hd.admm_status(), minlength=4).tolist()
        dy, dw = torch.randn(batch, ny, **f), torch.randn(batch, N * s + n, **f)
        for key, a, b in (("primal_ms", dy, None), ("dual_ms", None, dw)):
            hd.check_certificates(x0, lb, ub, a, b)
            out[key] = statistics.median(timed(lambda: hd.check_certificates(x0, lb, ub, a, b)) for _ in range(7))
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker")
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker)
    variants = (["a"] if a.parent_lib else []) + ["b", "c"]
    runs = {v: [] for v in variants}
    extra = {"primal_ms": [], "dual_ms": []}
    for _ in range(a.rounds):
        for v in variants:
            env = dict(os.environ)
            if v == "a":
                env["PDPLQR_LIB"] = os.path.abspath(a.parent_lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", v], env=env, capture_output=True,
                               text=True, timeout=300)
            if p.returncode != 0:  # nothing more is started after a failure
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                sys.exit(p.returncode or 1)
            r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            runs[v].append(r["solve_ms"])
            for k in extra:
                if k in r:
                    extra[k].append(r[k])
            print(v, r, flush=True)
    s = n + m
    res = {
        "config": {"n": n, "m": m, "N": N, "batch": batch, "rows_per_stage": nc, "solver": "serial", "keep_factors": 1,
                   "iterations": N_ITER, "check_every": CHECK, "eps": 0.0, "adaptive_rho": 0, "rounds": a.rounds},
        "solve_ms": {v: {"median": statistics.median(x), "min": min(x), "max": max(x), "runs": x} for v, x in runs.items()},
        "kernel_ms": {k: statistics.median(x) for k, x in extra.items() if x},
        # compulsory bytes of one primal test: E, c, D, dy (two vectors in the loop), lb, ub
        "primal_bytes_per_stage": 8 * (n * s + n + nc * s + 4 * nc),
        "primal_bytes_per_test": 8 * (n * s + n + nc * s + 4 * nc) * N * batch,
    }
    if "primal_ms" in res["kernel_ms"]:
        res["primal_GBps"] = res["primal_bytes_per_test"] / res["kernel_ms"]["primal_ms"] / 1e6
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
