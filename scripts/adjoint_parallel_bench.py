#!/usr/bin/env python3
"""Cost of pdplqr_adjoint_parallel against the primal PARALLEL solve and the
serial adjoint, device buffers, keep_factors = 1, num_segments = 8:

  c2      one N = 1024, 12/4 problem (the README's C2)
  b64     batch 64 x N = 1024, 12/4
  n8192   one N = 8192, 24/8 problem

Per configuration, four cases:
  primal_ms         (a) PARALLEL backward + forward
  adjoint_ms        (b) pdplqr_adjoint_parallel, five outputs
  adjoint_vec_ms    (c) the same with gE = gH = NULL
  serial_adjoint_ms (d) pdplqr_adjoint on a SERIAL handle with the same data
Each figure is the median of --reps event-timed samples after --warmup, one
sample = --inner back-to-back calls on the handle's own stream (which is
torch's current stream: no cross-stream joins) divided by --inner; the four
cases are interleaved sample by sample.  Prints ONE JSON line (and writes it
to --out).  One process, one device; run it under `timeout`.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pdp-lqr_amd"))

import torch  # noqa: E402

CONFIGS = {"c2": (12, 4, 1024, 1), "b64": (12, 4, 1024, 64), "n8192": (24, 8, 8192, 1)}


def gen(n, m, N, batch, dev, seed=0):
    f64, s = torch.float64, n + m
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    E = torch.empty(batch, N, s, n, dtype=f64, device=dev)  # column-major n x s blocks
    E[:, :, :m, :] = torch.randn(batch, N, m, n, dtype=f64, device=dev, generator=g)
    E[:, :, m:, :] = 0.1 * torch.randn(batch, N, n, n, dtype=f64, device=dev, generator=g)
    E[:, :, m:, :] += torch.eye(n, dtype=f64, device=dev)
    c = torch.randn(batch, N * n, dtype=f64, device=dev, generator=g)
    M = torch.randn(batch, N, s, s, dtype=f64, device=dev, generator=g)
    H = torch.empty(batch, N * s * s + n * n, dtype=f64, device=dev)
    H[:, :N * s * s] = (M @ M.transpose(-1, -2) / s + torch.eye(s, dtype=f64, device=dev)).reshape(batch, -1)
    MN = torch.randn(batch, n, n, dtype=f64, device=dev, generator=g)
    H[:, N * s * s:] = (MN @ MN.transpose(-1, -2) / n + torch.eye(n, dtype=f64, device=dev)).reshape(batch, n * n)
    h = torch.randn(batch, N * s + n, dtype=f64, device=dev, generator=g)
    x0 = torch.randn(batch, n, dtype=f64, device=dev, generator=g)
    return E.reshape(batch, -1), c, H, h, x0


def run_config(name, a, dev, stream):
    from pdplqr import BatchedLQRSolver

    n, m, N, batch = CONFIGS[name]
    s = n + m
    E, c, H, h, x0 = gen(n, m, N, batch, dev)
    f64 = torch.float64
    ws0 = torch.zeros(batch, N * s + n, dtype=f64, device=dev)
    gws = torch.randn_like(ws0)
    handles, sols = {}, {}
    for solver in ("parallel", "serial"):
        bs = BatchedLQRSolver(n, m, N, batch, solver=solver, num_segments=8, keep_factors=True)
        bs.handle.set_stream(stream.cuda_stream)
        bs.set_model(E, c, H, h)
        bs.update_problem_data(ws0, sigma=1e-6)
        bs.backward()
        sols[solver] = torch.empty_like(ws0)
        bs.forward(x0, sols[solver])
        handles[solver] = bs
    par, ser = handles["parallel"], handles["serial"]
    outs = {k: [torch.empty(batch, cnt, dtype=f64, device=dev) for cnt in (N * n * s, N * n, N * s * s + n * n, N * s + n, n)]
            for k in ("parallel", "serial")}
    gp, gs = outs["parallel"], outs["serial"]

    def primal():
        par.backward()
        par.forward(x0, sols["parallel"])

    runs = {
        "primal_ms": primal,
        "adjoint_ms": lambda: par.adjoint_parallel(sols["parallel"], gws, *gp),
        "adjoint_vec_ms": lambda: par.adjoint_parallel(sols["parallel"], gws, None, gp[1], None, gp[3], gp[4]),
        "serial_adjoint_ms": lambda: ser.adjoint(sols["serial"], gws, *gs),
    }
    times = {k: [] for k in runs}
    for it in range(a.warmup + a.reps):
        for k, fn in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                fn()
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                times[k].append(e0.elapsed_time(e1) / a.inner)
    torch.cuda.synchronize()
    # the two adjoints on the same data: the figures compare like with like
    par.adjoint_parallel(sols["parallel"], gws, *gp)
    ser.adjoint(sols["serial"], gws, *gs)
    torch.cuda.synchronize()
    agree = max(float(torch.linalg.norm(p - q) / torch.linalg.norm(q)) for p, q in zip(gp, gs))
    import ctypes as C

    from pdplqr import lib
    seg = (C.c_int32 * 2)()
    S = lib().pdplqr_debug_parallel(par.handle.h, 5, seg, C.c_longlong(8))
    ok = bool((par.status() == 0).all()) and bool((ser.status() == 0).all())
    for bs in handles.values():
        bs.close()  # while the stream is alive
    res = {"n": n, "m": m, "N": N, "batch": batch, "device_segments": int(S), "status_ok": ok,
           "parallel_vs_serial_rel": agree}
    for k, v in times.items():
        res[k] = round(statistics.median(v), 4)
        res[k.replace("_ms", "_min_ms")] = round(min(v), 4)
    res["adjoint_over_primal"] = round(res["adjoint_ms"] / res["primal_ms"], 3)
    res["serial_over_parallel_adjoint"] = round(res["serial_adjoint_ms"] / res["adjoint_ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,b64,n8192")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("adjoint_parallel_bench: no GPU (this measurement has no CPU form)")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    res = {"device": torch.cuda.get_device_name(dev), "num_segments": 8, "reps": a.reps, "inner": a.inner,
           "configs": {}}
    for name in a.configs.split(","):
        res["configs"][name] = run_config(name, a, dev, stream)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
