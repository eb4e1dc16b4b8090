#!/usr/bin/env python3
"""Cost of the adjoint of the penalised x-update (pdplqr_adjoint_rows) at the
conic configuration: N = 512, nx = 12, nu = 4, batch 1024, 4 constraint rows
per stage (none at the terminal), keep_factors = 1, device buffers.

Prints ONE JSON line (and writes it to --out):
  adjoint_rows_ms   pdplqr_adjoint_rows, all eight gradients, gvs given
  adjoint_ms        pdplqr_adjoint, all five gradients, on the same model
                    without rows (the path that existed before)
  rows_kernel_ms    the rows kernel alone (k_adjoint_rows, gD + gg + grho)
  rows_bytes        its compulsory bytes
  copy_ms           a device-to-device copy_ moving the same bytes (read + write), same run
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

from adjoint_bench import HBM_PEAK_GBS, gen  # noqa: E402


def rows_bytes(n, m, N, batch, nc):
    """Compulsory traffic of the rows kernel, all outputs, nc rows on every stage
    k < N: per stage it writes grad D (nc s), grad g and grad rho (2 nc) and
    reads D (nc s), w and v (2 s), rho, g and gvs (3 nc)."""
    s = n + m
    wr = N * (nc * s + 2 * nc)
    rd = N * (nc * s + 2 * s + 3 * nc)
    return 8 * batch * wr, 8 * batch * rd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=512)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--n", type=int, default=12)
    ap.add_argument("--m", type=int, default=4)
    ap.add_argument("--nc", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("adjoint_rows_bench: no GPU (this measurement has no CPU form)")
    from pdplqr import BatchedLQRSolver, lib

    n, m, N, batch, nc = a.n, a.m, a.N, a.batch, a.nc
    s = n + m
    f64 = torch.float64
    dev = torch.device("cuda", 0)
    # one stream for torch and the handles: events recorded on it bracket exactly the handles' work
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    E, c, H, h, x0 = gen(n, m, N, batch, dev)
    ncs = [nc] * N + [0]
    ny, ndD = N * nc, N * nc * s
    D = torch.randn(batch, ndD, dtype=f64, device=dev)
    rho = 0.5 + 19.5 * torch.rand(batch, ny, dtype=f64, device=dev)
    ys, zs, gvs = (torch.randn(batch, ny, dtype=f64, device=dev) for _ in range(3))
    ws0 = torch.zeros(batch, N * s + n, dtype=f64, device=dev)
    rows = BatchedLQRSolver(n, m, N, batch, keep_factors=True, ncs=ncs)
    plain = BatchedLQRSolver(n, m, N, batch, keep_factors=True)
    outs = {}
    for bs, nm in ((rows, "rows"), (plain, "plain")):
        bs.handle.set_stream(stream.cuda_stream)
        bs.set_model(E, c, H, h, D if bs is rows else None)
        if bs is rows:
            bs.update_problem_data(ws0, ys, zs, 1.0 / rho, sigma=1e-6)
            bs.backward(rho)
        else:
            bs.update_problem_data(ws0, sigma=1e-6)
            bs.backward()
        outs[nm] = torch.empty_like(ws0)
        bs.forward(x0, outs[nm])
    torch.cuda.synchronize()
    del E, c, H, h
    gws = torch.randn_like(ws0)
    new = lambda cnt: torch.empty(batch, cnt, dtype=f64, device=dev)  # noqa: E731
    gE, gc, gH, gh, gx = new(N * n * s), new(N * n), new(N * s * s + n * n), new(N * s + n), new(n)
    gD, gg, grho = new(ndD), new(ny), new(ny)
    wr, rd = rows_bytes(n, m, N, batch, nc)
    half = (wr + rd) // 2 // 8
    src = torch.randn(half, dtype=f64, device=dev)
    dst = torch.empty_like(src)
    L = lib()
    L.pdplqr_debug_adjoint_rows.argtypes = [C.c_void_p] * 7
    L.pdplqr_debug_adjoint_rows.restype = C.c_int
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def kernel():
        rc = L.pdplqr_debug_adjoint_rows(rows.handle.h, p(outs["rows"]), p(rho), p(gvs), p(gD), p(gg), p(grho))
        assert rc == 0, L.pdplqr_last_error()

    runs = {
        "adjoint_rows_ms": lambda: rows.adjoint_rows(outs["rows"], rho, gws, gvs, gE, gc, gH, gh, gx, gD, gg, grho),
        "adjoint_ms": lambda: plain.adjoint(outs["plain"], gws, gE, gc, gH, gh, gx),
        "rows_kernel_ms": kernel,
        "copy_ms": lambda: dst.copy_(src),
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
    torch.cuda.synchronize()
    rows.close()  # while their stream is alive
    plain.close()
    res = {"config": {"n": n, "m": m, "N": N, "batch": batch, "nc": nc, "keep_factors": 1, "reps": a.reps},
           "device": torch.cuda.get_device_name(dev)}
    for k, v in times.items():
        res[k] = round(statistics.median(v), 4)
        res[k.replace("_ms", "_min_ms")] = round(min(v), 4)
    res["adjoint_rows_over_adjoint"] = round(res["adjoint_rows_ms"] / res["adjoint_ms"], 3)
    res["rows_bytes"] = wr + rd
    res["rows_bytes_written"] = wr
    res["rows_bytes_read"] = rd
    res["rows_kernel_gbs"] = round((wr + rd) / res["rows_kernel_ms"] / 1e6, 1)
    res["rows_kernel_hbm_fraction"] = round(res["rows_kernel_gbs"] / HBM_PEAK_GBS, 3)
    res["copy_gbs"] = round((wr + rd) / res["copy_ms"] / 1e6, 1)
    res["rows_kernel_over_copy"] = round(res["rows_kernel_ms"] / res["copy_ms"], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
