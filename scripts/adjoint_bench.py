#!/usr/bin/env python3
"""Cost of the adjoint solve (pdplqr_adjoint) at the headline configuration:
N = 1024, nx = 12, nu = 4, batch 4096, keep_factors = 1, device buffers.

Prints ONE JSON line (and writes it to --out):
  primal_ms        backward + forward of the handle
  adjoint_ms       pdplqr_adjoint, all five gradients
  adjoint_vec_ms   pdplqr_adjoint with gH = gE = NULL (the vector-only cost)
  grad_kernel_ms   the gradient pass alone (k_adjoint_grad, all five outputs)
  grad_bytes       its compulsory bytes
  copy_ms          a device-to-device copy_ moving the same bytes (read + write), same run
Each time is the median of --reps event-timed calls after --warmup calls, the
calls of the six measurements interleaved.  One process, one device; run it
under `timeout`.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pdp-lqr_amd"))

import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E (bench.py)


def gen(n, m, N, batch, dev, seed=0):
    f64, s = torch.float64, n + m
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    E = torch.empty(batch, N, s, n, dtype=f64, device=dev)  # column-major n x s blocks
    E[:, :, :m, :] = torch.randn(batch, N, m, n, dtype=f64, device=dev, generator=g)
    E[:, :, m:, :] = 0.1 * torch.randn(batch, N, n, n, dtype=f64, device=dev, generator=g)
    E[:, :, m:, :] += torch.eye(n, dtype=f64, device=dev)
    c = torch.randn(batch, N * n, dtype=f64, device=dev, generator=g)
    H = torch.empty(batch, N * s * s + n * n, dtype=f64, device=dev)
    chunk = max(1, (1 << 27) // (N * s * s))
    for b0 in range(0, batch, chunk):
        b1 = min(batch, b0 + chunk)
        M = torch.randn(b1 - b0, N, s, s, dtype=f64, device=dev, generator=g)
        H[b0:b1, :N * s * s] = (M @ M.transpose(-1, -2) / s + torch.eye(s, dtype=f64, device=dev)).reshape(b1 - b0, -1)
        del M
    MN = torch.randn(batch, n, n, dtype=f64, device=dev, generator=g)
    H[:, N * s * s:] = (MN @ MN.transpose(-1, -2) / n + torch.eye(n, dtype=f64, device=dev)).reshape(batch, n * n)
    h = torch.randn(batch, N * s + n, dtype=f64, device=dev, generator=g)
    x0 = torch.randn(batch, n, dtype=f64, device=dev, generator=g)
    return E.reshape(batch, -1), c, H, h, x0


def grad_bytes(n, m, N, batch):
    """Compulsory traffic of the gradient pass, all outputs: per stage it writes
    grad H (s^2), grad E (n s), grad c (n), grad h (s) and reads w, v (2 s),
    Lxx (n (n + 1) / 2), p and p^ (2 n); the terminal adds n^2 + n written and
    2 n read, grad x0 n + n."""
    s = n + m
    wr = N * (s * s + n * s + n + s) + n * n + n + n
    rd = N * (2 * s + n * (n + 1) // 2 + 2 * n) + 2 * n + n
    return 8 * batch * wr, 8 * batch * rd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--n", type=int, default=12)
    ap.add_argument("--m", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("adjoint_bench: no GPU (this measurement has no CPU form)")
    from pdplqr import BatchedLQRSolver, lib

    n, m, N, batch = a.n, a.m, a.N, a.batch
    s = n + m
    dev = torch.device("cuda", 0)
    # one stream for torch and the handle: events recorded on it bracket exactly the handle's work
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    E, c, H, h, x0 = gen(n, m, N, batch, dev)
    bs = BatchedLQRSolver(n, m, N, batch, keep_factors=True)
    hd = bs.handle
    hd.set_stream(stream.cuda_stream)
    bs.set_model(E, c, H, h)
    torch.cuda.synchronize()
    del E, c, H, h
    ws = torch.zeros(batch, N * s + n, dtype=torch.float64, device=dev)
    bs.update_problem_data(ws, sigma=1e-6)
    out = torch.empty_like(ws)
    gws = torch.randn_like(ws)
    gE = torch.empty(batch, N * n * s, dtype=torch.float64, device=dev)
    gc = torch.empty(batch, N * n, dtype=torch.float64, device=dev)
    gH = torch.empty(batch, N * s * s + n * n, dtype=torch.float64, device=dev)
    gh = torch.empty_like(ws)
    gx = torch.empty(batch, n, dtype=torch.float64, device=dev)
    wr, rd = grad_bytes(n, m, N, batch)
    half = (wr + rd) // 2 // 8
    src = torch.randn(half, dtype=torch.float64, device=dev)
    dst = torch.empty_like(src)
    L = lib()
    L.pdplqr_debug_adjoint_grad.argtypes = [C.c_void_p] * 7
    L.pdplqr_debug_adjoint_grad.restype = C.c_int
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def primal():
        bs.backward()
        bs.forward(x0, out)

    def kernel():
        rc = L.pdplqr_debug_adjoint_grad(hd.h, p(out), p(gE), p(gc), p(gH), p(gh), p(gx))
        assert rc == 0, L.pdplqr_last_error()

    runs = {
        "primal_ms": primal,
        "adjoint_ms": lambda: bs.adjoint(out, gws, gE, gc, gH, gh, gx),
        "adjoint_vec_ms": lambda: bs.adjoint(out, gws, None, gc, None, gh, gx),
        "grad_kernel_ms": kernel,
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
    bs.close()  # while its stream is alive
    res = {"config": {"n": n, "m": m, "N": N, "batch": batch, "keep_factors": 1, "reps": a.reps},
           "device": torch.cuda.get_device_name(dev)}
    for k, v in times.items():
        res[k] = round(statistics.median(v), 4)
        res[k.replace("_ms", "_min_ms")] = round(min(v), 4)
    res["grad_bytes"] = wr + rd
    res["grad_bytes_written"] = wr
    res["grad_bytes_read"] = rd
    res["grad_kernel_gbs"] = round((wr + rd) / res["grad_kernel_ms"] / 1e6, 1)
    res["grad_kernel_hbm_fraction"] = round(res["grad_kernel_gbs"] / HBM_PEAK_GBS, 3)
    res["copy_gbs"] = round((wr + rd) / res["copy_ms"] / 1e6, 1)
    res["grad_kernel_over_copy"] = round(res["grad_kernel_ms"] / res["copy_ms"], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
