#!/usr/bin/env python3
"""Cost and gain of the ADMM polish (pdplqr_admm_set_polish) at the conic
configuration: N = 512, nx = 12, nu = 4, batch 1024, 4 constraint rows per stage
(a box on the inputs, none at the terminal), SERIAL, keep_factors = 1, device
buffers, rho fixed.

Prints ONE JSON line (and writes it to --out):
  loose_ms          admm_solve at eps_abs = --eps (1e-3), no polish
  polish_ms         the same with polish on (delta 1e-6, 3 refinement steps)
  tight_ms          admm_solve at eps_abs = --tight-eps, no polish: the accuracy
                    the polish reaches, by iterating
  *_err             max |w - w_ref| over the batch, w_ref = admm_solve at 1e-11
  polish_status     how many problems were accepted / rejected / not attempted
  kkt_ms            pdplqr_admm_kkt_residuals alone (both launches)
  kkt_bytes         its compulsory bytes; copy_ms: a device copy_ of as many
Each time is the median of --reps event-timed calls after --warmup calls, the
calls of the measurements interleaved.  One process, one device; run it under
`timeout`.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pdp-lqr_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from adjoint_bench import HBM_PEAK_GBS  # noqa: E402


def gen(n, m, N, batch, dev, seed=0):
    """Strictly convex problems on stable dynamics (the construction of
    tests/admm_infeas_ref.py::random_packed, for which the loop converges):
    E_k = [B / sqrt(n) | A + 0.02 noise] with |eig(A)| = 0.9, H_k = M M^T / s +
    I / 2, in the boundary layout (column-major per stage)."""
    f64, s = torch.float64, n + m
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    rn = lambda *shape: torch.randn(*shape, dtype=f64, device=dev, generator=g)  # noqa: E731
    A = rn(n, n)
    A = A * (0.9 / torch.linalg.eigvals(A.cpu()).abs().max().item())
    Ek = torch.cat([rn(batch, N, n, m) / n ** 0.5, A + 0.02 * rn(batch, N, n, n)], dim=3)  # [b][k][n][s]
    E = Ek.transpose(2, 3).reshape(batch, -1)  # column-major
    M = rn(batch, N, s, s)
    H = torch.matmul(M, M.transpose(2, 3)) / s + 0.5 * torch.eye(s, dtype=f64, device=dev)
    Mn = rn(batch, n, n)
    HN = torch.matmul(Mn, Mn.transpose(1, 2)) / n + 0.5 * torch.eye(n, dtype=f64, device=dev)
    H = torch.cat([H.reshape(batch, -1), HN.reshape(batch, -1)], dim=1)  # (symmetric: either order)
    return E.contiguous(), 0.1 * rn(batch, N * n), H.contiguous(), rn(batch, N * s + n), rn(batch, n)


def kkt_bytes(n, m, N, batch, nc):
    """Compulsory reads of the two launches, nc rows on every stage k < N.  The
    stage-local half reads H, E, D, h, w, c, x_{k+1} and y, lb, ub; the
    recursion reads H, E, D, h, w and y again (another grid)."""
    s = n + m
    local = N * (s * s + n * s + nc * s + 2 * s + 2 * n + 3 * nc)
    grad = N * (s * s + n * s + nc * s + 2 * s + nc)
    return 8 * batch * local, 8 * batch * grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=512)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--n", type=int, default=12)
    ap.add_argument("--m", type=int, default=4)
    ap.add_argument("--rho", type=float, default=1.0)
    ap.add_argument("--eps", type=float, default=1e-3)
    ap.add_argument("--tight-eps", type=float, default=1e-9)
    ap.add_argument("--max-iter", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("polish_bench: no GPU (this measurement has no CPU form)")
    from pdplqr import BatchedLQRSolver

    n, m, N, batch, nc = a.n, a.m, a.N, a.batch, a.m
    s = n + m
    f64 = torch.float64
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)  # one stream for torch and the handle: the events bracket the handle's work
    torch.cuda.set_stream(stream)
    E, c, H, h, x0 = gen(n, m, N, batch, dev)
    ncs = [nc] * N + [0]
    ny, nw = N * nc, N * s + n
    Dk = torch.zeros(nc, s, dtype=f64, device=dev)
    Dk[:, :m] = torch.eye(m, dtype=f64, device=dev)
    D = Dk.t().reshape(-1).repeat(N).expand(batch, -1).contiguous()  # column-major per stage
    # the box: half the mean |u| of the unconstrained optimum, so that a good part of the rows is active
    plain = BatchedLQRSolver(n, m, N, batch, keep_factors=True)
    plain.handle.set_stream(stream.cuda_stream)
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
    rho = torch.full((batch, ny), a.rho, dtype=f64, device=dev)
    bs = BatchedLQRSolver(n, m, N, batch, keep_factors=True, ncs=ncs)
    bs.handle.set_stream(stream.cuda_stream)
    bs.set_model(E, c, H, h, D)
    w, y, z = (torch.zeros(batch, k, dtype=f64, device=dev) for k in (nw, ny, ny))
    kw = dict(sigma=1e-6, alpha=1.6, max_iter=a.max_iter, check_every=25, eps_rel=0.0, adaptive_rho=False)

    def solve(eps, polish, **over):
        w.zero_(), y.zero_(), z.zero_()
        bs.set_polish(polish)
        return bs.admm_solve(x0, lb, ub, rho, w, y, z, eps_abs=eps, **{**kw, **over})

    ref_info = solve(1e-11, False, max_iter=8000)
    w_ref = w.clone()
    res = {"config": {"n": n, "m": m, "N": N, "batch": batch, "nc": nc, "rho": a.rho, "eps": a.eps,
                      "tight_eps": a.tight_eps, "width": width, "keep_factors": 1, "reps": a.reps},
           "device": torch.cuda.get_device_name(dev),
           "ref_iters_max": int(ref_info["iters"].max()), "ref_converged": int(ref_info["converged"].sum())}
    meas = None

    def kkt():
        nonlocal meas
        meas = bs.kkt_residuals(x0, lb, ub, w, y)

    lo, gr = kkt_bytes(n, m, N, batch, nc)
    src = torch.randn((lo + gr) // 2 // 8, dtype=f64, device=dev)
    dst = torch.empty_like(src)
    runs = {
        "loose_ms": lambda: solve(a.eps, False),
        "polish_ms": lambda: solve(a.eps, True),
        "tight_ms": lambda: solve(a.tight_eps, False),
        "kkt_ms": kkt,
        "copy_ms": lambda: dst.copy_(src),
    }
    times = {k: [] for k in runs}
    for it in range(a.warmup + a.reps):
        for k, fn in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            info = fn()
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                times[k].append(e0.elapsed_time(e1))
            if it == 0 and k in ("loose_ms", "polish_ms", "tight_ms"):
                nm = k[:-3]
                res[nm + "_err"] = float((w - w_ref).abs().max())
                res[nm + "_iters_max"] = int(info["iters"].max())
                res[nm + "_converged"] = int(info["converged"].sum())
                if nm == "polish":
                    pi = bs.polish_info()
                    res["polish_status"] = {str(v): int((pi["status"] == v).sum()) for v in (0, 1, 2)}
                    res["polish_n_active_mean"] = float(pi["n_active"].mean())
                    # an accepted polish is exact only when the active-set guess was right:
                    # per-problem errors of the accepted ones
                    ea = (w - w_ref).abs().amax(dim=1)[torch.tensor(pi["status"] == 1, device=dev)]
                    if ea.numel():
                        res["polish_err_accepted"] = float(ea.max())
                        res["polish_err_accepted_median"] = float(ea.median())
                        res["polish_accepted_below_1e-8"] = int((ea < 1e-8).sum())
                if nm == "loose":
                    res["loose_err_median"] = float((w - w_ref).abs().amax(dim=1).median())
    torch.cuda.synchronize()
    bs.close()  # while its stream is alive
    for k, v in times.items():
        res[k] = round(statistics.median(v), 4)
        res[k.replace("_ms", "_min_ms")] = round(min(v), 4)
        res[k.replace("_ms", "_max_ms")] = round(max(v), 4)
    res["polish_cost_ms"] = round(res["polish_ms"] - res["loose_ms"], 4)
    res["kkt_bytes"] = lo + gr
    res["kkt_gbs"] = round((lo + gr) / res["kkt_ms"] / 1e6, 1)
    res["kkt_hbm_fraction"] = round(res["kkt_gbs"] / HBM_PEAK_GBS, 3)
    res["kkt_over_copy"] = round(res["kkt_ms"] / res["copy_ms"], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
