"""Reference gradients of the penalised x-update and of the box-constrained
solve for the adjoint_rows / BoxLQRLayer tests (CPU, torch float64).

Extends tests/adjoint_ref.py: the dense KKT system of ONE problem is assembled
in torch from the boundary-layout arrays, with the stage problem

    H~_k = sym(H_k) + sigma I + D_k^T diag(rho_k) D_k
    h~_k = h_k - sigma wbar_k - D_k^T (rho_k o g_k)

built in torch from (H, D, rho, g, wbar, sigma), so autograd reaches D, g and
rho as leaves.  ``admm_step`` restates one iteration of the ADMM of
csrc/admm.hip's header on the same dense solve, and ``active_set_solution``
solves the box-constrained problem's KKT system with its active rows as
equalities.  Nothing here comes from the product or the oracle.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import adjoint_ref

F64 = torch.float64
ROW_KEYS = ("gE", "gc", "gH", "gh", "gx", "gD", "gg", "grho")


def offsets(n, m, N, ncs):
    """(d_off, y_off): N + 2 entries each, as the handle's tables."""
    s = n + m
    d_off, y_off = [0], [0]
    for k, nc in enumerate(ncs):
        d_off.append(d_off[-1] + int(nc) * (s if k < N else n))
        y_off.append(y_off[-1] + int(nc))
    return d_off, y_off


def dense_D(D, n, m, N, ncs):
    """The ny x (N s + n) matrix of all rows from the flat column-major blocks."""
    s = n + m
    d_off, y_off = offsets(n, m, N, ncs)
    Df = torch.zeros(y_off[-1], N * s + n, dtype=F64)
    for k, nc in enumerate(ncs):
        d = s if k < N else n
        if nc:
            Df[y_off[k]:y_off[k + 1], k * s:k * s + d] = D[d_off[k]:d_off[k + 1]].view(d, int(nc)).t()
    return Df


def kkt_system(E, c, H, h, x0):
    """(K, r, nw) of adjoint_ref.dense_kkt_solution: K [w; lambda] = r."""
    n, m, N = adjoint_ref._dims(c, h, x0)
    s = n + m
    nw = N * s + n
    dim = nw + (N + 1) * n
    K = torch.zeros(dim, dim, dtype=F64)
    r = torch.zeros(dim, dtype=F64)
    for k in range(N + 1):
        d = s if k < N else n
        o = k * s
        Hk = H[k * s * s:k * s * s + d * d].view(d, d).t()
        K[o:o + d, o:o + d] = 0.5 * (Hk + Hk.t())
    r[:nw] = -h
    eye = torch.eye(n, dtype=F64)
    K[nw:nw + n, m:s] = eye
    K[m:s, nw:nw + n] = eye
    r[nw:nw + n] = x0
    for k in range(N):
        Ek = E[k * n * s:(k + 1) * n * s].view(s, n).t()
        row = nw + (k + 1) * n
        xo = (k + 1) * s + (m if k + 1 < N else 0)
        K[row:row + n, xo:xo + n] = eye
        K[xo:xo + n, row:row + n] = eye
        K[row:row + n, k * s:(k + 1) * s] = -Ek
        K[k * s:(k + 1) * s, row:row + n] = -Ek.t()
        r[row:row + n] = c[k * n:(k + 1) * n]
    return K, r, nw


def penalised_system(E, c, H, h, x0, Df, rho, g, wbar, sigma):
    """The KKT system of the x-update: H~, h~ in place of H, h."""
    K, r, nw = kkt_system(E, c, H, h, x0)
    Kp = K.clone()
    Kp[:nw, :nw] = K[:nw, :nw] + sigma * torch.eye(nw, dtype=F64) + Df.t() @ (rho[:, None] * Df)
    rp = r.clone()
    rp[:nw] = r[:nw] + sigma * wbar + Df.t() @ (rho * g)
    return Kp, rp, nw


def x_update(E, c, H, h, x0, Df, rho, g, wbar, sigma):
    Kp, rp, nw = penalised_system(E, c, H, h, x0, Df, rho, g, wbar, sigma)
    return torch.linalg.solve(Kp, rp)[:nw]


def random_rows(n, m, N, batch, ncs, seed):
    """D dense standard normal, rho in [0.5, 20], ys, zs, gvs standard normal;
    inv_rho = 1 / rho."""
    rng = np.random.default_rng(seed + 77)
    d_off, y_off = offsets(n, m, N, ncs)
    D = rng.standard_normal((batch, d_off[-1]))
    rho = rng.uniform(0.5, 20.0, (batch, y_off[-1]))
    ys = rng.standard_normal((batch, y_off[-1]))
    zs = rng.standard_normal((batch, y_off[-1]))
    gvs = rng.standard_normal((batch, y_off[-1]))
    return D, rho, ys, zs, gvs


@functools.lru_cache(maxsize=None)
def case(n, m, N, batch, ncs, seed=0, sigma=0.0):
    """One random batch with rows and its reference gradients (computed once per
    session; callers must not modify the arrays).  ``ncs`` is a tuple of N + 1
    counts.  Leaves of the autograd: E, c, H, h, x0, D, g, rho."""
    E, c, H, h, x0, gws = adjoint_ref.random_problem(n, m, N, batch, seed)
    D, rho, ys, zs, gvs = random_rows(n, m, N, batch, ncs, seed)
    irho = 1.0 / rho
    g = zs - irho * ys
    wbar = np.zeros_like(h)
    if sigma != 0.0:
        wbar = np.random.default_rng(seed + 1000).standard_normal(h.shape)
    out = {k: [] for k in ("ws",) + ROW_KEYS}
    t = lambda a, rg=False: torch.tensor(a, dtype=F64, requires_grad=rg)  # noqa: E731
    for b in range(batch):
        lv = [t(a[b], True) for a in (E, c, H, h, x0, D, g, rho)]
        Df = dense_D(lv[5], n, m, N, ncs)
        w = x_update(*lv[:5], Df, lv[7], lv[6], t(wbar[b]), sigma)
        loss = (t(gws[b]) * w).sum() + (t(gvs[b]) * (Df @ w)).sum()
        grads = torch.autograd.grad(loss, lv, allow_unused=True)
        out["ws"].append(w.detach().numpy())
        for key, gr, leaf in zip(ROW_KEYS, grads, lv):
            out[key].append((gr if gr is not None else torch.zeros_like(leaf)).numpy())
    return dict(E=E, c=c, H=H, h=h, x0=x0, D=D, rho=rho, irho=irho, ys=ys, zs=zs, g=g, gws=gws, gvs=gvs, wbar=wbar,
                sigma=sigma, ncs=np.asarray(ncs, dtype=np.int32), **{k: np.stack(v) for k, v in out.items()})


# ---- the box-constrained problem (BoxLQRLayer) --------------------------------

def admm_step(E, c, H, h, x0, D, lb, ub, w, y, z, rho, sigma, alpha, dims):
    """One iteration of csrc/admm.hip's header, differentiable: (w+, y+, z+)."""
    n, m, N, ncs = dims
    Df = dense_D(D, n, m, N, ncs)
    wt = x_update(E, c, H, h, x0, Df, rho, z - y / rho, w, sigma)
    vrel = alpha * (Df @ wt) + (1.0 - alpha) * z
    wn = alpha * wt + (1.0 - alpha) * w
    zn = torch.minimum(torch.maximum(vrel + y / rho, lb), ub)
    yn = y + rho * (vrel - zn)
    return wn, yn, zn


def admm_solve(E, c, H, h, x0, D, lb, ub, rho, sigma, alpha, dims, tol=1e-14, max_iter=20000, eps_abs=None,
               check_every=25):
    """The fixed point (w, y, z) of admm_step from a zero start and the
    iterations taken.  Stops when the max-norm change of the iterate is <= tol,
    or, with ``eps_abs``, by pdplqr_admm_solve's test with eps_rel = 0 every
    ``check_every`` iterations: |D w+ - z+|_inf and |D^T rho o (z+ - z)|_inf
    both <= eps_abs."""
    n, m, N, ncs = dims
    with torch.no_grad():
        Df = dense_D(D, n, m, N, ncs)
        ny = Df.shape[0]
        Kp, _, nw = penalised_system(E, c, H, h, x0, Df, rho, torch.zeros(ny, dtype=F64), torch.zeros(Df.shape[1], dtype=F64), sigma)
        Ki = torch.linalg.inv(Kp)
        _, r0, _ = kkt_system(E, c, H, h, x0)
        w, y, z = torch.zeros(nw, dtype=F64), torch.zeros(ny, dtype=F64), torch.zeros(ny, dtype=F64)
        for it in range(1, max_iter + 1):
            r = r0.clone()
            r[:nw] = r0[:nw] + sigma * w + Df.t() @ (rho * (z - y / rho))
            wt = (Ki @ r)[:nw]
            vrel = alpha * (Df @ wt) + (1.0 - alpha) * z
            wn = alpha * wt + (1.0 - alpha) * w
            zn = torch.minimum(torch.maximum(vrel + y / rho, lb), ub)
            yn = y + rho * (vrel - zn)
            if eps_abs is None:
                stop = max((wn - w).abs().max().item(), (yn - y).abs().max().item(), (zn - z).abs().max().item()) <= tol
            else:
                stop = (it % check_every == 0 and (Df @ wn - zn).abs().max().item() <= eps_abs
                        and (Df.t() @ (rho * (zn - z))).abs().max().item() <= eps_abs)
            w, y, z = wn, yn, zn
            if stop:
                break
    return w, y, z, it


def active_set_solution(E, c, H, h, x0, D, lb, ub, at_lb, at_ub, dims):
    """ws of min 1/2 w^T H w + h^T w s.t. dynamics and D_i w = lb_i (rows in
    at_lb), = ub_i (rows in at_ub): the box-constrained optimum when those are
    its active rows.  Differentiable in all eight inputs."""
    n, m, N, ncs = dims
    K, r, nw = kkt_system(E, c, H, h, x0)
    Df = dense_D(D, n, m, N, ncs)
    idx = torch.tensor(np.flatnonzero(at_lb | at_ub), dtype=torch.long)
    A = Df[idx]
    bnd = torch.where(torch.tensor(at_lb), lb, ub)[idx]
    na, dim = A.shape[0], K.shape[0]
    Ka = torch.zeros(dim + na, dim + na, dtype=F64)
    Ka[:dim, :dim] = K
    Ka[dim:, :nw] = A
    Ka[:nw, dim:] = A.t()
    return torch.linalg.solve(Ka, torch.cat([r, bnd]))[:nw]


BOX_KEYS = ("E", "c", "H", "h", "x0", "D", "lb", "ub")


def box_problem(n, m, N, seed, width=0.4):
    """One problem with u-box rows (D_k = [I_m 0], k < N; none at the terminal):
    numpy arrays of BOX_KEYS plus gws, and dims = (n, m, N, ncs)."""
    E, c, H, h, x0, g = adjoint_ref.random_problem(n, m, N, 1, seed)
    s = n + m
    ncs = tuple([m] * N + [0])
    Dk = np.zeros((m, s))
    Dk[:, :m] = np.eye(m)
    D = np.tile(Dk.reshape(-1, order="F"), N)
    lb, ub = -width * np.ones(N * m), width * np.ones(N * m)
    return dict(E=E[0], c=c[0], H=H[0], h=h[0], x0=x0[0], D=D, lb=lb, ub=ub, gws=g[0]), (n, m, N, ncs)


@functools.lru_cache(maxsize=None)
def box_case(n, m, N, seed, rho=10.0, sigma=1e-6, alpha=1.6, eps_abs=None, max_iter=20000):
    """box_problem solved to its ADMM fixed point (admm_solve's stopping rules),
    with the active set read off it, the strict-complementarity margin and the
    active-set autograd gradients of sum(gws * ws) for all eight inputs."""
    p, dims = box_problem(n, m, N, seed)
    t = {k: torch.tensor(p[k], dtype=F64, requires_grad=True) for k in BOX_KEYS}
    rho_t = torch.full((N * m,), rho, dtype=F64)
    w, y, z, iters = admm_solve(*[t[k].detach() for k in BOX_KEYS], rho_t, sigma, alpha, dims, eps_abs=eps_abs,
                                max_iter=max_iter)
    y, z = y.numpy(), z.numpy()
    at_lb, at_ub = y < -1e-9, y > 1e-9
    act = at_lb | at_ub
    margin = min(np.abs(y[act]).min() if act.any() else np.inf,
                 np.minimum(z - p["lb"], p["ub"] - z)[~act].min() if (~act).any() else np.inf)
    ws = active_set_solution(*[t[k] for k in BOX_KEYS], at_lb, at_ub, dims)
    grads = torch.autograd.grad((torch.tensor(p["gws"]) * ws).sum(), [t[k] for k in BOX_KEYS])
    return dict(p, dims=dims, w=w.numpy(), y=y, z=z, iters=iters, at_lb=at_lb, at_ub=at_ub, margin=float(margin),
                ws=ws.detach().numpy(), rho=rho, sigma=sigma, alpha=alpha,
                grads={k: gr.numpy() for k, gr in zip(BOX_KEYS, grads)})


# The worst gradient error tests/test_adjoint_rows_cpu.py::test_recursion_at_layer_settings
# measures on the CPU at the GPU layer test's stopping rules (checked there within
# a factor 2; tests/test_gpu_box_layer.py allows 10 times this)
LAYER_CPU_ERR = {(3, 2, 6): 2.3e-12, (12, 4, 4): 3.0e-10}
# ... and the worst error of the solution itself against the active-set optimum there
LAYER_CPU_WS_ERR = {(3, 2, 6): 3.9e-13, (12, 4, 4): 2.8e-10}
