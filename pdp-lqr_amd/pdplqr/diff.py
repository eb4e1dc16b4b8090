"""Differentiable batched LQ solve for torch (new: the reference has no such layer).

``LQRLayer(n, m, N, batch)`` maps the problem data ``(E, c, H, h, x0)`` --
float64 CUDA tensors in the boundary layout of include/pdplqr.h -- to the
optimum ``ws`` of

    min sum 1/2 w_k^T (H_k + sigma I) w_k + h_k^T w_k
    s.t. x_{k+1} = E_k w_k + c_k,  x_0 = x0

on the serial HIP solver (or, with ``solver="parallel"``, the segmented one),
and is differentiable once: ``backward`` is one call of ``pdplqr_adjoint``
(``pdplqr_adjoint_parallel``): an extra solve on the cached factor plus one
streamed gradient pass, which writes only the gradients autograd asks for.  ``H`` is
taken as symmetric; its gradient is the one with respect to the symmetric
matrix.  There is no CPU path.

``BoxLQRLayer`` (below) is the same for the box-constrained problem
``lb <= D w <= ub`` solved by ``pdplqr_admm_solve``: its backward pass iterates
the adjoint of one ADMM step at the solution, one ``pdplqr_adjoint_rows`` call
on the cached factor per iteration.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .solvers import _Handle


class _LQRSolve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, layer, E, c, H, h, x0):
        ins = [layer._check(t, nm, cnt) for t, nm, cnt in zip((E, c, H, h, x0), ("E", "c", "H", "h", "x0"), layer._per)]
        hd = layer._hd
        hd.set_model(*ins[:4])
        hd.update_problem_data(layer._wbar, None, None, None, layer.sigma)
        hd.backward(None)
        ws = torch.empty(layer.batch, layer._per[3], dtype=torch.float64, device=layer._dev)
        hd.forward(ins[4], ws)
        layer._gen += 1  # the handle now holds THIS call's factorization
        ctx.layer, ctx.gen = layer, layer._gen
        ctx.shapes = [t.shape for t in (E, c, H, h, x0)]
        ctx.save_for_backward(ws)
        return ws

    @staticmethod
    @once_differentiable
    def backward(ctx, gws):
        layer = ctx.layer
        if ctx.gen != layer._gen:
            raise RuntimeError(
                "LQRLayer: backward through a solution whose factorization is gone: the layer was called again "
                f"(call {layer._gen}) after the call being differentiated (call {ctx.gen}), and its handle keeps "
                "one factorization.  Call backward before the next forward, or use one LQRLayer per live graph.")
        (ws,) = ctx.saved_tensors
        outs = [torch.empty(layer.batch, cnt, dtype=torch.float64, device=layer._dev) if need else None
                for cnt, need in zip(layer._per, ctx.needs_input_grad[1:])]
        adjoint = layer._hd.adjoint_parallel if layer.solver == "parallel" else layer._hd.adjoint
        adjoint(ws, gws.contiguous(), *outs)
        return (None,) + tuple(o.view(shp) if o is not None else None for o, shp in zip(outs, ctx.shapes))


class LQRLayer:
    """``ws = layer(E, c, H, h, x0)``; owns a keep_factors handle.

    ``solver="serial"`` (the default) solves on the batched serial kernels and
    differentiates with ``pdplqr_adjoint``.  ``solver="parallel"`` cuts the
    horizon into segments (``num_segments``, ``segment_len``, ``condensed`` as
    for ``BatchedLQRSolver``) and differentiates with
    ``pdplqr_adjoint_parallel``: the choice for one long-horizon problem.

    The handle holds ONE factorization: call ``backward`` on a result before
    the layer is called again (a later ``backward`` raises ``RuntimeError``)."""

    def __init__(self, n: int, m: int, N: int, batch: int, device: int = 0, sigma: float = 0.0,
                 solver: str = "serial", num_segments: int = 2, segment_len: int = 0, condensed: str = "CHOLESKY"):
        self.n, self.m, self.N, self.batch, self.sigma = int(n), int(m), int(N), int(batch), float(sigma)
        if solver not in ("serial", "parallel"):
            raise ValueError(f"LQRLayer: solver must be 'serial' or 'parallel', not {solver!r}")
        self.solver = solver
        s = n + m
        # doubles per problem of E, c, H, h (= ws), x0
        self._per = (N * n * s, N * n, N * s * s + n * n, N * s + n, n)
        self._dev = torch.device("cuda", int(device))
        if solver == "parallel":
            ct = {"LU": _lib.PDPLQR_CONDENSED_LU, "CHOLESKY": _lib.PDPLQR_CONDENSED_CHOLESKY}[condensed]
            self._hd = _Handle(n, m, N, batch, _lib.PDPLQR_SOLVER_PARALLEL, num_segments=num_segments,
                               condensed_type=ct, device=device, keep_factors=True, segment_len=segment_len)
        else:
            self._hd = _Handle(n, m, N, batch, _lib.PDPLQR_SOLVER_SERIAL, device=device, keep_factors=True)
        self._wbar = torch.zeros(batch, self._per[3], dtype=torch.float64, device=self._dev)  # proximal centre
        self._gen = 0

    def _check(self, t, name, per):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.device != self._dev:
            raise TypeError(f"LQRLayer: {name} must be a float64 tensor on {self._dev}")
        if t.numel() != self.batch * per:
            raise ValueError(f"LQRLayer: {name} has {t.numel()} entries, expected batch * {per}")
        return t.detach().contiguous()

    def __call__(self, E, c, H, h, x0):
        return _LQRSolve.apply(self, E, c, H, h, x0)

    @property
    def handle(self) -> _Handle:
        return self._hd

    def close(self):
        self._hd.close()


class _BoxLQRSolve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, layer, E, c, H, h, x0, D, lb, ub):
        names = ("E", "c", "H", "h", "x0", "D", "lb", "ub")
        ins = [layer._check(t, nm, cnt) for t, nm, cnt in zip((E, c, H, h, x0, D, lb, ub), names, layer._per)]
        hd, rho = layer._hd, layer._rho
        hd.set_model(*ins[:4], ins[5])
        new = lambda cnt: torch.zeros(layer.batch, cnt, dtype=torch.float64, device=layer._dev)  # noqa: E731
        ws, ys, zs = new(layer._per[3]), new(layer.ny), new(layer.ny)  # the zero start
        hd.admm_solve(ins[4], ins[6], ins[7], rho, ws, ys, zs, layer._settings)
        layer.admm_info = hd.admm_info()
        if layer.backward_mode == "active_set":
            wt = ws  # (pdplqr_admm_adjoint factors for itself, at the point the solve left in the handle)
        else:
            # one protocol x-update at the returned (w*, y*, z*): the handle's factor, g and
            # lp now belong to the fixed point, whatever path admm_solve's last iteration took
            hd.update_problem_data(ws, ys, zs, layer._irho, layer.sigma)
            hd.backward(rho)
            wt = torch.empty_like(ws)
            hd.forward(ins[4], wt)
        layer._gen += 1  # the handle now holds THIS call's factorization
        ctx.layer, ctx.gen = layer, layer._gen
        ctx.converged = bool(layer.admm_info["converged"].all())
        ctx.infeasible = None  # (index, kind) of the first problem certified infeasible / unbounded
        if layer.detect_infeasible:
            bad = (layer.admm_info["status"] >= _lib.PDPLQR_ADMM_PRIMAL_INFEASIBLE).nonzero()[0]
            if bad.size:
                b = int(bad[0])
                kind = ("primal infeasible (no point satisfies the dynamics and lb <= D w <= ub)"
                        if layer.admm_info["status"][b] == _lib.PDPLQR_ADMM_PRIMAL_INFEASIBLE
                        else "dual infeasible (the cost is unbounded below)")
                ctx.infeasible = (b, kind)
        ctx.shapes = [t.shape for t in (E, c, H, h, x0, D, lb, ub)]
        ctx.save_for_backward(wt, ys, zs, ins[6], ins[7])
        return ws

    @staticmethod
    @once_differentiable
    def backward(ctx, gws):
        layer = ctx.layer
        if ctx.gen != layer._gen:
            raise RuntimeError(
                "BoxLQRLayer: backward through a solution whose factorization is gone: the layer was called again "
                f"(call {layer._gen}) after the call being differentiated (call {ctx.gen}), and its handle keeps "
                "one factorization.  Call backward before the next forward, or use one BoxLQRLayer per live graph.")
        if ctx.infeasible is not None:  # (allow_unconverged does not override: there is no optimum)
            raise RuntimeError(
                f"BoxLQRLayer: problem {ctx.infeasible[0]} of the batch is {ctx.infeasible[1]} (layer.admm_info"
                '["status"]); there is no optimum to differentiate.')
        if layer.backward_mode == "active_set":  # (its own status decides, per problem)
            return _BoxLQRSolve._backward_active_set(ctx, layer, gws.contiguous())
        if not ctx.converged and not layer.allow_unconverged:
            raise RuntimeError(
                "BoxLQRLayer: the ADMM solve being differentiated did not converge for every problem of the batch "
                "(layer.admm_info); the fixed-point adjoint is meaningless there.  Raise max_iter, loosen eps, or "
                "build the layer with allow_unconverged=True.")
        wt, ys, zs, lb, ub = ctx.saved_tensors
        hd, rho, al, sg = layer._hd, layer._rho, layer.alpha, layer.sigma
        tt = zs + ys / rho
        at_lb, at_ub = tt <= lb, tt >= ub
        M = (~(at_lb | at_ub)).to(torch.float64)
        gws = gws.contiguous()
        a_w, a_y, a_z = torch.zeros_like(gws), torch.zeros_like(ys), torch.zeros_like(ys)
        gh, gg = torch.empty_like(gws), torch.empty_like(ys)

        def cotangents():
            b_w = gws + a_w
            q = a_z - rho * a_y
            return b_w, q, rho * a_y + M * q

        # a <- dl/ds + J^T a through one ADMM step at the fixed point s = (w, y, z)
        layer.adjoint_iterations = 0
        for it in range(1, layer.adj_max_iter + 1):
            b_w, q, b_vr = cotangents()
            hd.adjoint_rows(wt, rho, al * b_w, al * b_vr, gh=gh, gg=gg)
            n_w = (1.0 - al) * b_w - sg * gh
            n_y = a_y + M * q / rho - gg / rho
            n_z = (1.0 - al) * b_vr + gg
            test = it % layer.check_every == 0 or it == layer.adj_max_iter
            if test:  # per problem: max-norm change <= adj_tol * max-norm
                ch = torch.cat([(n_w - a_w).abs(), (n_y - a_y).abs(), (n_z - a_z).abs()], dim=1).amax(dim=1)
                nrm = torch.cat([n_w.abs(), n_y.abs(), n_z.abs()], dim=1).amax(dim=1)
            a_w, a_y, a_z = n_w, n_y, n_z
            layer.adjoint_iterations = it
            if test and bool((ch <= layer.adj_tol * nrm).all().item()):
                break

        b_w, q, b_vr = cotangents()
        need = ctx.needs_input_grad[1:]
        outs = [torch.empty(layer.batch, cnt, dtype=torch.float64, device=layer._dev) if nd else None
                for cnt, nd in zip(layer._per[:6], need[:6])]
        if any(o is not None for o in outs):
            hd.adjoint_rows(wt, rho, al * b_w, al * b_vr, *outs)
        outs.append(q * at_lb if need[6] else None)
        outs.append(q * at_ub if need[7] else None)
        return (None,) + tuple(o.view(shp) if o is not None else None for o, shp in zip(outs, ctx.shapes))

    @staticmethod
    def _backward_active_set(ctx, layer, gws):
        """One pdplqr_admm_adjoint call, asking only for what autograd needs."""
        hd = layer._hd
        outs = [torch.empty(layer.batch, cnt, dtype=torch.float64, device=layer._dev) if nd else None
                for cnt, nd in zip(layer._per, ctx.needs_input_grad[1:])]
        hd.admm_adjoint(gws.contiguous(), None, *outs)
        layer.adjoint_info = hd.admm_adjoint_info()
        layer.adjoint_iterations = layer.polish_refine_iter + 1
        bad = (layer.adjoint_info["status"] != _lib.PDPLQR_ADMM_ADJOINT_EXACT).nonzero()[0]
        if bad.size and not layer.allow_unconverged:
            b = int(bad[0])
            why = ("the factorisation at the solution failed" if layer.adjoint_info["status"][b] ==
                   _lib.PDPLQR_ADMM_ADJOINT_FAILED else "its polish was rejected or the solve did not converge")
            raise RuntimeError(
                f"BoxLQRLayer: problem {b} of the batch has no exact active-set gradient ({why}; "
                "layer.adjoint_info, layer.admm_info).  Raise max_iter, tighten eps, or build the layer with "
                "allow_unconverged=True.")
        return (None,) + tuple(o.view(shp) if o is not None else None for o, shp in zip(outs, ctx.shapes))


class BoxLQRLayer:
    """``ws = layer(E, c, H, h, x0, D, lb, ub)``: the optimum of

        min sum 1/2 w_k^T H_k w_k + h_k^T w_k
        s.t. x_{k+1} = E_k w_k + c_k,  x_0 = x0,  lb <= D w <= ub

    by ``pdplqr_admm_solve`` from a zero start (rows per stage ``ncs``, N + 1
    counts), differentiable once in all eight inputs (float64 CUDA tensors in
    the boundary layout of include/pdplqr.h).

    ``rho`` (a number, or ``[batch][ny]`` values) is fixed: adaptive rho is off,
    the backward pass assumes the rho the solve ended with.  ``eps`` is the
    absolute tolerance of the ADMM residuals (``eps_rel`` = 0).  ``backward`` is
    a fixed-point adjoint iteration through one ADMM step at the solution, one
    ``pdplqr_adjoint_rows`` call on the cached factor per iteration, until the
    max-norm change of the adjoint state is at most ``adj_tol`` times its
    max-norm for every problem (tested every ``check_every`` iterations with one
    small device-to-host read) or ``adj_max_iter`` is reached; it needs about
    as many iterations as the forward solve.  The gradients are those of the
    optimum when it is strictly complementary.  ``backward`` raises
    ``RuntimeError`` if a problem did not converge (unless
    ``allow_unconverged``), or if the layer was called again in between (the
    handle keeps ONE factorization).  ``admm_info`` holds the last solve's
    outcome, ``adjoint_iterations`` the last backward's count.

    ``detect_infeasible``: run OSQP's infeasibility certificates in the solve
    (``admm_info["status"]``: 2 = no feasible point, 3 = cost unbounded below);
    ``backward`` then raises ``RuntimeError`` naming the first such problem and
    its kind, before the "did not converge" error and whatever
    ``allow_unconverged`` says.

    ``polish``: polish the solve (``pdplqr_admm_set_polish``): a problem whose
    polished point passes OSQP's acceptance rule returns the optimum on its
    active set instead of the ``eps``-accurate iterate
    (``admm_info["polish_status"]``: 1 accepted, 2 rejected), so a loose
    ``eps`` gives what thousands of iterations at a tight one gave.  The
    explicit x-update the backward pass differentiates through then runs at
    the polished ``(w, y, z)``, which is a fixed point of the ADMM step.

    ``backward_mode``: ``"fixed_point"`` (the default) is the iteration above.
    ``"active_set"`` (needs ``polish=True``) differentiates the optimum exactly
    on the active set the polish guessed: ``backward`` is one
    ``pdplqr_admm_adjoint`` call -- ``polish_refine_iter + 1`` solves on the
    factor of the polishing system, no host round trip, accuracy independent
    of ``eps`` and ``adj_tol`` -- and ``forward`` skips
    the explicit x-update.  It raises ``RuntimeError`` naming the first problem
    whose gradient is not exact (``adjoint_info["status"]`` != 1: polish
    rejected, solve not converged, or a failed factorisation) unless
    ``allow_unconverged``.  A row with ``lb == ub`` sends its whole gradient to
    ``lb`` in this mode; the fixed-point mode sends it to both ``lb`` and ``ub``."""

    def __init__(self, n: int, m: int, N: int, batch: int, ncs, rho, sigma: float = 1e-6, alpha: float = 1.6,
                 eps: float = 1e-6, max_iter: int = 4000, adj_tol: float = 1e-8, adj_max_iter: int = 4000,
                 check_every: int = 25, allow_unconverged: bool = False, device: int = 0,
                 detect_infeasible: bool = False, eps_prim_inf: float = 1e-4, eps_dual_inf: float = 1e-4,
                 polish: bool = False, polish_delta: float = 1e-6, polish_refine_iter: int = 3,
                 backward_mode: str = "fixed_point"):
        from .solvers import admm_settings

        if backward_mode not in ("fixed_point", "active_set"):
            raise ValueError('BoxLQRLayer: backward_mode is "fixed_point" or "active_set"')
        if backward_mode == "active_set" and not polish:
            raise ValueError('BoxLQRLayer: backward_mode="active_set" requires polish=True')
        self.backward_mode = backward_mode
        self.polish_refine_iter = int(polish_refine_iter)
        self.adjoint_info = None

        self.n, self.m, self.N, self.batch = int(n), int(m), int(N), int(batch)
        self.sigma, self.alpha = float(sigma), float(alpha)
        self.adj_tol, self.adj_max_iter, self.check_every = float(adj_tol), int(adj_max_iter), int(check_every)
        self.allow_unconverged = bool(allow_unconverged)
        self.detect_infeasible = bool(detect_infeasible)
        s = n + m
        ncs = [int(x) for x in ncs]
        if len(ncs) != N + 1:
            raise ValueError("BoxLQRLayer: ncs needs N + 1 entries")
        self.ny = sum(ncs)
        if self.ny == 0:
            raise ValueError("BoxLQRLayer: no constraint rows (use LQRLayer)")
        ndD = sum(nc * (s if k < N else n) for k, nc in enumerate(ncs))
        # doubles per problem of E, c, H, h (= ws), x0, D, lb, ub
        self._per = (N * n * s, N * n, N * s * s + n * n, N * s + n, n, ndD, self.ny, self.ny)
        self._dev = torch.device("cuda", int(device))
        self._hd = _Handle(n, m, N, batch, _lib.PDPLQR_SOLVER_SERIAL, device=device, keep_factors=True, ncs=ncs)
        rho = torch.as_tensor(rho, dtype=torch.float64).detach().to(self._dev)
        self._rho = (rho.expand(batch, self.ny) if rho.numel() == 1 else rho.reshape(batch, self.ny)).contiguous()
        self._irho = (1.0 / self._rho).contiguous()
        self._settings = admm_settings(sigma, alpha, max_iter, check_every, eps, 0.0, False)
        if self.detect_infeasible:
            self._hd.set_infeasibility_detection(True, eps_prim_inf, eps_dual_inf)
        self.polish = bool(polish)
        if self.polish:
            self._hd.set_polish(True, polish_delta, polish_refine_iter)
        self._gen = 0
        self.admm_info = None
        self.adjoint_iterations = 0

    def _check(self, t, name, per):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.device != self._dev:
            raise TypeError(f"BoxLQRLayer: {name} must be a float64 tensor on {self._dev}")
        if t.numel() != self.batch * per:
            raise ValueError(f"BoxLQRLayer: {name} has {t.numel()} entries, expected batch * {per}")
        return t.detach().contiguous().view(self.batch, per)

    def __call__(self, E, c, H, h, x0, D, lb, ub):
        return _BoxLQRSolve.apply(self, E, c, H, h, x0, D, lb, ub)

    @property
    def handle(self) -> _Handle:
        return self._hd

    def close(self):
        self._hd.close()


class _ConeLQRSolve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, layer, E, c, H, h, x0, D, lb, ub):
        # BoxLQRLayer's forward protocol in its fixed-point mode (the solve from a zero start, then the
        # explicit x-update at the returned point); the handle projects onto the layer's cones
        return _BoxLQRSolve.forward(ctx, layer, E, c, H, h, x0, D, lb, ub)

    @staticmethod
    @once_differentiable
    def backward(ctx, gws):
        layer = ctx.layer
        if ctx.gen != layer._gen:
            raise RuntimeError(
                "ConeLQRLayer: backward through a solution whose factorization is gone: the layer was called again "
                f"(call {layer._gen}) after the call being differentiated (call {ctx.gen}), and its handle keeps "
                "one factorization.  Call backward before the next forward, or use one ConeLQRLayer per live graph.")
        if not ctx.converged and not layer.allow_unconverged:
            raise RuntimeError(
                "ConeLQRLayer: the ADMM solve being differentiated did not converge for every problem of the batch "
                "(layer.admm_info); the fixed-point adjoint is meaningless there.  Raise max_iter, loosen eps, or "
                "build the layer with allow_unconverged=True.")
        wt, ys, zs, lb, ub = ctx.saved_tensors
        outs = [torch.empty(layer.batch, cnt, dtype=torch.float64, device=layer._dev) if nd else None
                for cnt, nd in zip(layer._per, ctx.needs_input_grad[1:])]
        hd = layer._hd
        hd.admm_adjoint_fixed_point(wt, ys, zs, lb, ub, layer._rho, gws.contiguous(), layer.sigma, layer.alpha,
                                    layer.adj_tol, layer.adj_max_iter, layer.check_every, *outs)
        layer.adjoint_info = hd.admm_adjoint_fixed_point_info()
        layer.adjoint_iterations = int(layer.adjoint_info["iters"].max())
        return (None,) + tuple(o.view(shp) if o is not None else None for o, shp in zip(outs, ctx.shapes))


class ConeLQRLayer(BoxLQRLayer):
    """``ws = layer(E, c, H, h, x0, D, lb, ub)``: ``BoxLQRLayer``'s problem with
    some rows of a stage forming second-order cones,

        min sum 1/2 w_k^T H_k w_k + h_k^T w_k
        s.t. x_{k+1} = E_k w_k + c_k,  x_0 = x0,
             lb <= D w <= ub on the rows in no cone,
             (D w - lb) in {(t, x): |x| <= t} on the rows of each cone,

    differentiable once in all eight inputs.  ``cones`` is a list of
    ``(stage, row, dim)`` as for ``set_cones`` (sorted by stage, then row; an
    empty list gives ``BoxLQRLayer``'s problem); ``ub`` of a cone row is not
    read and its gradient is zero.  ``rho`` must be constant within a cone.

    A ``BoxLQRLayer`` in its fixed-point mode (its constructor, argument checks
    and forward: ``pdplqr_admm_solve`` from a zero start at the fixed ``rho``,
    then the explicit x-update at the returned point) whose handle carries the
    cones and whose backward is ONE ``pdplqr_admm_adjoint_fixed_point`` call:
    the fixed-point adjoint of DESIGN.md section 5.11 iterated on the device
    until every problem's max-norm change is at most ``adj_tol`` times its
    max-norm (tested every ``check_every`` iterations; a problem that passes is
    frozen) or ``adj_max_iter``, writing only the gradients autograd asks for.
    The gradients are those of the optimum where the projection is
    differentiable (no cone argument on a face or at the apex, box rows
    strictly complementary).  ``backward`` raises ``RuntimeError`` if a problem
    did not converge (unless ``allow_unconverged``) or the layer was called
    again in between (the handle keeps ONE factorization).  ``admm_info`` holds
    the last solve's outcome, ``adjoint_info`` the last backward's per-problem
    ``iters`` / ``converged`` / ``resid``, ``adjoint_iterations`` its largest
    iteration count.  Polish, infeasibility detection and the active-set
    backward are statements about box rows and are not offered here."""

    def __init__(self, n: int, m: int, N: int, batch: int, ncs, rho, cones=(), sigma: float = 1e-6,
                 alpha: float = 1.6, eps: float = 1e-6, max_iter: int = 4000, adj_tol: float = 1e-8,
                 adj_max_iter: int = 4000, check_every: int = 25, allow_unconverged: bool = False, device: int = 0):
        super().__init__(n, m, N, batch, ncs, rho, sigma=sigma, alpha=alpha, eps=eps, max_iter=max_iter,
                         adj_tol=adj_tol, adj_max_iter=adj_max_iter, check_every=check_every,
                         allow_unconverged=allow_unconverged, device=device)
        self.cones = [tuple(int(x) for x in cn) for cn in cones]
        if self.cones:
            self._hd.set_cones(self.cones)

    def __call__(self, E, c, H, h, x0, D, lb, ub):
        return _ConeLQRSolve.apply(self, E, c, H, h, x0, D, lb, ub)
