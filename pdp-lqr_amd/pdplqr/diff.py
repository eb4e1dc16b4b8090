"""Differentiable batched LQ solve for torch (new: the reference has no such layer).

``LQRLayer(n, m, N, batch)`` maps the problem data ``(E, c, H, h, x0)`` --
float64 CUDA tensors in the boundary layout of include/pdplqr.h -- to the
optimum ``ws`` of

    min sum 1/2 w_k^T (H_k + sigma I) w_k + h_k^T w_k
    s.t. x_{k+1} = E_k w_k + c_k,  x_0 = x0

on the serial HIP solver, and is differentiable once: ``backward`` is one call
of ``pdplqr_adjoint`` (an extra solve on the cached factor plus one streamed
gradient pass), which writes only the gradients autograd asks for.  ``H`` is
taken as symmetric; its gradient is the one with respect to the symmetric
matrix.  There is no CPU path.
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
        layer._hd.adjoint(ws, gws.contiguous(), *outs)
        return (None,) + tuple(o.view(shp) if o is not None else None for o, shp in zip(outs, ctx.shapes))


class LQRLayer:
    """``ws = layer(E, c, H, h, x0)``; owns a serial keep_factors handle.

    The handle holds ONE factorization: call ``backward`` on a result before
    the layer is called again (a later ``backward`` raises ``RuntimeError``)."""

    def __init__(self, n: int, m: int, N: int, batch: int, device: int = 0, sigma: float = 0.0):
        self.n, self.m, self.N, self.batch, self.sigma = int(n), int(m), int(N), int(batch), float(sigma)
        s = n + m
        # doubles per problem of E, c, H, h (= ws), x0
        self._per = (N * n * s, N * n, N * s * s + n * n, N * s + n, n)
        self._dev = torch.device("cuda", int(device))
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
