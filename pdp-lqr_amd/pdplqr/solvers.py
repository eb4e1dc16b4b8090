"""Host-side mirror of the reference solver classes over the C ABI.

Same names, arguments and protocol as the reference (C++ namespace ``lqr``):

* ``LQRSolver(model)``                                   lqr_solver.hpp:9-77
* ``LQRParallelSolver(model, num_segments, load_balancing=True,
  solver_type=CondensedSystemSolverType.CHOLESKY)``      lqr_solver_parallel.hpp:19-238
* ``QDLDLSolver(model)``                                 qdldl_solver.hpp:14-151

each with ``update_problem_data(ws, ys, zs, inv_rho_vecs, sigma)``,
``backward(rho_vecs)`` (``QDLDLSolver``: ``inv_rho_vecs``),
``backward_without_factorization(rho_vecs)`` (Riccati solvers),
``forward(x0, ws)`` (writes ``ws`` in place, as the reference's
``std::vector<VectorXs>&``) and ``clear_workspace()``.  All compute runs in
HIP kernels on the MI355X (libpdplqr.so); there is no CPU fallback.

``BatchedLQRSolver`` is the batched entry point the reference lacks: ``batch``
independent problems of one shape, host numpy or device (torch) buffers.
"""
from __future__ import annotations

import atexit
import ctypes as C
import enum
import weakref
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import AdmmSettings, Config, check, lib
from .model import LQRModel, pack_model, pack_stage_vectors, w_sizes


class CondensedSystemSolverType(enum.IntEnum):
    """lqr_solver_parallel.hpp:14-17"""

    LU = _lib.PDPLQR_CONDENSED_LU
    CHOLESKY = _lib.PDPLQR_CONDENSED_CHOLESKY


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch") and hasattr(x, "data_ptr")


def _ptr(x, what: str):
    """(pointer, mem) for a float64 contiguous numpy array or torch tensor."""
    if x is None:
        return None, None
    if _is_torch(x):
        import torch

        if x.dtype != torch.float64 or not x.is_contiguous():
            raise TypeError(f"{what}: torch tensor must be float64 and contiguous")
        mem = _lib.PDPLQR_MEM_DEVICE if x.is_cuda else _lib.PDPLQR_MEM_HOST
        return C.c_void_p(x.data_ptr()), mem
    a = x
    if not isinstance(a, np.ndarray) or a.dtype != np.float64 or not a.flags["C_CONTIGUOUS"]:
        raise TypeError(f"{what}: expected a C-contiguous float64 numpy array")
    return C.c_void_p(a.ctypes.data), _lib.PDPLQR_MEM_HOST


def _mem_of(*ps):
    mems = {m for (_, m) in ps if m is not None}
    if len(mems) > 1:
        raise TypeError("mixing host and device buffers in one call")
    return mems.pop() if mems else _lib.PDPLQR_MEM_HOST


_LIVE = weakref.WeakSet()  # open handles, closed by _close_all at interpreter exit
_ATEXIT = False


def _close_all():
    """Destroy every handle still open when the interpreter exits, while the
    HIP runtime (torch's, which libpdplqr.so binds to) is fully alive: this
    hook is registered after torch is imported, so it runs before torch's own
    exit hooks and long before the runtime's static destructors in exit()
    (teardown order)."""
    for hd in list(_LIVE):
        try:
            hd.close()
        except Exception:
            pass


class _Handle:
    """Owns one pdplqr_handle."""

    def __init__(self, nx, nu, N, batch=1, solver=_lib.PDPLQR_SOLVER_SERIAL, num_segments=1, load_balancing=True,
                 condensed_type=_lib.PDPLQR_CONDENSED_CHOLESKY, device=0, keep_factors=True, ncs=None,
                 rho_dyn=1e-6, kkt_sigma=1e-6, segment_len=0, devices=None):
        L = lib()
        cfg = Config()
        L.pdplqr_config_init(C.byref(cfg))
        cfg.nx, cfg.nu, cfg.N, cfg.batch = int(nx), int(nu), int(N), int(batch)
        cfg.solver = int(solver)
        cfg.num_segments = int(num_segments)
        cfg.load_balancing = int(bool(load_balancing))
        cfg.condensed_type = int(condensed_type)
        cfg.device = int(device)
        cfg.keep_factors = int(bool(keep_factors))
        cfg.rho_dyn = float(rho_dyn)
        cfg.kkt_sigma = float(kkt_sigma)
        cfg.segment_len = int(segment_len)
        self._devs = None
        if devices is not None and len(devices) > 0:
            # the horizon split over the listed GPUs by this one handle
            # (multidev.hip; one entry: the same split with one slice)
            self._devs = np.ascontiguousarray(np.asarray(devices, dtype=np.int32))
            cfg.num_devices = int(self._devs.size)
            cfg.devices = self._devs.ctypes.data_as(C.POINTER(C.c_int32))
        self._ncs = None
        if ncs is not None:
            self._ncs = np.ascontiguousarray(np.asarray(ncs, dtype=np.int32))
            cfg.ncs = self._ncs.ctypes.data_as(C.POINTER(C.c_int32))
        self.cfg = cfg
        h = C.c_void_p()
        check(L.pdplqr_create(C.byref(cfg), C.byref(h)))
        self.h = h
        global _ATEXIT
        if not _ATEXIT:  # (lib() imported torch first: this hook runs before torch's)
            atexit.register(_close_all)
            _ATEXIT = True
        _LIVE.add(self)
        self.nx, self.nu, self.N, self.batch = int(nx), int(nu), int(N), int(batch)
        self.ncs = self._ncs if self._ncs is not None else np.zeros(N + 1, dtype=np.int32)
        self.ny = int(np.sum(self.ncs))
        self._polish = self._polish_ran = False  # set_polish's state; the last admm_solve ran with it on

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            lib().pdplqr_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # stream ordering with torch ---------------------------------------------
    # The handle launches on its own (non-blocking) stream.  When a call is
    # handed torch CUDA tensors, that stream first waits for torch's current
    # stream (the tensors may have been written there), and torch's current
    # stream waits for the handle's work after the call (outputs are read
    # there, inputs may be freed or overwritten there): events only, no host
    # synchronisation.  Host (numpy) calls are synchronous in the C ABI.
    def _torch_stream(self):
        import torch

        hs = getattr(self, "_ts", None)
        if hs is None:
            hs = self._ts = torch.cuda.ExternalStream(self.stream(), device=torch.device("cuda", self.cfg.device))
        return hs

    def _enter(self, *objs):
        if not any(o is not None and _is_torch(o) and o.is_cuda for o in objs):
            return None
        import torch

        hs = self._torch_stream()
        cur = torch.cuda.current_stream(hs.device)
        if cur.cuda_stream == hs.cuda_stream:
            return None
        hs.wait_stream(cur)
        return cur

    def _leave(self, cur):
        if cur is not None:
            cur.wait_stream(self._torch_stream())

    # raw protocol (pointers already validated) -----------------------------
    def set_model(self, E, c, H, h, D=None):
        ps = [_ptr(E, "E"), _ptr(c, "c"), _ptr(H, "H"), _ptr(h, "h"), _ptr(D, "D")]
        mem = _mem_of(*ps)
        cur = self._enter(E, c, H, h, D)
        check(lib().pdplqr_set_model(self.h, ps[0][0], ps[1][0], ps[2][0], ps[3][0], ps[4][0], mem))
        self._leave(cur)

    def update_problem_data(self, ws, ys, zs, inv_rho, sigma):
        ps = [_ptr(ws, "ws"), _ptr(ys, "ys"), _ptr(zs, "zs"), _ptr(inv_rho, "inv_rho")]
        mem = _mem_of(*ps)
        cur = self._enter(ws, ys, zs, inv_rho)
        check(lib().pdplqr_update_problem_data(self.h, ps[0][0], ps[1][0], ps[2][0], ps[3][0], float(sigma), mem))
        self._leave(cur)

    def backward(self, rho):
        p = _ptr(rho, "rho")
        cur = self._enter(rho)
        check(lib().pdplqr_backward(self.h, p[0], _mem_of(p)))
        self._leave(cur)

    def backward_without_factorization(self, rho):
        p = _ptr(rho, "rho")
        cur = self._enter(rho)
        check(lib().pdplqr_backward_without_factorization(self.h, p[0], _mem_of(p)))
        self._leave(cur)

    def forward(self, x0, ws_out):
        ps = [_ptr(x0, "x0"), _ptr(ws_out, "ws")]
        cur = self._enter(x0, ws_out)
        check(lib().pdplqr_forward(self.h, ps[0][0], ps[1][0], _mem_of(*ps)))
        self._leave(cur)

    def adjoint(self, ws, gws, gE=None, gc=None, gH=None, gh=None, gx=None):
        """Gradients of a scalar loss with respect to E, c, H, h, x0 from
        ``gws`` = d loss / d ws (include/pdplqr.h: pdplqr_adjoint).  Outputs
        left ``None`` are not computed."""
        objs = [ws, gws, gE, gc, gH, gh, gx]
        ps = [_ptr(o, nm) for o, nm in zip(objs, ("ws", "gws", "gE", "gc", "gH", "gh", "gx"))]
        cur = self._enter(*objs)
        check(lib().pdplqr_adjoint(self.h, *[p[0] for p in ps], _mem_of(*ps)))
        self._leave(cur)

    def adjoint_parallel(self, ws, gws, gE=None, gc=None, gH=None, gh=None, gx=None):
        """``adjoint`` on a PARALLEL handle (include/pdplqr.h:
        pdplqr_adjoint_parallel): the same arguments and gradients."""
        objs = [ws, gws, gE, gc, gH, gh, gx]
        ps = [_ptr(o, nm) for o, nm in zip(objs, ("ws", "gws", "gE", "gc", "gH", "gh", "gx"))]
        cur = self._enter(*objs)
        check(lib().pdplqr_adjoint_parallel(self.h, *[p[0] for p in ps], _mem_of(*ps)))
        self._leave(cur)

    def adjoint_rows(self, ws, rho, gws, gvs=None, gE=None, gc=None, gH=None, gh=None, gx=None, gD=None, gg=None,
                     grho=None):
        """``adjoint`` for a handle with constraint rows (include/pdplqr.h:
        pdplqr_adjoint_rows): ``rho`` as given to ``backward``, ``gvs`` =
        d loss / d (D ws) or ``None``; adds the gradients of ``D``, of the
        penalty target ``g`` and of ``rho``."""
        objs = [ws, rho, gws, gvs, gE, gc, gH, gh, gx, gD, gg, grho]
        names = ("ws", "rho", "gws", "gvs", "gE", "gc", "gH", "gh", "gx", "gD", "gg", "grho")
        ps = [_ptr(o, nm) for o, nm in zip(objs, names)]
        cur = self._enter(*objs)
        check(lib().pdplqr_adjoint_rows(self.h, *[p[0] for p in ps], _mem_of(*ps)))
        self._leave(cur)

    def admm_adjoint(self, gws, gvs=None, gE=None, gc=None, gH=None, gh=None, gx=None, gD=None, glb=None, gub=None):
        """Gradients of the box-constrained optimum of the last ``admm_solve``
        (polish on) on its guessed active set (include/pdplqr.h:
        pdplqr_admm_adjoint): ``gws`` = d loss / d ws, ``gvs`` = d loss /
        d (D ws) or ``None``; outputs left ``None`` are not computed."""
        objs = [gws, gvs, gE, gc, gH, gh, gx, gD, glb, gub]
        names = ("gws", "gvs", "gE", "gc", "gH", "gh", "gx", "gD", "glb", "gub")
        ps = [_ptr(o, nm) for o, nm in zip(objs, names)]
        cur = self._enter(*objs)
        check(lib().pdplqr_admm_adjoint(self.h, *[p[0] for p in ps], _mem_of(*ps)))
        self._leave(cur)

    def admm_adjoint_info(self):
        """The last ``admm_adjoint``: ``status`` (1 exact, 2 approximate: the
        polish was rejected or the solve did not end solved, 3 the
        factorisation failed) and ``resid`` [batch][2]: max|D_a v| / max|v| after
        the last refinement step and that step's relative change of v."""
        st = np.zeros(self.batch, dtype=np.int32)
        rs = np.zeros((self.batch, 2))
        check(lib().pdplqr_admm_adjoint_info(self.h, st.ctypes.data_as(C.POINTER(C.c_int32)),
                                             C.c_void_p(rs.ctypes.data)))
        return {"status": st, "resid": rs}

    def clear_workspace(self):
        check(lib().pdplqr_clear_workspace(self.h))

    def model_upload_bytes(self) -> int:
        """Host -> device model bytes since creation (pdplqr_get_model_upload_bytes)."""
        v = C.c_int64(0)
        check(lib().pdplqr_get_model_upload_bytes(self.h, C.byref(v)))
        return int(v.value)

    def synchronize(self):
        check(lib().pdplqr_synchronize(self.h))

    def stream(self) -> int:
        return int(lib().pdplqr_get_stream(self.h) or 0)

    def set_stream(self, stream_ptr: int):
        check(lib().pdplqr_set_stream(self.h, C.c_void_p(stream_ptr)))
        self._ts = None

    def status(self) -> np.ndarray:
        out = np.zeros(self.batch, dtype=np.int32)
        check(lib().pdplqr_get_status(self.h, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def value_function(self, b: int, k: int):
        n = self.nx
        P = np.zeros(n * n)
        p = np.zeros(n)
        check(lib().pdplqr_get_value_function(self.h, int(b), int(k), C.c_void_p(P.ctypes.data),
                                              C.c_void_p(p.ctypes.data)))
        return P.reshape(n, n, order="F"), p

    def admm_solve(self, x0, lb, ub, rho, ws, ys, zs, settings: "AdmmSettings"):
        ps = [_ptr(x0, "x0"), _ptr(lb, "lb"), _ptr(ub, "ub"), _ptr(rho, "rho"), _ptr(ws, "ws"), _ptr(ys, "ys"),
              _ptr(zs, "zs")]
        mem = _mem_of(*ps)
        cur = self._enter(x0, lb, ub, rho, ws, ys, zs)
        check(lib().pdplqr_admm_solve(self.h, C.byref(settings), *[p[0] for p in ps], mem))
        self._polish_ran = self._polish
        self._leave(cur)

    def admm_info(self):
        it = np.zeros(self.batch, dtype=np.int32)
        cv = np.zeros(self.batch, dtype=np.int32)
        rp = np.zeros(self.batch)
        rd = np.zeros(self.batch)
        rho = np.zeros((self.batch, max(self.ny, 1)))
        i32 = C.POINTER(C.c_int32)
        n = check(lib().pdplqr_admm_info(self.h, it.ctypes.data_as(i32), cv.ctypes.data_as(i32),
                                         C.c_void_p(rp.ctypes.data), C.c_void_p(rd.ctypes.data),
                                         C.c_void_p(rho.ctypes.data)))
        info = {"iterations": int(n), "iters": it, "converged": cv.astype(bool), "prim_res": rp, "dual_res": rd,
                "rho": rho[:, :self.ny], "status": self.admm_status()}
        if self._polish_ran:
            info["polish_status"] = self.polish_info()["status"]
        return info

    def set_polish(self, enable: bool, delta: float = 1e-6, refine_iter: int = 3):
        """Switch the polish of ``admm_solve`` on or off (include/pdplqr.h:
        pdplqr_admm_set_polish; OSQP's defaults).  With it on, a problem that
        ended SOLVED gets the solution of the equality-constrained problem on its
        guessed active rows when that passes OSQP's acceptance rule."""
        check(lib().pdplqr_admm_set_polish(self.h, int(bool(enable)), float(delta), int(refine_iter)))
        self._polish = bool(enable)

    def polish_info(self):
        """The polish of the last admm_solve: ``status`` (0 not attempted, 1
        accepted, 2 rejected), ``n_active`` (rows guessed active) and ``measures``
        [batch][8]: the KKT measures of the ADMM iterate, then of the polished pair."""
        st = np.zeros(self.batch, dtype=np.int32)
        na = np.zeros(self.batch, dtype=np.int32)
        ms = np.zeros((self.batch, 8))
        i32 = C.POINTER(C.c_int32)
        check(lib().pdplqr_admm_polish_info(self.h, st.ctypes.data_as(i32), na.ctypes.data_as(i32),
                                            C.c_void_p(ms.ctypes.data)))
        return {"status": st, "n_active": na, "measures": ms}

    def kkt_residuals(self, x0, lb, ub, ws, ys):
        """The KKT measures of any ``(ws, ys)`` (pdplqr_admm_kkt_residuals; needs
        only set_model).  Host (numpy) or device (torch) inputs; returns
        ``measures [batch][4]`` in the same memory: row residual, dynamics
        residual, reduced gradient, objective."""
        objs = [x0, lb, ub, ws, ys]
        ps = [_ptr(o, nm) for o, nm in zip(objs, ("x0", "lb", "ub", "ws", "ys"))]
        mem = _mem_of(*ps)
        if mem == _lib.PDPLQR_MEM_DEVICE:
            import torch

            meas = torch.zeros(self.batch, 4, dtype=torch.float64, device=ws.device)
            pm = C.c_void_p(meas.data_ptr())
        else:
            meas = np.zeros((self.batch, 4))
            pm = C.c_void_p(meas.ctypes.data)
        cur = self._enter(*objs, meas)
        check(lib().pdplqr_admm_kkt_residuals(self.h, *[p[0] for p in ps], pm, mem))
        self._leave(cur)
        return meas

    def set_cones(self, cones):
        """Declare second-order cones over the handle's constraint rows
        (include/pdplqr.h: pdplqr_admm_set_cones): ``cones`` is a sequence of
        ``(stage, row, dim)`` sorted by stage, then row; rows ``row .. row + dim - 1``
        of that stage ask ``D w - lb`` in ``{(t, x): |x| <= t}``.  An empty
        sequence clears them."""
        tab = np.ascontiguousarray(np.asarray(list(cones), dtype=np.int32).reshape(-1, 3).T)
        i32 = C.POINTER(C.c_int32)
        check(lib().pdplqr_admm_set_cones(self.h, int(tab.shape[1]), tab[0].ctypes.data_as(i32),
                                          tab[1].ctypes.data_as(i32), tab[2].ctypes.data_as(i32)))

    def project(self, v, lb, ub):
        """The projection of ``v`` onto the handle's constraint set
        (pdplqr_admm_project): box rows clamp to ``[lb, ub]``, the rows of a cone
        give ``lb + P_K(v - lb)``.  Host (numpy) or device (torch) inputs
        ``[batch][ny]``; returns the result in the same memory."""
        objs = [v, lb, ub]
        ps = [_ptr(o, nm) for o, nm in zip(objs, ("v", "lb", "ub"))]
        mem = _mem_of(*ps)
        if mem == _lib.PDPLQR_MEM_DEVICE:
            import torch

            out = torch.empty_like(v)
            po = C.c_void_p(out.data_ptr())
        else:
            out = np.empty_like(v)
            po = C.c_void_p(out.ctypes.data)
        cur = self._enter(*objs, out)
        check(lib().pdplqr_admm_project(self.h, *[p[0] for p in ps], po, mem))
        self._leave(cur)
        return out

    def project_vjp(self, v, lb, ub, gout, want=("gv", "glb", "gub")):
        """The transposed Jacobian of ``project`` at ``v`` applied to ``gout``,
        the cotangent of its output (pdplqr_admm_project_vjp): a dict of those
        of ``gv``, ``glb``, ``gub`` named in ``want``, ``[batch][ny]`` in the
        inputs' memory.  Changes no handle state."""
        objs = [v, lb, ub, gout]
        ps = [_ptr(o, nm) for o, nm in zip(objs, ("v", "lb", "ub", "gout"))]
        mem = _mem_of(*ps)
        if mem == _lib.PDPLQR_MEM_DEVICE:
            import torch

            outs = {k: torch.empty_like(v) for k in want}
            po = [C.c_void_p(outs[k].data_ptr()) if k in outs else None for k in ("gv", "glb", "gub")]
        else:
            outs = {k: np.empty_like(v) for k in want}
            po = [C.c_void_p(outs[k].ctypes.data) if k in outs else None for k in ("gv", "glb", "gub")]
        cur = self._enter(*objs, *outs.values())
        check(lib().pdplqr_admm_project_vjp(self.h, *[p[0] for p in ps], *po, mem))
        self._leave(cur)
        return outs

    def admm_adjoint_fixed_point(self, ws, ys, zs, lb, ub, rho, gws, sigma, alpha, tol=1e-8, max_iter=4000,
                                 check_every=25, gE=None, gc=None, gH=None, gh=None, gx=None, gD=None, glb=None,
                                 gub=None):
        """Gradients of the ADMM fixed point ``(ws, ys, zs)`` the handle last
        factored the x-update at, by the fixed-point adjoint iterated on the
        device (include/pdplqr.h: pdplqr_admm_adjoint_fixed_point): box rows
        and the handle's cones alike.  ``ws`` is that x-update's ``forward``
        result, ``gws`` = d loss / d ws; outputs left ``None`` are not
        computed.  ``admm_adjoint_fixed_point_info()`` tells how it ended."""
        objs = [ws, ys, zs, lb, ub, rho, gws, gE, gc, gH, gh, gx, gD, glb, gub]
        names = ("ws", "ys", "zs", "lb", "ub", "rho", "gws", "gE", "gc", "gH", "gh", "gx", "gD", "glb", "gub")
        ps = [_ptr(o, nm) for o, nm in zip(objs, names)]
        cur = self._enter(*objs)
        check(lib().pdplqr_admm_adjoint_fixed_point(self.h, *[p[0] for p in ps[:7]], float(sigma), float(alpha),
                                                    float(tol), int(max_iter), int(check_every),
                                                    *[p[0] for p in ps[7:]], _mem_of(*ps)))
        self._leave(cur)

    def admm_adjoint_fixed_point_info(self):
        """The last ``admm_adjoint_fixed_point``, per problem: ``iters`` (the
        iteration of its last test), ``converged`` and ``resid`` [batch][2]:
        the max-norm change and the max-norm of the adjoint state there."""
        it = np.zeros(self.batch, dtype=np.int32)
        cv = np.zeros(self.batch, dtype=np.int32)
        rs = np.zeros((self.batch, 2))
        i32 = C.POINTER(C.c_int32)
        check(lib().pdplqr_admm_adjoint_fixed_point_info(self.h, it.ctypes.data_as(i32), cv.ctypes.data_as(i32),
                                                         C.c_void_p(rs.ctypes.data)))
        return {"iters": it, "converged": cv.astype(bool), "resid": rs}

    def set_infeasibility_detection(self, enable: bool, eps_prim_inf: float = 1e-4, eps_dual_inf: float = 1e-4):
        """Switch OSQP's infeasibility certificates of ``admm_solve`` on or off
        (include/pdplqr.h: pdplqr_admm_set_infeasibility_detection)."""
        check(lib().pdplqr_admm_set_infeasibility_detection(self.h, int(bool(enable)), float(eps_prim_inf),
                                                            float(eps_dual_inf)))

    def admm_status(self) -> np.ndarray:
        """PDPLQR_ADMM_* per problem after the last admm_solve: 0 unsolved, 1 solved,
        2 primal infeasible, 3 dual infeasible (cost unbounded below)."""
        out = np.zeros(self.batch, dtype=np.int32)
        check(lib().pdplqr_admm_status(self.h, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def admm_certificate(self, dy=None, dw=None):
        """The dy / dw of the deciding test for the problems with status 2 / 3
        (zeros for the rest), into the given buffers; with none given, returns
        new host arrays ``(dy, dw)``."""
        if dy is None and dw is None:
            dy = np.zeros((self.batch, self.ny))
            dw = np.zeros((self.batch, self.N * (self.nx + self.nu) + self.nx))
        ps = [_ptr(dy, "dy"), _ptr(dw, "dw")]
        cur = self._enter(dy, dw)
        check(lib().pdplqr_admm_certificate(self.h, ps[0][0], ps[1][0], _mem_of(*ps)))
        self._leave(cur)
        return dy, dw

    def check_certificates(self, x0, lb, ub, dy=None, dw=None, eps_prim_inf: float = 1e-4,
                           eps_dual_inf: float = 1e-4):
        """The two certificate tests on given vectors (pdplqr_admm_check_certificates;
        needs only set_model).  Host (numpy) or device (torch) inputs; returns
        ``(measures [batch][8], verdict [batch])`` in the same memory: verdict bit 0
        = primal infeasible, bit 1 = dual infeasible.  ``dy`` / ``dw`` None skips
        that half."""
        objs = [x0, lb, ub, dy, dw]
        ps = [_ptr(o, nm) for o, nm in zip(objs, ("x0", "lb", "ub", "dy", "dw"))]
        mem = _mem_of(*ps)
        if mem == _lib.PDPLQR_MEM_DEVICE:
            import torch

            dev = next(o for o in objs if o is not None).device
            meas = torch.zeros(self.batch, 8, dtype=torch.float64, device=dev)
            verdict = torch.zeros(self.batch, dtype=torch.int32, device=dev)
            pm, pv = C.c_void_p(meas.data_ptr()), C.c_void_p(verdict.data_ptr())
        else:
            meas = np.zeros((self.batch, 8))
            verdict = np.zeros(self.batch, dtype=np.int32)
            pm, pv = C.c_void_p(meas.ctypes.data), C.c_void_p(verdict.ctypes.data)
        cur = self._enter(*objs, meas)
        check(lib().pdplqr_admm_check_certificates(self.h, *[p[0] for p in ps], float(eps_prim_inf),
                                                   float(eps_dual_inf), pm, pv, mem))
        self._leave(cur)
        return meas, verdict

    def segments(self, ns: int):
        a = np.zeros(ns, dtype=np.int32)
        b = np.zeros(ns, dtype=np.int32)
        check(lib().pdplqr_get_segments(self.h, a.ctypes.data_as(C.POINTER(C.c_int32)),
                                        b.ctypes.data_as(C.POINTER(C.c_int32))))
        return a, b


def admm_settings(sigma=1e-6, alpha=1.6, max_iter=4000, check_every=25, eps_abs=1e-3, eps_rel=1e-3,
                  adaptive_rho=True, adaptive_rho_tolerance=5.0) -> AdmmSettings:
    st = AdmmSettings()
    lib().pdplqr_admm_settings_init(C.byref(st))
    st.sigma, st.alpha = float(sigma), float(alpha)
    st.max_iter, st.check_every = int(max_iter), int(check_every)
    st.eps_abs, st.eps_rel = float(eps_abs), float(eps_rel)
    st.adaptive_rho, st.adaptive_rho_tolerance = int(bool(adaptive_rho)), float(adaptive_rho_tolerance)
    return st


def _stage_vecs(model: LQRModel, vecs, what):
    return pack_stage_vectors(vecs, [int(x) for x in model.ncs]) if model.ncs else np.zeros(0)


class _ModelSolver:
    """Shared body of the reference-mirroring single-problem solvers."""

    _solver_kind = _lib.PDPLQR_SOLVER_SERIAL
    _reupload_model = True  # Riccati solvers re-read model_ on every call (lqr_solver.hpp:25)

    def _init_handle(self, model: LQRModel, device=0, keep_factors=True, **kw):
        self.model_ = model  # non-owning in the reference: the model must outlive the solver
        self._hd = _Handle(model.n, model.m, model.N, 1, self._solver_kind, device=device,
                           keep_factors=keep_factors, ncs=[int(x) for x in model.ncs], **kw)
        self._upload_model()

    def _upload_model(self):
        pm = pack_model(self.model_)
        self._pm = pm
        self._hd.set_model(pm.E, pm.c, pm.H, pm.h, pm.D if pm.D.size else None)

    def _y(self, v):
        if self._hd.ny == 0:
            return None
        return np.ascontiguousarray(pack_stage_vectors(v, [int(x) for x in self.model_.ncs]))

    def clear_workspace(self):
        self._hd.clear_workspace()

    def update_problem_data(self, ws: Sequence[np.ndarray], ys, zs, inv_rho_vecs, sigma: float):
        m = self.model_
        if self._reupload_model:
            self._upload_model()
        w = np.ascontiguousarray(pack_stage_vectors(ws, w_sizes(m.n, m.m, m.N)))
        self._hd.update_problem_data(w, self._y(ys), self._y(zs), self._y(inv_rho_vecs), sigma)

    def backward(self, rho_vecs):
        self._hd.backward(self._y(rho_vecs))

    def forward(self, x0, ws: List[np.ndarray]):
        m = self.model_
        out = np.zeros(m.N * (m.n + m.m) + m.n)
        self._hd.forward(np.ascontiguousarray(x0, dtype=np.float64), out)
        s = m.n + m.m
        for k in range(m.N):
            ws[k][:] = out[k * s:(k + 1) * s]
        ws[m.N][:] = out[m.N * s:]
        return ws

    def status(self) -> int:
        return int(self._hd.status()[0])

    def admm_solve(self, x0, ws: List[np.ndarray], ys, zs, rho_vecs, sigma: float = 1e-6, alpha: float = 1.6,
                   max_iter: int = 4000, check_every: int = 25, eps_abs: float = 1e-3, eps_rel: float = 1e-3,
                   adaptive_rho: bool = True, adaptive_rho_tolerance: float = 5.0,
                   detect_infeasibility: bool = False, eps_prim_inf: float = 1e-4, eps_dual_inf: float = 1e-4):
        """ADMM outer loop over this solver (new: absent in the reference,
        README.md:8) for the bounds ``e_lb <= D_con w <= e_ub`` stored in the
        model's nodes (lqr_model.hpp:21-24).  ``ws, ys, zs`` are the warm start
        (``initialize_vectors``) and are overwritten in place with the solution;
        ``rho_vecs`` as the reference's.  Returns admm_info() of problem 0."""
        m = self.model_
        if self._reupload_model:
            self._upload_model()
        ncs = [int(x) for x in m.ncs]
        w = np.ascontiguousarray(pack_stage_vectors(ws, w_sizes(m.n, m.m, m.N)))
        lb = np.ascontiguousarray(pack_stage_vectors([nd.e_lb for nd in m.nodes], ncs)) if self._hd.ny else None
        ub = np.ascontiguousarray(pack_stage_vectors([nd.e_ub for nd in m.nodes], ncs)) if self._hd.ny else None
        y, z, r = self._y(ys), self._y(zs), self._y(rho_vecs)
        st = admm_settings(sigma, alpha, max_iter, check_every, eps_abs, eps_rel, adaptive_rho,
                           adaptive_rho_tolerance)
        if detect_infeasibility:  # (off: the handle's default; unsupported kinds raise here)
            self._hd.set_infeasibility_detection(True, eps_prim_inf, eps_dual_inf)
        else:
            self._hd.set_infeasibility_detection(False)
        self._hd.admm_solve(np.ascontiguousarray(x0, dtype=np.float64), lb, ub, r, w, y, z, st)
        s = m.n + m.m
        for k in range(m.N):
            ws[k][:] = w[k * s:(k + 1) * s]
        ws[m.N][:] = w[m.N * s:]
        off = 0
        for k, nc in enumerate(ncs):
            if nc:
                ys[k][:] = y[off:off + nc]
                zs[k][:] = z[off:off + nc]
            off += nc
        info = self._hd.admm_info()
        return {"iterations": info["iterations"], "iters": int(info["iters"][0]),
                "converged": bool(info["converged"][0]), "prim_res": float(info["prim_res"][0]),
                "dual_res": float(info["dual_res"][0]), "status": int(info["status"][0])}


class LQRSolver(_ModelSolver):
    """Serial square-root Riccati (lqr_solver.hpp:9-77), HIP backward/forward."""

    _solver_kind = _lib.PDPLQR_SOLVER_SERIAL

    def __init__(self, model: LQRModel, device: int = 0, keep_factors: bool = True):
        self._init_handle(model, device=device, keep_factors=keep_factors)

    def backward_without_factorization(self, rho_vecs):
        self._hd.backward_without_factorization(self._y(rho_vecs))

    def value_function(self, k: int):
        """(P_k, p_k) with P_k = Lxx Lxx^T of the stage-k workspace."""
        return self._hd.value_function(0, k)


class LQRParallelSolver(_ModelSolver):
    """Parallel DP over horizon segments (lqr_solver_parallel.hpp:19-238)."""

    _solver_kind = _lib.PDPLQR_SOLVER_PARALLEL

    def __init__(self, model: LQRModel, num_segments: int, load_balancing: bool = True,
                 solver_type: CondensedSystemSolverType = CondensedSystemSolverType.CHOLESKY, device: int = 0,
                 segment_len: int = 0, devices=None):
        """``devices``: a list of HIP ordinals; more than one splits the horizon
        across them (one slice per device, one RCCL all-gather of the slice
        elements per backward; include/pdplqr.h num_devices) -- the multi-GPU
        form of the reference's OpenMP team (lqr_solver_parallel.hpp:102-113)."""
        self.num_segments = int(num_segments)
        self._init_handle(model, device=device, keep_factors=True, num_segments=num_segments,
                          load_balancing=load_balancing, condensed_type=int(solver_type), segment_len=segment_len,
                          devices=devices)

    def backward_without_factorization(self, rho_vecs):
        self._hd.backward_without_factorization(self._y(rho_vecs))

    def segments(self):
        return self._hd.segments(self.num_segments)


class QDLDLSolver(_ModelSolver):
    """KKT + sparse LDL^T path (qdldl_solver.hpp:14-151).  The KKT matrix is
    frozen at construction with rho_dyn = sigma = 1e-6 (qdldl_solver.hpp:38-42)."""

    _solver_kind = _lib.PDPLQR_SOLVER_KKT
    # form_rhs / update_rhs_initial_stage read model_ on every call
    # (kkt.hpp:207-300); the matrix itself stays the one formed at construction
    # (the C ABI forms it on the first model upload only).
    _reupload_model = True

    def __init__(self, model: LQRModel, device: int = 0):
        self._init_handle(model, device=device, keep_factors=False, rho_dyn=1e-6, kkt_sigma=1e-6)

    def backward(self, inv_rho_vecs):  # NOTE: inverse rho, as the reference (qdldl_solver.hpp:24)
        self._hd.backward(self._y(inv_rho_vecs))


class BatchedLQRSolver:
    """``batch`` independent LQ problems of one shape (n, m, N), solved by one
    set of HIP launches.  Buffers are batch-major flat arrays in the boundary
    layout (include/pdplqr.h): numpy (host) or torch CUDA tensors (device)."""

    def __init__(self, n: int, m: int, N: int, batch: int, solver: str = "serial", num_segments: int = 1,
                 load_balancing: bool = True, condensed: str = "CHOLESKY", keep_factors: bool = False,
                 ncs=None, device: int = 0, segment_len: int = 0, rho_dyn: float = 1e-6, kkt_sigma: float = 1e-6,
                 devices=None):
        kind = {"serial": _lib.PDPLQR_SOLVER_SERIAL, "parallel": _lib.PDPLQR_SOLVER_PARALLEL,
                "kkt": _lib.PDPLQR_SOLVER_KKT}[solver]
        self.n, self.m, self.N, self.batch = n, m, N, batch
        self._hd = _Handle(n, m, N, batch, kind, num_segments=num_segments, load_balancing=load_balancing,
                           condensed_type=int(CondensedSystemSolverType[condensed]), device=device,
                           keep_factors=keep_factors, ncs=ncs, segment_len=segment_len, rho_dyn=rho_dyn,
                           kkt_sigma=kkt_sigma, devices=devices)

    @property
    def handle(self) -> _Handle:
        return self._hd

    def set_model(self, E, c, H, h, D=None):
        self._hd.set_model(E, c, H, h, D)

    def update_problem_data(self, ws, ys=None, zs=None, inv_rho=None, sigma: float = 0.0):
        self._hd.update_problem_data(ws, ys, zs, inv_rho, sigma)

    def backward(self, rho=None):
        self._hd.backward(rho)

    def backward_without_factorization(self, rho=None):
        self._hd.backward_without_factorization(rho)

    def forward(self, x0, ws_out):
        self._hd.forward(x0, ws_out)
        return ws_out

    def adjoint(self, ws, gws, gE=None, gc=None, gH=None, gh=None, gx=None):
        """d loss / d (E, c, H, h, x0) from gws = d loss / d ws (serial solver,
        keep_factors=True, after backward + forward); see pdplqr_adjoint."""
        self._hd.adjoint(ws, gws, gE, gc, gH, gh, gx)

    def adjoint_parallel(self, ws, gws, gE=None, gc=None, gH=None, gh=None, gx=None):
        """``adjoint`` for a ``solver="parallel"`` handle (keep_factors=True,
        after backward): the adjoint solve runs segmented, at log depth in
        the horizon; see pdplqr_adjoint_parallel."""
        self._hd.adjoint_parallel(ws, gws, gE, gc, gH, gh, gx)

    def adjoint_rows(self, ws, rho, gws, gvs=None, gE=None, gc=None, gH=None, gh=None, gx=None, gD=None, gg=None,
                     grho=None):
        """The same after a penalised x-update (``ncs`` > 0): also d loss /
        d (D, g, rho), with ``gvs`` = d loss / d (D ws); see pdplqr_adjoint_rows."""
        self._hd.adjoint_rows(ws, rho, gws, gvs, gE, gc, gH, gh, gx, gD, gg, grho)

    def admm_adjoint(self, gws, gvs=None, gE=None, gc=None, gH=None, gh=None, gx=None, gD=None, glb=None, gub=None):
        """d loss / d (E, c, H, h, x0, D, lb, ub) of the optimum the last
        ``admm_solve`` (polish on) returned, exact on its active set; see
        pdplqr_admm_adjoint."""
        self._hd.admm_adjoint(gws, gvs, gE, gc, gH, gh, gx, gD, glb, gub)

    def admm_adjoint_info(self):
        return self._hd.admm_adjoint_info()

    def synchronize(self):
        self._hd.synchronize()

    def status(self):
        return self._hd.status()

    def admm_solve(self, x0, lb, ub, rho, ws, ys=None, zs=None, sigma: float = 1e-6, alpha: float = 1.6,
                   max_iter: int = 4000, check_every: int = 25, eps_abs: float = 1e-3, eps_rel: float = 1e-3,
                   adaptive_rho: bool = True, adaptive_rho_tolerance: float = 5.0,
                   detect_infeasibility: bool = False, eps_prim_inf: float = 1e-4, eps_dual_inf: float = 1e-4):
        """ADMM outer loop for the box constraints lb <= D w <= ub on the device
        (include/pdplqr.h: pdplqr_admm_solve).  ws/ys/zs hold the warm start and
        are overwritten with the solution; returns admm_info().
        ``detect_infeasibility``: recognise problems with no feasible point or a
        cost unbounded below at the termination tests (``admm_info()["status"]``
        2 / 3; ``admm_certificate()`` has the certificates)."""
        st = admm_settings(sigma, alpha, max_iter, check_every, eps_abs, eps_rel, adaptive_rho,
                           adaptive_rho_tolerance)
        self._hd.set_infeasibility_detection(detect_infeasibility, eps_prim_inf, eps_dual_inf)
        self._hd.admm_solve(x0, lb, ub, rho, ws, ys, zs, st)
        return self._hd.admm_info()

    def admm_certificate(self, dy=None, dw=None):
        return self._hd.admm_certificate(dy, dw)

    def check_certificates(self, x0, lb, ub, dy=None, dw=None, eps_prim_inf: float = 1e-4,
                           eps_dual_inf: float = 1e-4):
        return self._hd.check_certificates(x0, lb, ub, dy, dw, eps_prim_inf, eps_dual_inf)

    def admm_info(self):
        return self._hd.admm_info()

    def set_polish(self, enable: bool, delta: float = 1e-6, refine_iter: int = 3):
        """Polish the solutions of the following ``admm_solve`` calls (off by
        default; ``admm_info()["polish_status"]``, ``polish_info()``)."""
        self._hd.set_polish(enable, delta, refine_iter)

    def polish_info(self):
        return self._hd.polish_info()

    def kkt_residuals(self, x0, lb, ub, ws, ys):
        return self._hd.kkt_residuals(x0, lb, ub, ws, ys)

    def set_cones(self, cones):
        """Second-order cones over the constraint rows for the following
        ``admm_solve`` calls: a sequence of ``(stage, row, dim)``; empty clears
        (see pdplqr_admm_set_cones)."""
        self._hd.set_cones(cones)

    def project(self, v, lb, ub):
        """The projection of ``v [batch][ny]`` onto the constraint set (boxes
        and cones); see pdplqr_admm_project."""
        return self._hd.project(v, lb, ub)

    def project_vjp(self, v, lb, ub, gout, want=("gv", "glb", "gub")):
        """The projection's transposed Jacobian at ``v`` applied to ``gout``;
        see pdplqr_admm_project_vjp."""
        return self._hd.project_vjp(v, lb, ub, gout, want)

    def admm_adjoint_fixed_point(self, ws, ys, zs, lb, ub, rho, gws, sigma, alpha, tol=1e-8, max_iter=4000,
                                 check_every=25, gE=None, gc=None, gH=None, gh=None, gx=None, gD=None, glb=None,
                                 gub=None):
        """The fixed-point adjoint of the ADMM loop at its solution, box and
        cone rows alike; see pdplqr_admm_adjoint_fixed_point."""
        self._hd.admm_adjoint_fixed_point(ws, ys, zs, lb, ub, rho, gws, sigma, alpha, tol, max_iter, check_every,
                                          gE, gc, gH, gh, gx, gD, glb, gub)

    def admm_adjoint_fixed_point_info(self):
        return self._hd.admm_adjoint_fixed_point_info()

    def value_function(self, b, k):
        return self._hd.value_function(b, k)

    def close(self):
        self._hd.close()
