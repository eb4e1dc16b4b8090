"""The PARALLEL solver's device segment planner (pdp-lqr_amd/csrc/parallel_host.hip
plan_segments) on the CPU, through pdplqr_debug_segment_plan (host arithmetic
only).  tests/golden/segment_plans.json holds, per configuration, the device
segments the library had before the planner became a function (read on an
MI355X through pdplqr_debug_parallel which = 5), with the resident-slot counts
of that device (pdplqr_debug_segment_slots) the planner is fed here.  The GPU
test at the end ties a created handle's segments to the same function."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

IP = C.POINTER(C.c_int32)
with open(os.path.join(GOLDEN, "segment_plans.json")) as _f:
    FIXTURES = json.load(_f)
# (N, ns, L): an explicit segment_len reads no slots
EXPLICIT = [(100, 4, 7), (9, 3, 2), (1024, 8, 1000), (5, 1, 1)]


def _plan(N, n, m, batch, ns, lb, seglen, slots):
    """(S or error code, starts, lengths, mw)"""
    from pdplqr._lib import lib

    L = lib()
    L.pdplqr_debug_segment_plan.argtypes = [C.c_int32] * 7 + [IP, IP, IP, C.c_int32, IP]
    L.pdplqr_debug_segment_plan.restype = C.c_int
    sl = np.ascontiguousarray(np.asarray(slots, dtype=np.int32))
    st, ln, mw = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32), C.c_int32(-1)
    S = L.pdplqr_debug_segment_plan(N, n, m, batch, ns, int(lb), seglen, sl.ctypes.data_as(IP), st.ctypes.data_as(IP),
                                    ln.ctypes.data_as(IP), N, C.byref(mw))
    if S < 0:
        return S, None, None, None
    assert S <= N
    return S, st[:S].tolist(), ln[:S].tolist(), int(mw.value)


def _ref_segments(N, ns, lb):
    """the reference segmentation (pdplqr_get_segments' formula, lqr_solver_parallel.hpp:70-81)"""
    scale = 1.55 if lb else 1.0
    start, length = [], []
    for i in range(ns):
        start.append(0 if i == 0 else start[-1] + length[-1])
        length.append(int(N / (scale + ns - 1)) if i < ns - 1 else N - start[i])
    return start, length


def _check_tiling(N, ns, lb, start, length):
    assert start[0] == 0 and min(length) >= 1
    for i in range(1, len(start)):
        assert start[i] == start[i - 1] + length[i - 1]
    assert start[-1] + length[-1] == N
    rs, _ = _ref_segments(N, ns, lb)
    assert set(rs) <= set(start)


@pytest.mark.parametrize("fx", FIXTURES,
                         ids=lambda f: "n%d_m%d_N%d_ns%d_b%d" % (f["n"], f["m"], f["N"], f["ns"], f["batch"]))
def test_planner_reproduces_recorded_segments(fx):
    S, st, ln, mw = _plan(fx["N"], fx["n"], fx["m"], fx["batch"], fx["ns"], fx["load_balancing"], fx["segment_len"],
                          fx["slots"])
    assert S == len(fx["start"]) == len(fx["len"])
    assert st == fx["start"] and ln == fx["len"]
    assert mw == fx["mw"]
    _check_tiling(fx["N"], fx["ns"], fx["load_balancing"], st, ln)


@pytest.mark.parametrize("lb", [False, True])
@pytest.mark.parametrize("N,ns,L", EXPLICIT)
def test_explicit_segment_len(N, ns, L, lb):
    S, st, ln, mw = _plan(N, 6, 3, 1, ns, lb, L, [0, 0, 0, 0])
    rs, rl = _ref_segments(N, ns, lb)
    want_st, want_ln = [], []
    for s0, l in zip(rs, rl):
        p = -(-l // L)
        at = s0
        for q in range(p):
            piece = l // p + (1 if q < l % p else 0)
            want_st.append(at)
            want_ln.append(piece)
            at += piece
    assert (S, st, ln) == (len(want_st), want_st, want_ln)
    assert mw == 1  # (the 4-wave family is only left by the cost model)
    _check_tiling(N, ns, lb, st, ln)


def test_empty_reference_segment_is_refused():
    assert _plan(2, 6, 3, 1, 3, True, 0, [512, 512, 1024, 1024])[0] < 0
    assert _plan(2, 6, 3, 1, 3, True, 1, [0, 0, 0, 0])[0] < 0


@pytest.mark.gpu
@pytest.mark.parametrize("n,m,N,ns", [(12, 4, 64, 2), (24, 8, 96, 2), (4, 2, 9, 3)])
def test_handle_segments_are_the_planner_s(n, m, N, ns):
    from pdplqr import _lib
    from pdplqr.solvers import _Handle

    L = _lib.lib()
    h = _Handle(n, m, N, batch=1, solver=_lib.PDPLQR_SOLVER_PARALLEL, num_segments=ns)
    try:
        buf = np.zeros(2 * N, dtype=np.int32)
        L.pdplqr_debug_parallel.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong]
        L.pdplqr_debug_parallel.restype = C.c_int
        S = L.pdplqr_debug_parallel(h.h, 5, buf.ctypes.data_as(C.c_void_p), buf.nbytes)
        assert 0 < S <= N
        slots = np.zeros(4, dtype=np.int32)
        L.pdplqr_debug_segment_slots.argtypes = [C.c_void_p, IP]
        L.pdplqr_debug_segment_slots.restype = C.c_int
        assert L.pdplqr_debug_segment_slots(h.h, slots.ctypes.data_as(IP)) == 0
        assert slots.min() >= 1
    finally:
        h.close()
    S2, st, ln, _ = _plan(N, n, m, 1, ns, True, 0, slots)
    assert S2 == S
    assert st == buf[0:2 * S:2].tolist() and ln == buf[1:2 * S:2].tolist()
    _check_tiling(N, ns, True, st, ln)
