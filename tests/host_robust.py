"""mesh3d_math.h's robust_gm and weighted gather and smalfit_plan.h's rules and plan for the robust block as Python calls:
tests/host_robust_shim.cpp built and loaded by tests/host_shim.py.  Nothing here needs a GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np

from tests import host_shim

_LIB = None
FACT_ORDER = ("chamfer_call", "surface_call", "chamfer_on", "point_dir", "vert_dir")


def load():
    """built without contraction, as tests/host_chamfer_gate.py builds its shim"""
    global _LIB
    if _LIB is None:
        lib = host_shim.build("host_robust_shim.cpp", "host_robust_shim", ("-ffp-contract=off",))
        lib.hrb_gm.argtypes = [C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
        lib.hrb_scale_sq.restype = C.c_float
        lib.hrb_scale_sq.argtypes = [C.c_float]
        lib.hrb_scale_on.argtypes = [C.c_float]
        lib.hrb_refusal.restype = C.c_char_p
        lib.hrb_refusal.argtypes = [C.c_void_p, C.c_void_p]
        lib.hrb_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.hrb_weighted_gather.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _LIB = lib
    return _LIB


def _facts(facts):
    full = dict(chamfer_call=True, surface_call=True, chamfer_on=True, point_dir=True, vert_dir=True)
    for k, v in facts.items():
        if k not in full:
            raise KeyError(k)
        full[k] = v
    return (C.c_int * 5)(*[int(full[k]) for k in FACT_ORDER])


def gm(d2, s2):
    """robust_gm on float32 squared distances -> (rho, w) float32"""
    d2 = np.ascontiguousarray(d2, np.float32).reshape(-1)
    rho, w = np.empty_like(d2), np.empty_like(d2)
    load().hrb_gm(len(d2), d2.ctypes.data, float(s2), rho.ctypes.data, w.ctypes.data)
    return rho, w


def scale_sq(sigma):
    return np.float32(load().hrb_scale_sq(float(sigma)))


def scale_on(sigma):
    return bool(load().hrb_scale_on(float(sigma)))


def refusal(block, **facts):
    """the text robust_args_refusal gives for the block, None when it is accepted"""
    msg = load().hrb_refusal(C.addressof(block), _facts(facts))
    return None if msg is None else msg.decode()


def plan(block, **facts):
    oi, of = (C.c_int * 4)(), (C.c_float * 4)()
    load().hrb_plan(None if block is None else C.addressof(block), _facts(facts), oi, of)
    return dict(chamfer=bool(oi[0]), surface_point=bool(oi[1]), surface_vert=bool(oi[2]), any=bool(oi[3]), s2=tuple(of))


def weighted_gather(q, self_index, x, owner, wt):
    """one vertex against the staged points -> (nearest index, its d^2, sum over owner == self of wt (q - x))"""
    q = np.ascontiguousarray(q, np.float32)
    x = np.ascontiguousarray(x, np.float32).reshape(-1, 3)
    owner, wt = np.ascontiguousarray(owner, np.int32), np.ascontiguousarray(wt, np.float32)
    g, best = np.zeros(3, np.float32), C.c_float()
    idx = load().hrb_weighted_gather(q.ctypes.data, int(self_index), len(x), x.ctypes.data, owner.ctypes.data, wt.ctypes.data,
                                     g.ctypes.data, C.byref(best))
    return idx, best.value, g


def constants():
    out = (C.c_int * 3)()
    load().hrb_constants(out)
    return dict(robust_lds_bytes=out[0], gated_lds_bytes=out[1], gate_chunk=out[2])


def sizeof_args():
    return load().hrb_sizeof_args()


def offsets():
    out = (C.c_int * 32)()
    n = load().hrb_offsets(out)
    return list(out[:n])
