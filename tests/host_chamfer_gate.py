"""mesh3d_math.h's gated chamfer scan and smalfit_plan.h's rules for the chamfer gate block as Python calls:
tests/host_chamfer_gate_shim.cpp built and loaded by tests/host_shim.py.  Nothing here needs a GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np

from tests import host_shim

_LIB = None


def load():
    """built without contraction, as tests/host_surface_gate.py builds its shim"""
    global _LIB
    if _LIB is None:
        lib = host_shim.build("host_chamfer_gate_shim.cpp", "host_chamfer_gate_shim", ("-ffp-contract=off",))
        lib.hcg_refusal.restype = C.c_char_p
        lib.hcg_refusal.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        lib.hcg_plan.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        lib.hcg_scan.argtypes = ([C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_float, C.c_float] +
                                 [C.c_void_p] * 4)
        lib.hcg_compatible.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
        lib.hcg_match.argtypes = [C.c_float, C.c_int, C.c_float, C.c_int, C.c_void_p]
        _LIB = lib
    return _LIB


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def scan(q, qn, x, xn, xb=None, owner=None, min_cos=-1.0, tau2=np.inf):
    """every query against the scanned set as the gated kernel does it -> dict(index, kept, d2, gather)"""
    q, x = _f32(q).reshape(-1, 3), _f32(x).reshape(-1, 3)
    use_cos = min_cos > -1.0
    qn = _f32(qn).reshape(-1, 3) if use_cos else None
    xn = _f32(xn).reshape(-1, 3) if use_cos else None
    xb = None if xb is None else np.ascontiguousarray(xb, np.uint8)
    owner = None if owner is None else np.ascontiguousarray(owner, np.int32)
    n = len(q)
    o = dict(index=np.empty(n, np.int32), kept=np.empty(n, np.uint8), d2=np.empty(n, np.float32), gather=np.zeros((n, 3), np.float32))
    load().hcg_scan(n, _p(q), _p(qn), len(x), _p(x), _p(xn), _p(xb), _p(owner), int(use_cos), float(min_cos), float(tau2),
                    _p(o["index"]), _p(o["kept"]), _p(o["d2"]), _p(o["gather"]))
    o["kept"] = o["kept"].astype(bool)
    return o


def compatible(a, b, c):
    """`count` independent pairs of unit normals -> (float32 dot product, compatible bool)"""
    a, b = _f32(a).reshape(-1, 3), _f32(b).reshape(-1, 3)
    dot, ok = np.empty(len(a), np.float32), np.empty(len(a), np.int32)
    load().hcg_compatible(len(a), _p(a), _p(b), float(c), _p(dot), _p(ok))
    return dot, ok.astype(bool)


def match(best, tag, tau2=np.inf, reject=False):
    kept = C.c_int()
    idx = load().hcg_match(float(best), int(tag), float(tau2), int(reject), C.byref(kept))
    return idx, bool(kept.value)


def tag(index, boundary):
    return load().hcg_tag(int(index), int(boundary))


def refusal(gate, chamfer_on=True, step=False, step_has_points=False):
    """the text chamfer_gate_args_refusal gives for the block, None when it is accepted"""
    msg = load().hcg_refusal(C.addressof(gate), int(chamfer_on), int(step), int(step_has_points))
    return None if msg is None else msg.decode()


PLAN_FLAGS = ("gated_point", "gated_vert", "cos_point", "cos_vert", "boundary", "vert_normals", "point_normals", "point_boundary")


def plan(gate, chamfer_on=True):
    oi, of = (C.c_int * 8)(), (C.c_float * 4)()
    load().hcg_plan(None if gate is None else C.addressof(gate), int(chamfer_on), oi, of)
    out = {k: bool(oi[i]) for i, k in enumerate(PLAN_FLAGS)}
    out.update(c_point=of[0], c_vert=of[1], tau2_point=of[2], tau2_vert=of[3])
    return out


def constants():
    out = (C.c_int * 4)()
    load().hcg_constants(out)
    return dict(chunk=out[0], record_bytes=out[1], lds_bytes=out[2], ungated_record_bytes=out[3])


def offsets():
    out = (C.c_int * 32)()
    n = load().hcg_offsets(out)
    return list(out[:n])
