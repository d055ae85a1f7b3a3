"""mesh3d_topology.h's boundary flags and vertex -> face table, mesh3d_math.h's gates and smalfit_plan.h's rules for the gate block as
Python calls: tests/host_surface_gate_shim.cpp built and loaded by tests/host_shim.py.  Nothing here needs a GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np

from tests import host_shim

_LIB = None


def load():
    """built without contraction, as tests/host_surface_term.py builds its shim"""
    global _LIB
    if _LIB is None:
        lib = host_shim.build("host_surface_gate_shim.cpp", "host_surface_gate_shim", ("-ffp-contract=off",))
        lib.hsg_refusal.restype = C.c_char_p
        lib.hsg_refusal.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
        lib.hsg_plan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        lib.hsg_boundary_match.argtypes = [C.c_uint, C.c_int, C.c_float]
        lib.hsg_compatible.argtypes = [C.c_int] + [C.c_void_p] * 4 + [C.c_float, C.c_void_p, C.c_void_p]
        lib.hsg_nearest_gated.argtypes = ([C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float,
                                           C.c_float] + [C.c_void_p] * 6)
        _LIB = lib
    return _LIB


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _i32(a):
    return np.ascontiguousarray(a, np.int32)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def boundary_flags(V, faces):
    faces = _i32(faces).reshape(-1, 3)
    out = np.zeros(len(faces), np.uint8)
    assert load().hsg_boundary_flags(int(V), len(faces), _p(faces), _p(out)) == 0
    return out


def vertex_faces(V, faces):
    faces = _i32(faces).reshape(-1, 3)
    off, vf = np.zeros(V + 1, np.int32), np.zeros(3 * len(faces), np.int32)
    assert load().hsg_vertex_faces(int(V), len(faces), _p(faces), _p(off), _p(vf)) == 0
    return off, vf


def compatible(u, a, b, c, thr):
    """`count` independent (unit normal, triangle) pairs -> (signed squared cosine float32, compatible bool)"""
    u, a, b, c = (_f32(x).reshape(-1, 3) for x in (u, a, b, c))
    ssc, ok = np.empty(len(u), np.float32), np.empty(len(u), np.int32)
    load().hsg_compatible(len(u), _p(u), _p(a), _p(b), _p(c), float(thr), _p(ssc), _p(ok))
    return ssc, ok.astype(bool)


def boundary_match(flags, winner, t):
    return bool(load().hsg_boundary_match(int(flags), int(winner), float(t)))


def closest_where(p, a, b, c):
    p, a, b, c = (_f32(x).reshape(-1, 3) for x in (p, a, b, c))
    n = len(p)
    o = dict(d2=np.empty(n, np.float32), bary=np.empty((n, 3), np.float32), r=np.empty((n, 3), np.float32),
             winner=np.empty(n, np.int32), t=np.empty(n, np.float32), d2_plain=np.empty(n, np.float32),
             bary_plain=np.empty((n, 3), np.float32), r_plain=np.empty((n, 3), np.float32))
    load().hsg_closest_where(n, _p(p), _p(a), _p(b), _p(c), *(_p(o[k]) for k in ("d2", "bary", "r", "winner", "t", "d2_plain",
                                                                                 "bary_plain", "r_plain")))
    return o


def nearest_gated(q, u, verts, faces, slices=1, min_cos=-1.0, tau2=np.inf, flags=None):
    """every query against the mesh as the gated kernels do it -> dict(face, kept, d2, bary, r)"""
    q, verts = _f32(q).reshape(-1, 3), _f32(verts).reshape(-1, 3)
    faces = _i32(faces).reshape(-1, 3)
    use_cos = min_cos > -1.0
    u = _f32(u).reshape(-1, 3) if use_cos else None
    fl = None if flags is None else np.ascontiguousarray(flags, np.uint8)
    n = len(q)
    o = dict(face=np.empty(n, np.int32), kept=np.empty(n, np.uint8), d2=np.empty(n, np.float32), bary=np.empty((n, 3), np.float32),
             r=np.empty((n, 3), np.float32))
    load().hsg_nearest_gated(n, _p(q), _p(u), _p(verts), len(faces), _p(faces), int(slices), int(use_cos), float(min_cos), float(tau2),
                             _p(fl), _p(o["face"]), _p(o["kept"]), _p(o["d2"]), _p(o["bary"]), _p(o["r"]))
    return o


def vertex_normals(verts, faces):
    verts, faces = _f32(verts).reshape(-1, 3), _i32(faces).reshape(-1, 3)
    out = np.empty_like(verts)
    assert load().hsg_vertex_normals(len(verts), _p(verts), len(faces), _p(faces), _p(out)) == 0
    return out


def face_unit_normals(verts, faces):
    verts, faces = _f32(verts).reshape(-1, 3), _i32(faces).reshape(-1, 3)
    out = np.empty((len(faces), 3), np.float32)
    load().hsg_face_unit_normals(_p(verts), len(faces), _p(faces), _p(out))
    return out


def refusal(gate, term, targets=True, step=False, step_has_points=False):
    """the text surface_gate_args_refusal gives for the gate block beside the term's block, None when it is accepted"""
    msg = load().hsg_refusal(C.addressof(gate), C.addressof(term), int(targets), int(step), int(step_has_points))
    return None if msg is None else msg.decode()


def plan(gate, point_dir=True, vert_dir=True):
    oi, of = (C.c_int * 4)(), (C.c_float * 4)()
    load().hsg_plan(None if gate is None else C.addressof(gate), int(point_dir), int(vert_dir), oi, of)
    return dict(any=bool(oi[0]), cos_point=bool(oi[1]), cos_vert=bool(oi[2]), boundary=bool(oi[3]), cc_point=of[0], cc_vert=of[1],
                tau2_point=of[2], tau2_vert=of[3])


def offsets():
    out = (C.c_int * 32)()
    n = load().hsg_offsets(out)
    return list(out[:n])
