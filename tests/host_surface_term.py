"""mesh3d_math.h's closest point on a triangle and smalfit_plan.h's rules, slice count and grids for the surface term as Python
calls: tests/host_surface_term_shim.cpp built and loaded by tests/host_shim.py.  Nothing here needs a GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np

from tests import host_shim

_LIB = None
POINTS = ("None", "SampleToObjective", "SampleToCaller", "Callers", "CallersCopied")      # Fit3dPoints, in its order


def load():
    """built without contraction: what the shim deviates by does not depend on which multiply-adds a host compiler fuses"""
    global _LIB
    if _LIB is None:
        lib = host_shim.build("host_surface_term_shim.cpp", "host_surface_term_shim", ("-ffp-contract=off",))
        lib.hst_refusal.restype = C.c_char_p
        lib.hst_refusal.argtypes = [C.c_void_p] + [C.c_int] * 8
        lib.hst_fit3d_points.argtypes = [C.c_float, C.c_int, C.c_int, C.c_int, C.c_int]
        _LIB = lib
    return _LIB


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def closest(p, a, b, c):
    """`count` independent pairs -> dict(d2, bary, r, dist2): point_triangle_closest, and point_triangle_dist2 beside it"""
    p, a, b, c = (_f32(x).reshape(-1, 3) for x in (p, a, b, c))
    n = len(p)
    o = dict(d2=np.empty(n, np.float32), bary=np.empty((n, 3), np.float32), r=np.empty((n, 3), np.float32),
             dist2=np.empty(n, np.float32))
    load().hst_closest(n, _p(p), _p(a), _p(b), _p(c), _p(o["d2"]), _p(o["bary"]), _p(o["r"]), _p(o["dist2"]))
    return o


def nearest(q, verts, faces, slices=1):
    """every query against the mesh as the kernels do it -> dict(face, d2, bary, r)"""
    q, verts = _f32(q).reshape(-1, 3), _f32(verts).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    n = len(q)
    o = dict(face=np.empty(n, np.int32), d2=np.empty(n, np.float32), bary=np.empty((n, 3), np.float32), r=np.empty((n, 3), np.float32))
    load().hst_nearest(n, _p(q), _p(verts), len(faces), _p(faces), int(slices), _p(o["face"]), _p(o["d2"]), _p(o["bary"]), _p(o["r"]))
    return o


def gather(V, corners, bary, r):
    corners = np.ascontiguousarray(corners, np.int32).reshape(-1, 3)
    bary, r = _f32(bary).reshape(-1, 3), _f32(r).reshape(-1, 3)
    g = np.empty((V, 3), np.float32)
    load().hst_gather(int(V), len(corners), _p(corners), _p(bary), _p(r), _p(g))
    return g


def refusal(args, max_meshes, max_points, targets, target_meshes, step, step_meshes, step_points, step_has_points):
    """the text surface_term_args_refusal gives for the block, None when it is accepted"""
    msg = load().hst_refusal(C.byref(args), int(max_meshes), int(max_points), int(targets), int(target_meshes), int(step),
                             int(step_meshes), int(step_points), int(step_has_points))
    return None if msg is None else msg.decode()


def offsets():
    out = (C.c_int * 32)()
    n = load().hst_offsets(out)
    return list(out[:n])


def slices(queries, faces, N):
    return int(load().hst_surface_slices(int(queries), int(faces), int(N)))


def near_grid(queries, faces, N):
    out = (C.c_int * 3)()
    load().hst_surface_near_grid(int(queries), int(faces), int(N), out)
    return tuple(out)


def fit3d_points(w_chamfer, points=False, points_out=False, same=False, point_surface=False):
    return POINTS[load().hst_fit3d_points(float(w_chamfer), int(points), int(points_out), int(same), int(point_surface))]
