"""mesh3d_math.h's point-to-triangle distance and smalfit_plan.h's rules, grids and chunk size for smalfit_mesh_score as
Python calls: tests/host_mesh_score_shim.cpp built and loaded by tests/host_shim.py.  Nothing here needs a GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np

from tests import host_shim

_LIB = None


def load():
    """built without contraction, so that the deviation recorded in tests/golden/hip_mesh_score_measured.json does not
    depend on which multiply-adds a host compiler chooses to fuse"""
    global _LIB
    if _LIB is None:
        lib = host_shim.build("host_mesh_score_shim.cpp", "host_mesh_score_shim", ("-ffp-contract=off",))
        lib.hms_mesh_score_args_refusal.restype = C.c_char_p
        lib.hms_mesh_score_args_refusal.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        _LIB = lib
    return _LIB


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def point_triangle_dist(lib, p, a, b, c):
    """sqrtf(point_triangle_dist2) of `count` independent pairs, arrays (count, 3) -> (count,) float32"""
    p, a, b, c = (_f32(x).reshape(-1, 3) for x in (p, a, b, c))
    out = np.empty(len(p), np.float32)
    lib.hms_point_triangle_dist(len(p), _p(p), _p(a), _p(b), _p(c), _p(out))
    return out


def surface_dist(lib, q, verts, faces):
    """least distance from every query to the triangles (verts, faces), as the kernel forms it -> (len(q),) float32"""
    q, verts = _f32(q).reshape(-1, 3), _f32(verts).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    out = np.empty(len(q), np.float32)
    lib.hms_surface_dist(len(q), _p(q), _p(verts), len(faces), _p(faces), _p(out))
    return out


def refusal(lib, args, max_meshes, max_points, target_meshes):
    """the text mesh_score_args_refusal gives for the block, None when it is accepted"""
    msg = lib.hms_mesh_score_args_refusal(C.byref(args), int(max_meshes), int(max_points), int(target_meshes))
    return None if msg is None else msg.decode()


def offsets(lib):
    out = (C.c_int * 16)()
    n = lib.hms_offsets(out)
    return list(out[:n])


def grid2(fn, *args):
    out = (C.c_int * 2)()
    fn(*[int(a) for a in args], out)
    return out[0], out[1]


def surface_chunk():
    """kSurfaceChunk: triangles mesh3d_surface_dist_kernel stages at a time"""
    return int(load().hms_surface_chunk())
