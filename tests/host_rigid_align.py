"""rigid_align_math.h's transform chain, pair sums, solve and built-in starts, the scan the kernels call and smalfit_plan.h's rules
and grids for smalfit_rigid_align as Python calls: tests/host_rigid_align_shim.cpp built and loaded by tests/host_shim.py.
Nothing here needs a GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np

from tests import host_shim

_LIB = None
NUM_MOMENTS = 19


def load():
    """built without contraction, as tests/host_robust.py builds its shim"""
    global _LIB
    if _LIB is None:
        lib = host_shim.build("host_rigid_align_shim.cpp", "host_rigid_align_shim", ("-ffp-contract=off",))
        vp, i, f = C.c_void_p, C.c_int, C.c_float
        lib.hra_constants.argtypes = [vp]
        lib.hra_apply.argtypes = [vp, i, vp, vp]
        lib.hra_means.argtypes = [i, vp, vp]
        lib.hra_cube_rotation.argtypes = [i, vp]
        lib.hra_start_transform.argtypes = [vp, vp, vp, vp]
        lib.hra_nearest.argtypes = [i, vp, i, vp, i, vp, vp, vp]
        lib.hra_pair_moments.argtypes = [vp, vp, f, vp]
        lib.hra_combine.argtypes = [vp, vp, f, f, vp]
        lib.hra_solve.argtypes = [vp, vp, vp, vp, vp, vp]
        lib.hra_iterate.argtypes = [i, vp, i, vp, vp, f, f, vp, vp, vp, vp]
        lib.hra_refusal.restype = C.c_char_p
        lib.hra_refusal.argtypes = [vp, vp]
        lib.hra_create_refusal.restype = C.c_char_p
        lib.hra_create_refusal.argtypes = [i, i, i, i, i]
        lib.hra_start_refusal.restype = C.c_char_p
        lib.hra_start_refusal.argtypes = [vp]
        lib.hra_grids.argtypes = [i, i, i, i, i, vp]
        lib.hra_offsets.argtypes = [vp]
        _LIB = lib
    return _LIB


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, np.float32)
    return a if shape is None else a.reshape(shape)


def constants():
    out = (C.c_float * 8)()
    load().hra_constants(out)
    return dict(moments=int(out[0]), sweeps=int(out[1]), rank_eps=float(out[2]), cube_rotations=int(out[3]),
                max_iterations=int(out[4]), start_tolerance=float(out[5]), queries=int(out[6]))


def apply(T, x):
    T, x = _f32(T, 12), _f32(x, (-1, 3))
    out = np.empty_like(x)
    load().hra_apply(T.ctypes.data, len(x), x.ctypes.data, out.ctypes.data)
    return out


def means(x):
    x = _f32(x, (-1, 3))
    out = np.empty(3, np.float32)
    load().hra_means(len(x), x.ctypes.data, out.ctypes.data)
    return out


def cube_rotation(k):
    R = np.empty(9, np.float32)
    load().hra_cube_rotation(int(k), R.ctypes.data)
    return R.reshape(3, 3)


def cube_rotations():
    return np.stack([cube_rotation(k) for k in range(24)])


def start_transform(R, cX, cP):
    R, cX, cP = _f32(R, 9), _f32(cX, 3), _f32(cP, 3)
    T = np.empty(12, np.float32)
    load().hra_start_transform(R.ctypes.data, cX.ctypes.data, cP.ctypes.data, T.ctypes.data)
    return T


def nearest(direction, T, x, p):
    """direction 0: for every vertex its nearest point under T; 1: for every point its nearest transformed vertex -> (idx, d2)"""
    T, x, p = _f32(T, 12), _f32(x, (-1, 3)), _f32(p, (-1, 3))
    n = len(x) if direction == 0 else len(p)
    idx, d2 = np.empty(n, np.int32), np.empty(n, np.float32)
    load().hra_nearest(int(direction), T.ctypes.data, len(x), x.ctypes.data, len(p), p.ctypes.data, idx.ctypes.data, d2.ctypes.data)
    return idx, d2


def pair_moments(xc, pc, d2):
    xc, pc = _f32(xc, 3), _f32(pc, 3)
    m = np.empty(NUM_MOMENTS, np.float32)
    load().hra_pair_moments(xc.ctypes.data, pc.ctypes.data, float(d2), m.ctypes.data)
    return m


def combine(mv, mp, wv, wp):
    mv = None if mv is None else _f32(mv, NUM_MOMENTS)
    mp = None if mp is None else _f32(mp, NUM_MOMENTS)
    M = np.empty(NUM_MOMENTS, np.float32)
    load().hra_combine(None if mv is None else mv.ctypes.data, None if mp is None else mp.ctypes.data, float(wv), float(wp), M.ctypes.data)
    return M


def moments_of_pairs(x, p, w, cX=None, cP=None):
    """the combined sums of the weighted pairs (x_i, p_i, w_i) in float32, centred at cX / cP (default: zero); d^2 is not formed"""
    x, p, w = _f32(x, (-1, 3)), _f32(p, (-1, 3)), _f32(w, -1)
    cX = np.zeros(3, np.float32) if cX is None else _f32(cX, 3)
    cP = np.zeros(3, np.float32) if cP is None else _f32(cP, 3)
    M = np.zeros(NUM_MOMENTS, np.float32)
    for i in range(len(x)):
        M = (M + w[i] * pair_moments(x[i] - cX, p[i] - cP, 0.0)).astype(np.float32)
    return M


def solve(M, cX, cP, prev):
    """-> (T (12,), kept, l1 - l2, scale)"""
    M, cX, cP, prev = _f32(M, NUM_MOMENTS), _f32(cX, 3), _f32(cP, 3), _f32(prev, 12)
    T, out2 = np.empty(12, np.float32), np.empty(2, np.float32)
    kept = load().hra_solve(M.ctypes.data, cX.ctypes.data, cP.ctypes.data, prev.ctypes.data, T.ctypes.data, out2.ctypes.data)
    return T, int(kept), float(out2[0]), float(out2[1])


def iterate(x, p, T, w_point=1.0, w_vert=1.0):
    """one float32 iteration of the definition -> dict(T, cost, kept, idx_v, idx_p)"""
    x, p, T = _f32(x, (-1, 3)), _f32(p, (-1, 3)), _f32(T, 12)
    out, cost = np.empty(12, np.float32), C.c_float()
    iv, ip = np.full(len(x), -2, np.int32), np.full(len(p), -2, np.int32)
    kept = load().hra_iterate(len(x), x.ctypes.data, len(p), p.ctypes.data, T.ctypes.data, float(w_point), float(w_vert), out.ctypes.data,
                              C.addressof(cost), iv.ctypes.data, ip.ctypes.data)
    return dict(T=out, cost=np.float32(cost.value), kept=int(kept), idx_v=iv, idx_p=ip)


def refusal(block, max_meshes=4, max_verts=512, max_points=512, max_starts=64):
    """the text rigid_align_args_refusal gives for the block on a handle of these capacities, None when it is accepted"""
    f = (C.c_int * 4)(max_meshes, max_verts, max_points, max_starts)
    msg = load().hra_refusal(C.addressof(block), f)
    return None if msg is None else msg.decode()


def create_refusal(given, max_meshes, max_verts, max_points, max_starts):
    msg = load().hra_create_refusal(int(given), max_meshes, max_verts, max_points, max_starts)
    return None if msg is None else msg.decode()


def start_refusal(R):
    R = _f32(R, 9)
    msg = load().hra_start_refusal(R.ctypes.data)
    return None if msg is None else msg.decode()


def grids(V, S, K, N, iterations):
    out = (C.c_int * 12)()
    load().hra_grids(V, S, K, N, iterations, out)
    return dict(scan_vert=tuple(out[0:3]), scan_point=tuple(out[3:6]), solve=tuple(out[6:8]), init=out[8], pick=out[9],
                launches=out[10], launches_one_direction=out[11])


def sizeof_args():
    return load().hra_sizeof_args()


def offsets():
    out = (C.c_int * 32)()
    n = load().hra_offsets(out)
    return list(out[:n])
