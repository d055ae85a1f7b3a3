"""The trimmed rigid pre-alignment's host side as Python calls: the key order and the fraction -> count rule of rigid_align_math.h,
smalfit_plan.h's rules and grids for smalfit_trimmed_rigid_align and one whole trimmed float32 iteration:
tests/host_rigid_trim_shim.cpp built and loaded by tests/host_shim.py.  Nothing here needs a GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np

from tests import host_shim

_LIB = None


def load():
    """built without contraction, as tests/host_rigid_align.py builds its shim"""
    global _LIB
    if _LIB is None:
        lib = host_shim.build("host_rigid_trim_shim.cpp", "host_rigid_trim_shim", ("-ffp-contract=off",))
        vp, i, f = C.c_void_p, C.c_int, C.c_float
        lib.hrt_keep_count.argtypes = [C.c_double, i]
        lib.hrt_key_bits.argtypes = [f]
        lib.hrt_key_bits.restype = C.c_uint
        lib.hrt_key_kept.argtypes = [C.c_uint, i, C.c_uint, i]
        lib.hrt_select.argtypes = [i, vp, vp, i, vp, vp]
        lib.hrt_iterate.argtypes = [i, vp, i, vp, vp, f, f, i, i, vp, vp, vp, vp, vp, vp, vp]
        lib.hrt_refusal.restype = C.c_char_p
        lib.hrt_refusal.argtypes = [vp, i, i, i, i]
        lib.hrt_on.argtypes = [vp, i, i, i, i]
        lib.hrt_grids.argtypes = [i, i, i, i, i, vp]
        lib.hrt_offsets.argtypes = [vp]
        _LIB = lib
    return _LIB


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, np.float32)
    return a if shape is None else a.reshape(shape)


def keep_count(fraction, count):
    return int(load().hrt_keep_count(float(fraction), int(count)))


def key_bits(d2):
    return int(load().hrt_key_bits(float(d2)))


def key_kept(bits, q, tbits, tq):
    return bool(load().hrt_key_kept(int(bits), int(q), int(tbits), int(tq)))


def select(d2, keep, idx=None):
    """-> (kept uint8 (count,), threshold bits, threshold query): the `keep` lowest keys of the queries with idx >= 0 (default: all)"""
    d2 = _f32(d2, -1)
    idx = np.zeros(len(d2), np.int32) if idx is None else np.ascontiguousarray(idx, np.int32)
    kept, thr = np.empty(len(d2), np.uint8), np.empty(2, np.uint32)
    load().hrt_select(len(d2), d2.ctypes.data, idx.ctypes.data, int(keep), kept.ctypes.data, thr.ctypes.data)
    return kept, int(thr[0]), int(thr[1].astype(np.int32))


def iterate(x, p, T, keep_point, keep_vert, w_point=1.0, w_vert=1.0):
    """one trimmed float32 iteration of the definition -> dict(T, cost, kept, idx_v, idx_p, kept_v, kept_p, trim_d2)"""
    x, p, T = _f32(x, (-1, 3)), _f32(p, (-1, 3)), _f32(T, 12)
    out, cost, d2 = np.empty(12, np.float32), C.c_float(), np.empty(2, np.float32)
    iv, ip = np.full(len(x), -2, np.int32), np.full(len(p), -2, np.int32)
    kv, kp = np.full(len(x), 255, np.uint8), np.full(len(p), 255, np.uint8)
    kept = load().hrt_iterate(len(x), x.ctypes.data, len(p), p.ctypes.data, T.ctypes.data, float(w_point), float(w_vert), int(keep_point),
                              int(keep_vert), out.ctypes.data, C.addressof(cost), iv.ctypes.data, ip.ctypes.data, kv.ctypes.data,
                              kp.ctypes.data, d2.ctypes.data)
    return dict(T=out, cost=np.float32(cost.value), kept=int(kept), idx_v=iv, idx_p=ip, kept_v=kv, kept_p=kp, trim_d2=d2)


def refusal(block, V=100, S=90, vert_dir=True, point_dir=True):
    """the text rigid_trim_args_refusal gives for the block, None when it is accepted"""
    msg = load().hrt_refusal(C.addressof(block), V, S, int(vert_dir), int(point_dir))
    return None if msg is None else msg.decode()


def trim_on(block, V=100, S=90, vert_dir=True, point_dir=True):
    return bool(load().hrt_on(None if block is None else C.addressof(block), V, S, int(vert_dir), int(point_dir)))


def grids(vert_dir, point_dir, K, N, iterations):
    out = (C.c_int * 5)()
    load().hrt_grids(int(vert_dir), int(point_dir), K, N, iterations, out)
    return dict(trim=tuple(out[0:3]), launches=out[3], untrimmed_launches=out[4])


def sizeof_args():
    return load().hrt_sizeof_args()


def offsets():
    out = (C.c_int * 16)()
    n = load().hrt_offsets(out)
    return list(out[:n])
