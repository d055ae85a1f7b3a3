"""fit3d_sequence_math.h's row sum, temporal gradient and loss and smalfit_plan.h's rules and plan for the scan-sequence block as
Python calls: tests/host_sequence_shim.cpp built and loaded by tests/host_shim.py.  Nothing here needs a GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np

from smalify_amd import _lib
from tests import host_shim

_LIB = None
FACT_ORDER = ("handle_meshes", "lengths_sum", "num_meshes", "step", "global_rot", "joint_rot", "trans")
WEIGHT_KEYS = ("w_temp_joint", "w_temp_global", "w_temp_trans")


def load():
    """built without contraction, as tests/host_robust.py builds its shim"""
    global _LIB
    if _LIB is None:
        lib = host_shim.build("host_sequence_shim.cpp", "host_sequence_shim", ("-ffp-contract=off",))
        lib.hsq_couple.restype = None
        lib.hsq_couple.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6
        lib.hsq_row_sum.restype = C.c_float
        lib.hsq_row_sum.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        lib.hsq_grad.restype = C.c_float
        lib.hsq_grad.argtypes = [C.c_float, C.c_float, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int]
        lib.hsq_loss.restype = C.c_float
        lib.hsq_loss.argtypes = [C.c_float, C.c_float, C.c_int]
        lib.hsq_create_refusal.restype = C.c_char_p
        lib.hsq_create_refusal.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
        lib.hsq_refusal.restype = C.c_char_p
        lib.hsq_refusal.argtypes = [C.c_void_p, C.c_void_p]
        lib.hsq_plan.restype = None
        lib.hsq_plan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        _LIB = lib
    return _LIB


def block(share_shape=True, weights=(0.0, 0.0, 0.0), losses=None, step_total=None):
    """a smalfit_sequence_args over host (or no) pointers"""
    q = _lib.SequenceArgs()
    q.share_shape = int(bool(share_shape))
    q.w_temp_joint, q.w_temp_global, q.w_temp_trans = (float(w) for w in weights)
    q.losses = losses
    q.step_total = step_total
    return q


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32).copy()


def _p(a):
    return None if a is None else a.ctypes.data


def couple(clips, state, share_shape=True, weights=(0.0, 0.0, 0.0), grads=("g_betas", "g_theta", "g_trans")):
    """the coupling on copies of the state's gradients -> dict(g_betas, g_theta, g_trans (None where not asked for), losses (4,))"""
    clips = [int(c) for c in clips]
    N = sum(clips)
    lengths = (C.c_int * len(clips))(*clips)
    g = {k: (_f32(state[k]) if k in grads else None) for k in ("g_betas", "g_theta", "g_trans")}
    x = {k: _f32(state[k]) for k in ("global_rot", "joint_rot", "trans")}
    losses = np.full(4, np.nan, np.float32)
    q = block(share_shape, weights, losses.ctypes.data)
    nb = int(state["g_betas"].shape[1])
    load().hsq_couple(N, len(clips), lengths, C.addressof(q), nb, _p(x["global_rot"]), _p(x["joint_rot"]), _p(x["trans"]),
                      _p(g["g_betas"]), _p(g["g_theta"]), _p(g["g_trans"]))
    g["losses"] = losses
    return g


def row_sum(g, col, start, length):
    g = np.ascontiguousarray(g, np.float32)
    return np.float32(load().hsq_row_sum(g.ctypes.data, int(g.shape[1]), int(col), int(start), int(length)))


def grad(g, w, L, x, prev, nxt, has_prev, has_next):
    return np.float32(load().hsq_grad(float(g), float(w), int(L), float(x), float(prev), float(nxt), int(has_prev), int(has_next)))


def loss(w, S, L):
    return np.float32(load().hsq_loss(float(w), float(S), int(L)))


def create_refusal(num_meshes, clips, given=True):
    clips = [int(c) for c in clips]
    lengths = (C.c_int * max(len(clips), 1))(*clips)
    msg = load().hsq_create_refusal(int(given), int(num_meshes), len(clips), lengths)
    return None if msg is None else msg.decode()


def refusal(q, **facts):
    """the text sequence_args_refusal gives for the block, None when it is accepted"""
    full = dict(handle_meshes=4, lengths_sum=4, num_meshes=4, step=True, global_rot=True, joint_rot=True, trans=True)
    for k, v in facts.items():
        if k not in full:
            raise KeyError(k)
        full[k] = v
    f = (C.c_int * len(FACT_ORDER))(*[int(full[k]) for k in FACT_ORDER])
    msg = load().hsq_refusal(C.addressof(q), f)
    return None if msg is None else msg.decode()


def plan(q, any_long=True, betas_given=True, num_meshes=4, num_clips=2, num_betas=20):
    out = (C.c_int * 6)()
    load().hsq_plan(None if q is None else C.addressof(q), int(any_long), int(betas_given), int(num_meshes), int(num_clips),
                    int(num_betas), out)
    return dict(launch=bool(out[0]), share=bool(out[1]), joint=bool(out[2]), **{"global": bool(out[3])}, trans=bool(out[4]),
                blocks=int(out[5]))


def sizeof_args():
    return load().hsq_sizeof_args()


def offsets():
    out = (C.c_int * 16)()
    n = load().hsq_offsets(out)
    return list(out[:n])
