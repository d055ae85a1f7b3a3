"""fit3d_sequence_vertex_math.h's stencils, gradient and losses and smalfit_plan.h's rules, plan and grid for the temporal terms on
posed vertices as Python calls: tests/host_sequence_vertex_shim.cpp built and loaded by tests/host_shim.py.  Nothing here needs a
GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np

from smalify_amd import _lib
from tests import host_shim

_LIB = None
FACT_ORDER = ("step", "num_verts", "verts", "handle_meshes", "num_meshes")
WEIGHT_KEYS = ("w_temp_vert_vel", "w_temp_vert_acc")


def load():
    """built without contraction, as tests/host_sequence.py builds its shim"""
    global _LIB
    if _LIB is None:
        lib = host_shim.build("host_sequence_vertex_shim.cpp", "host_sequence_vertex_shim", ("-ffp-contract=off",))
        lib.hsv_term.restype = None
        lib.hsv_term.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.hsv_step_total.restype = C.c_float
        lib.hsv_step_total.argtypes = [C.c_float] * 3
        lib.hsv_refusal.restype = C.c_char_p
        lib.hsv_refusal.argtypes = [C.c_void_p, C.c_void_p]
        lib.hsv_plan.restype = None
        lib.hsv_plan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        _LIB = lib
    return _LIB


def block(weights=(0.0, 0.0), losses=None, step_total=None):
    """a smalfit_sequence_vertex_args over host (or no) pointers"""
    q = _lib.SequenceVertexArgs()
    q.w_temp_vert_vel, q.w_temp_vert_acc = (float(w) for w in weights)
    q.losses = losses
    q.step_total = step_total
    return q


def term(clips, verts, weights, want_dverts=True, want_dtrans=True):
    """the two terms at verts (N,V,3) -> dict(dverts, dtrans (None where not asked for), losses (3,)), float32, summed in the
    kernels' order"""
    clips = [int(c) for c in clips]
    N = sum(clips)
    x = np.ascontiguousarray(verts, np.float32)
    assert x.shape[0] == N and x.shape[2] == 3
    V = int(x.shape[1])
    lengths = (C.c_int * len(clips))(*clips)
    dverts = np.full((N, V, 3), np.nan, np.float32) if want_dverts else None
    dtrans = np.full((N, 3), np.nan, np.float32) if want_dtrans else None
    losses = np.full(3, np.nan, np.float32)
    q = block(weights, losses.ctypes.data)
    load().hsv_term(N, len(clips), lengths, C.addressof(q), V, x.ctypes.data, None if dverts is None else dverts.ctypes.data,
                    None if dtrans is None else dtrans.ctypes.data)
    return dict(dverts=dverts, dtrans=dtrans, losses=losses)


def step_total(base, parameter_terms, vertex_terms):
    return np.float32(load().hsv_step_total(float(base), float(parameter_terms), float(vertex_terms)))


def refusal(q, **facts):
    """the text sequence_vertex_args_refusal gives for the block (None: a NULL block), None when it is accepted"""
    full = dict(step=True, num_verts=7, verts=True, handle_meshes=4, num_meshes=4)
    for k, v in facts.items():
        if k not in full:
            raise KeyError(k)
        full[k] = v
    f = (C.c_int * len(FACT_ORDER))(*[int(full[k]) for k in FACT_ORDER])
    msg = load().hsv_refusal(None if q is None else C.addressof(q), f)
    return None if msg is None else msg.decode()


def plan(q, longest=5, num_verts=3889, num_meshes=4):
    out = (C.c_int * 6)()
    load().hsv_plan(None if q is None else C.addressof(q), int(longest), int(num_verts), int(num_meshes), out)
    return dict(launch=bool(out[0]), vel=bool(out[1]), acc=bool(out[2]), grid=(int(out[3]), int(out[4])), partials=int(out[5]))


def sizeof_args():
    return load().hsv_sizeof_args()


def sizeof_sequence_args():
    return load().hsv_sizeof_sequence_args()


def offsets():
    out = (C.c_int * 16)()
    n = load().hsv_offsets(out)
    return list(out[:n])
