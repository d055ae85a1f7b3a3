"""smalfit_plan.h's rules and grids for smalfit_fit_metrics as Python calls: tests/host_metrics_shim.cpp built
and loaded by tests/host_shim.py.  Nothing here needs a GPU."""
from __future__ import annotations

import ctypes as C

from tests import host_shim


def load():
    lib = host_shim.build("host_metrics_shim.cpp", "host_metrics_shim")
    lib.hm_metrics_args_refusal.restype = C.c_char_p
    lib.hm_metrics_args_refusal.argtypes = [C.c_void_p, C.c_int]
    return lib


def refusal(lib, args, max_frames):
    """the text metrics_args_refusal gives for the block, None when it is accepted"""
    msg = lib.hm_metrics_args_refusal(C.byref(args), int(max_frames))
    return None if msg is None else msg.decode()


def grid2(fn, a, b):
    out = (C.c_int * 2)()
    fn(int(a), int(b), out)
    return out[0], out[1]
