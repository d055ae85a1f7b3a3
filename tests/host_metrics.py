"""smalfit_plan.h's rules and grids for smalfit_fit_metrics as Python calls: tests/host_metrics_shim.cpp built by g++ the way
tests/host_plan.py builds its shim, loaded through ctypes.  Nothing here needs a GPU."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_metrics_shim.cpp")
SO = os.path.join(HERE, "_build", "libhost_metrics_shim.so")
DEPS = (SRC, os.path.join(HERE, "..", "smalify_amd", "csrc", "smalfit_plan.h"), os.path.join(HERE, "..", "include", "smalfit.h"))


def load():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", SRC, "-o", SO], check=True)
    lib = C.CDLL(SO)
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
