"""The test-only host shims: a C++ source of tests/ that wraps headers of smalify_amd/csrc in extern "C" functions, compiled by
g++ into tests/_build/ and loaded through ctypes.  One rule for all of them: built again when the source, a header of
smalify_amd/csrc or include/smalfit.h is newer than the library.  Nothing here needs a GPU."""
from __future__ import annotations

import ctypes as C
import glob
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
BUILD = os.path.join(HERE, "_build")
HEADERS = (os.path.join(HERE, "..", "smalify_amd", "csrc", "*.h"), os.path.join(HERE, "..", "include", "*.h"))


def build(source, name, extra_flags=()):
    """tests/<source> -> tests/_build/lib<name>.so, loaded.  extra_flags: beside -O2 -std=c++17 -shared -fPIC"""
    src, so = os.path.join(HERE, source), os.path.join(BUILD, "lib%s.so" % name)
    deps = [src] + [h for pattern in HEADERS for h in glob.glob(pattern)]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(BUILD, exist_ok=True)
        tmp = "%s.%d.tmp" % (so, os.getpid())
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", *extra_flags, src, "-o", tmp], check=True)
        os.replace(tmp, so)
    return C.CDLL(so)


def mesh3d():
    """tests/host_mesh3d_shim.cpp.  Without contraction: its float32 sums are compared with the kernels' term by term"""
    return build("host_mesh3d_shim.cpp", "host_mesh3d_shim", ("-ffp-contract=off",))
