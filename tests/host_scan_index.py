"""mesh3d_grid.h's scan index -- the library's builder and a host walker that takes every decision from the header -- as Python
calls: tests/host_scan_index_shim.cpp built and loaded by tests/host_shim.py.  Nothing here needs a GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np

from tests import host_shim

_LIB = None
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def load():
    """built without contraction, as the sibling shims are; OpenMP only spreads the queries over the cores"""
    global _LIB
    if _LIB is None:
        lib = host_shim.build("host_scan_index_shim.cpp", "host_scan_index_shim", ("-ffp-contract=off", "-fopenmp"))
        lib.hsi_create.restype = C.c_char_p
        lib.hsi_create.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.POINTER(C.c_void_p)]
        lib.hsi_destroy.argtypes = [C.c_void_p]
        lib.hsi_stats.restype = C.c_ulonglong
        lib.hsi_stats.argtypes = [C.c_void_p, C.c_void_p]
        lib.hsi_cell_edge.restype = C.c_float
        lib.hsi_cell_edge.argtypes = [C.c_void_p]
        lib.hsi_box.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.hsi_csr.argtypes = [C.c_void_p] * 4
        lib.hsi_linear_keys.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p]
        lib.hsi_walk_keys.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
        lib.hsi_ring_cells.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        lib.hsi_query_cell.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.hsi_grid_dims.restype = C.c_float
        lib.hsi_grid_dims.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_float, C.c_void_p]
        lib.hsi_args_refusal.restype = C.c_char_p
        lib.hsi_args_refusal.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong]
        lib.hsi_stats_refusal.restype = C.c_char_p
        lib.hsi_stats_refusal.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        _LIB = lib
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


STAT_KEYS = ("cells", "occupied_cells", "entries", "oversize", "largest_cell")


class Index:
    """one mesh's grid as the library builds it (build_scan_grid) + its staged records"""

    def __init__(self, verts, faces, cell_scale=0.0):
        self.lib = load()
        self.verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
        self.faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
        h = C.c_void_p()
        why = self.lib.hsi_create(_p(self.verts), len(self.verts), _p(self.faces), len(self.faces), float(cell_scale), C.byref(h))
        if why is not None:
            raise ValueError(why.decode())
        self.handle = h

    def __del__(self):
        if getattr(self, "handle", None):
            self.lib.hsi_destroy(self.handle)
            self.handle = None

    def stats(self):
        """the dict engine.MeshTargets.index_stats gives for this mesh"""
        out = (C.c_int * 8)()
        nbytes = self.lib.hsi_stats(self.handle, out)
        d = {"dims": tuple(out[:3]), "bytes": int(nbytes)}
        d.update(zip(STAT_KEYS, out[3:8]))
        return d

    @property
    def cell_edge(self):
        return float(self.lib.hsi_cell_edge(self.handle))

    def box(self):
        lo, hi = np.empty(3, np.float32), np.empty(3, np.float32)
        self.lib.hsi_box(self.handle, _p(lo), _p(hi))
        return lo, hi

    def csr(self):
        s = self.stats()
        off, face, over = np.empty(s["cells"] + 1, np.int32), np.empty(max(s["entries"], 1), np.int32), np.empty(max(s["oversize"], 1), np.int32)
        self.lib.hsi_csr(self.handle, _p(off), _p(face), _p(over))
        return off, face[:s["entries"]], over[:s["oversize"]]

    def _queries(self, q, normals):
        q = np.ascontiguousarray(q, np.float32).reshape(-1, 3)
        u = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        return q, u

    def linear_keys(self, q, normals=None, cc=0.0):
        """the linear scan's 64-bit key of every query (all ones: none), over all records; normals: the compatible scan"""
        q, u = self._queries(q, normals)
        keys = np.empty(len(q), np.uint64)
        self.lib.hsi_linear_keys(self.handle, len(q), _p(q), _p(u) if u is not None else None, int(u is not None), float(cc), _p(keys))
        return keys

    def walk_keys(self, q, normals=None, cc=0.0, tau2=np.inf):
        """-> (the walk's keys, how): how % 100 = rings walked, how // 100 % 10 = 1 when it fell back to the linear scan,
        how // 1000 = 1 when the truncation ended it"""
        q, u = self._queries(q, normals)
        keys, how = np.empty(len(q), np.uint64), np.empty(len(q), np.int32)
        self.lib.hsi_walk_keys(self.handle, len(q), _p(q), _p(u) if u is not None else None, int(u is not None), float(cc), float(tau2),
                               _p(keys), _p(how))
        return keys, how

    def ring_cells(self, c, r):
        c = np.ascontiguousarray(c, np.int32)
        out = np.empty((2 * r + 1) ** 3, np.int32)
        n = self.lib.hsi_ring_cells(self.handle, _p(c), int(r), _p(out))
        return out[:n]

    def query_cell(self, q):
        q, c = np.ascontiguousarray(q, np.float32), np.empty(3, np.int32)
        self.lib.hsi_query_cell(self.handle, _p(q), _p(c))
        return c


def key_d2(keys):
    """the float32 d^2 in the high half of every key"""
    return (np.asarray(keys, np.uint64) >> np.uint64(32)).astype(np.uint32).view(np.float32)


def key_face(keys):
    return (np.asarray(keys, np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.int64)


def grid_dims(extent, area, faces, scale):
    """scan_grid_dims -> (h, dims)"""
    e, d = np.ascontiguousarray(extent, np.float32), np.empty(3, np.int32)
    h = load().hsi_grid_dims(_p(e), float(area), int(faces), float(scale), _p(d))
    return float(h), tuple(int(x) for x in d)


def constants():
    f, i = (C.c_float * 3)(), (C.c_int * 5)()
    load().hsi_constants(f, i)
    return dict(cell_scale=f[0], slack_ulps=f[1], bound_ulps=f[2], max_dim=i[0], max_cells=i[1], oversize_cells=i[2], max_rings=i[3],
                grid_queries=i[4])


def max_rings(faces):
    """scan_max_rings: the last ring a walk over a mesh of `faces` triangles visits before the linear scan"""
    return int(load().hsi_max_rings(int(faces)))


def launch_grids(V, N):
    out = (C.c_int * 4)()
    load().hsi_launch_grids(int(V), int(N), out)
    return (out[0], out[1]), (out[2], out[3])


def args_refusal(args, verts):
    v = np.ascontiguousarray(verts, np.float32)
    msg = load().hsi_args_refusal(C.byref(args), _p(v), v.size)
    return None if msg is None else msg.decode()


def stats_refusal(stats, has_index, mesh, num_meshes):
    msg = load().hsi_stats_refusal(C.byref(stats) if stats is not None else None, int(has_index), int(mesh), int(num_meshes))
    return None if msg is None else msg.decode()


def offsets():
    out = (C.c_int * 16)()
    n = load().hsi_offsets(out)
    return list(out[:n])
