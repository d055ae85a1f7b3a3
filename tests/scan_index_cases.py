"""Targets and query placements of the scan-index tests (tests/test_scan_index_cpu.py, tests/test_gpu_scan_index.py): the same lists
on the host walker and on the device.  Every comparison those tests make is between two paths of one build -- the walk over the
grid against the linear scan -- and is bit for bit, so nothing here is a reference value."""
from __future__ import annotations

import numpy as np

from tests import mesh_score_cases as mc

TARGET_FACES = (1, 2, 7, 513, 1280)
QUERY_COUNTS = (3, 4, 5, 65, 130)          # kScanGridQueries = 4 queries a block: one short, full, one over, and partial last blocks
PAIR_SCALE = 1.4142135                     # cell_scale at which the two-triangle target's cell edge is exactly 1


def icosphere(level):
    """the unit icosphere: 20 x 4^level faces, consistently wound outward"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                  [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], np.float64)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
                  [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]], np.int32)
    from smalify_amd.fitter_3d.utils import subdivide_mesh
    for _ in range(level):
        v, f = subdivide_mesh(v, f, 1)
        v = v.astype(np.float64)
    v = v / np.linalg.norm(v, axis=1, keepdims=True)
    return v.astype(np.float32), f


def pair(swapped=False):
    """two triangles either side of the edge x = 1 of the plane z = 0; at PAIR_SCALE the grid is 2 x 1 x 1 with that edge on the
    cell boundary, and every point of the plane x = 1 is equally far from both"""
    v = np.array([[0, 0.5, 0], [1, 0, 0], [1, 1, 0], [2, 0.5, 0]], np.float32)
    f = np.array([[0, 1, 2], [3, 2, 1]], np.int32)
    return v, (f[::-1].copy() if swapped else f)


def target(F):
    """(verts, faces) of the F-face target: one triangle, the pair, triangle soups with slivers and a collinear face, the icosphere"""
    if F == 1:
        return np.array([[0.1, 0.2, 0.3], [0.9, 0.1, 0.4], [0.3, 0.8, 0.2]], np.float32), np.array([[0, 1, 2]], np.int32)
    if F == 2:
        return pair()
    if F == 1280:
        return icosphere(3)
    return mc.soup(F, seed=F)


def flat_target():
    """a 12 x 12 grid of the plane z = 0.25: zero extent along z, one cell there"""
    n = 12
    x, y = np.meshgrid(np.arange(n + 1, dtype=np.float32) / n, np.arange(n + 1, dtype=np.float32) / n, indexing="ij")
    v = np.stack([x.ravel(), y.ravel(), np.full(x.size, 0.25, np.float32)], 1)
    i = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None]).ravel()
    f = np.concatenate([np.stack([i, i + n + 1, i + n + 2], 1), np.stack([i, i + n + 2, i + 1], 1)]).astype(np.int32)
    return v.astype(np.float32), f


def degenerate_target():
    """zero-area and collinear triangles among ordinary ones"""
    v, f = mc.soup(40, seed=3)
    v = v.copy()
    v[3 * 2 + 1] = v[3 * 2]
    v[3 * 2 + 2] = v[3 * 2]                                   # face 2: a point
    v[3 * 5 + 2] = v[3 * 5]                                   # face 5: a segment, two corners coincide
    v[3 * 9 + 2] = (v[3 * 9] + v[3 * 9 + 1]) * np.float32(0.5)  # face 9: collinear
    return v, f


def oversize_target():
    """one triangle spanning the whole box among 500 small ones: it goes on the oversize list"""
    v, f = mc.soup(500, seed=11, extent=1.0, size=0.05)
    big = np.array([[-1.2, -1.2, -1.2], [1.2, 1.2, -1.0], [-1.0, 1.2, 1.2]], np.float32)
    return np.concatenate([v, big]), np.concatenate([f, [[len(v), len(v) + 1, len(v) + 2]]]).astype(np.int32)


def box_directions():
    """the 26 ways out of a box: through its 6 faces, 12 edges and 8 corners"""
    return np.array([[x, y, z] for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)], np.float32)


def placements(verts, faces, lo, hi, cell_edge, count, seed=0, special=True):
    """`count` float32 queries round the target whose grid box is [lo, hi] with cells of `cell_edge`, the kinds interleaved so that
    a short list has one of each: inside the box; outside through each of the 26 directions (near and a box away); exactly on cell
    boundaries; exactly on target vertices (d^2 = 0); near the surface; at 100 x the extent (the fallback); with `special`, NaN
    and +-inf coordinates (no key)"""
    rs = np.random.RandomState(seed)
    v = np.asarray(verts, np.float32)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ext = np.maximum(hi - lo, 1e-3)
    mid, emax = 0.5 * (lo + hi), float(ext.max())
    dirs = box_directions()
    kinds = []
    kinds.append(lambda i: lo + rs.uniform(0, 1, 3) * (hi - lo))                                             # inside
    kinds.append(lambda i: mid + dirs[i % 26] * (0.5 * ext + emax * (0.05 if (i // 26) % 2 == 0 else 1.0)) +
                 (dirs[i % 26] == 0) * rs.uniform(-0.4, 0.4, 3) * ext)                                    # outside
    kinds.append(lambda i: lo + np.floor(rs.uniform(0, 1, 3) * (hi - lo) / cell_edge) * np.float64(np.float32(cell_edge)))   # cell boundaries
    kinds.append(lambda i: v[rs.randint(len(v))].astype(np.float64))                                         # target vertices
    kinds.append(lambda i: mc.points_near(v, faces, 1, rs.randint(1 << 30), sigma=0.02 * emax)[0].astype(np.float64))
    kinds.append(lambda i: mid + dirs[i % 26] * 100.0 * emax)                                                # far: the fallback
    out = np.empty((count, 3), np.float32)
    for i in range(count):
        out[i] = kinds[i % len(kinds)](i // len(kinds))
    if special and count >= 16:
        out[count - 3] = (np.nan, 0.0, 0.0)
        out[count - 2] = (0.0, np.inf, 0.0)
        out[count - 1] = (0.0, 0.0, -np.inf)
    return out


def unit_normals(count, seed):
    rs = np.random.RandomState(seed)
    u = rs.randn(count, 3)
    return (u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32)


def sliver_scene(faces=5000, per_face=40, seed=5):
    """the near-surface recipe of tests/mesh_score_cases.py (near_surface_pairs: every shape of triangle, slivers included) as ONE
    mesh: `faces` unconnected triangles and faces x per_face queries, each within ~1e-4 of the plane of its own triangle, inside
    and around it"""
    rs = np.random.RandomState(seed)
    _, a, b, c = mc.near_surface_pairs(faces, rs)
    v = np.stack([a, b, c], 1).reshape(-1, 3)
    f = np.arange(3 * faces, dtype=np.int32).reshape(faces, 3)
    n = faces * per_face
    own = np.repeat(np.arange(faces), per_face)
    u, w = rs.uniform(-0.2, 1.2, (n, 1)), rs.uniform(-0.2, 1.2, (n, 1))
    q = (a[own] + u * (b[own] - a[own]) + w * (c[own] - a[own]) + mc.NEAR_SURFACE_SIGMA * rs.randn(n, 3)).astype(np.float32)
    return v, f, q


def standin(subdiv=0):
    """the stand-in SMAL-topology template, subdivided `subdiv` times: 7774 x 4^subdiv faces"""
    from smalify_amd import synthetic
    from smalify_amd.fitter_3d.utils import subdivide_mesh
    md = synthetic.synthetic_model(seed=0, shape_family_id=-1)
    return subdivide_mesh(np.asarray(md.v_template, np.float32), np.asarray(md.faces, np.int32), subdiv)
