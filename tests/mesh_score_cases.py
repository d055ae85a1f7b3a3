"""The expected values and the cases of smalfit_mesh_score, shared by tests/test_mesh_score_cpu.py (the host shim) and
tests/test_gpu_mesh_score.py (HIP through the C-ABI).  Nothing here asserts or needs a GPU.

The reference is a float64 numpy brute force written from the definition include/smalfit.h words (test infrastructure; the
reference project has no evaluation code for its 3-D fitter):

  distance(p, (a, b, c)) = sqrt of the minimum of
    - the three squared point-to-segment distances, parameter clamped to [0, 1], a zero-length segment being its end point;
    - the squared distance to the plane when n = (b - a) x (c - a) != 0 and the three edge functions against n are >= 0.

Errors are counted in ulp(L) = 2^-23 L, L = the largest coordinate magnitude of the points involved: the float32 form
subtracts coordinates of that size before anything else, so its absolute error scales with L and not with the distance.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from smalify_amd import _lib
from tests import mesh3d_forms as mf

QUERIES = 64                       # kMeshQueries: queries per block of mesh3d_surface_dist_kernel
# the accuracy study's inputs: 2 M near-surface pairs, slivers included (restated from the measurement the definition was chosen by)
ACCURACY_PAIRS = 2_000_000
ACCURACY_SEED = 0
NEAR_SURFACE_SIGMA = 1e-4
SHIM_BAR_FACTOR = 2.0              # CPU: the shim stays within 2 x its recorded deviation ...
REGION_WALK_FLOOR = 64.0           # ... and in any case below this many ulp(L): a region-walk implementation measures 3e4
DEVICE_FACTOR_OVER_SHIM = 4.0      # GPU: 4 x the shim's recorded deviation (room for the device's own fma contraction) ...
DEVICE_RATCHET = 3.0               # ... and 3 x the device's own recorded deviation


# ---------------------------------------------------------------------------------------------------------------
# float64 reference
# ---------------------------------------------------------------------------------------------------------------
def _seg2(p, a, b):
    ab = b - a
    l2 = (ab * ab).sum(-1)
    with np.errstate(all="ignore"):
        t = np.where(l2 > 0, ((p - a) * ab).sum(-1) / np.where(l2 > 0, l2, 1.0), 0.0)
    t = np.clip(t, 0.0, 1.0)
    r = p - (a + t[..., None] * ab)
    return (r * r).sum(-1)


def point_triangle_dist(p, a, b, c):
    """float64 distance of broadcastable (..., 3) arrays, by the definition above"""
    p, a, b, c = (np.asarray(x, np.float64) for x in (p, a, b, c))
    d2 = np.minimum(np.minimum(_seg2(p, a, b), _seg2(p, b, c)), _seg2(p, c, a))
    n = np.cross(b - a, c - a)
    nn = (n * n).sum(-1)
    s0 = (np.cross(b - a, p - a) * n).sum(-1)
    s1 = (np.cross(c - b, p - b) * n).sum(-1)
    s2 = (np.cross(a - c, p - c) * n).sum(-1)
    inside = (nn > 0) & (s0 >= 0) & (s1 >= 0) & (s2 >= 0)
    h = ((p - a) * n).sum(-1)
    with np.errstate(all="ignore"):
        dp = np.where(nn > 0, h * h / np.where(nn > 0, nn, 1.0), np.inf)
    return np.sqrt(np.where(inside, np.minimum(dp, d2), d2))


def surface_dist(q, verts, faces, pair_budget=1 << 20):
    """(len(q),) float64: least distance from every query to the triangles, in chunks of about pair_budget pairs"""
    q = np.asarray(q, np.float64).reshape(-1, 3)
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b, c = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
    step = max(1, pair_budget // max(len(f), 1))
    out = np.empty(len(q))
    for s in range(0, len(q), step):
        out[s:s + step] = point_triangle_dist(q[s:s + step, None, :], a, b, c).min(1)
    return out


def surface_dist_culled(q, verts, faces, block=256):
    """surface_dist for whole meshes, within seconds: the same float64 pair function, evaluated only on the pairs that can hold
    the minimum.  A triangle's centroid lies on it, so the least centroid distance bounds a query's distance from above; a
    triangle whose bounding sphere (centroid, farthest corner) lies beyond that bound cannot be the nearest.  The culling is
    conservative (1e-9 slack on distances of order 1): tests/test_mesh_score_cpu.py checks it equals the brute force"""
    q = np.asarray(q, np.float64).reshape(-1, 3)
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    cen = (a + b + c) / 3.0
    rad = np.sqrt(np.maximum.reduce([((x - cen) ** 2).sum(-1) for x in (a, b, c)]))
    c2 = (cen * cen).sum(-1)
    out = np.empty(len(q))
    for s in range(0, len(q), block):
        qb = q[s:s + block]
        dc = np.sqrt(np.maximum((qb * qb).sum(-1)[:, None] + c2[None] - 2.0 * qb @ cen.T, 0.0))
        keep = dc - rad[None] <= dc.min(1)[:, None] + 1e-9
        qi, fi = np.nonzero(keep)                                        # row-major: qi ascending, every query at least once
        d = point_triangle_dist(qb[qi], a[fi], b[fi], c[fi])
        out[s:s + block] = np.minimum.reduceat(d, np.searchsorted(qi, np.arange(len(qb))))
    return out


def box_surface_dist(p, lo, hi):
    """distance from p to the SURFACE of the axis-aligned box [lo, hi], closed form: outside the solid the distance to the
    box, inside it the distance to the nearest face"""
    p, lo, hi = (np.asarray(x, np.float64) for x in (p, lo, hi))
    gap = np.maximum(np.maximum(lo - p, p - hi), 0.0)
    outside = np.sqrt((gap * gap).sum(-1))
    inside = np.minimum((p - lo).min(-1), (hi - p).min(-1))
    return np.where((gap > 0).any(-1), outside, inside)


def ulp_l(*arrays):
    """2^-23 x the largest coordinate magnitude over all the arrays (one value)"""
    return 2.0 ** -23 * max(float(np.abs(np.asarray(x, np.float64)).max()) for x in arrays)


def deviation_ulp(got32, want64, L_ulp):
    return float((np.abs(np.asarray(got32, np.float64) - want64) / L_ulp).max())


def near_surface_pairs(count=ACCURACY_PAIRS, seed=ACCURACY_SEED):
    """float32 (p, a, b, c): a in [-1, 1]^3, b and c within [-1, 1]^3 of a (coordinates in [-2, 2], every shape of triangle,
    slivers included), p = a + u (b - a) + v (c - a) + 1e-4 x normal noise with u, v in [-0.2, 1.2]: within ~1e-4 of the
    plane, inside and around the triangle"""
    rs = seed if isinstance(seed, np.random.RandomState) else np.random.RandomState(seed)
    a = rs.uniform(-1, 1, (count, 3)).astype(np.float32)
    b = (a + rs.uniform(-1, 1, (count, 3))).astype(np.float32)
    c = (a + rs.uniform(-1, 1, (count, 3))).astype(np.float32)
    u, v = rs.uniform(-0.2, 1.2, (count, 1)), rs.uniform(-0.2, 1.2, (count, 1))
    p = (a + u * (b - a) + v * (c - a) + NEAR_SURFACE_SIGMA * rs.randn(count, 3)).astype(np.float32)
    return p, a, b, c


def accuracy_pairs():
    """the 2 M pairs the definition was chosen by: near_surface_pairs' recipe on RandomState(0) after the draws of the three
    studies that preceded it in that measurement (generic, near-surface, small triangles: the worst deviation is heavy-tailed
    over slivers -- 28 to 66 ulp(L) over other draws -- so the stream is restated, not only the recipe)"""
    n = ACCURACY_PAIRS
    rs = np.random.RandomState(ACCURACY_SEED)
    for study in ("generic", "near-surface", "small triangles"):
        for _ in range(3):
            rs.uniform(-1, 1, (n, 3))
        if study == "near-surface":
            rs.uniform(-0.2, 1.2, (n, 1)), rs.uniform(-0.2, 1.2, (n, 1)), rs.randn(n, 3)
        else:
            rs.uniform(-1, 1, (n, 3))
    return near_surface_pairs(n, rs)


def pair_ulp(p, a, b, c):
    """ulp(L) of every pair: L = the largest coordinate magnitude of its four points"""
    L = np.maximum.reduce([np.abs(np.asarray(x, np.float64)).max(-1) for x in (p, a, b, c)])
    return L * 2.0 ** -23


def region_walk_dist32(p, a, b, c):
    """Ericson's closest point on a triangle evaluated in float32 numpy: what NOT to implement.  Only here so that the CPU
    test can show the bar tells the two forms apart"""
    dt = np.float32
    p, a, b, c = (np.asarray(x, dt) for x in (p, a, b, c))
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = (ab * ap).sum(-1), (ac * ap).sum(-1)
    bp = p - b
    d3, d4 = (ab * bp).sum(-1), (ac * bp).sum(-1)
    cp = p - c
    d5, d6 = (ab * cp).sum(-1), (ac * cp).sum(-1)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    out, done = np.zeros_like(p), np.zeros(len(p), bool)

    def put(m, val):
        m = m & ~done
        out[m] = val[m]
        done[:] |= m
    with np.errstate(all="ignore"):
        put((d1 <= 0) & (d2 <= 0), a)
        put((d3 >= 0) & (d4 <= d3), b)
        put((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + (d1 / (d1 - d3))[:, None] * ab)
        put((d6 >= 0) & (d5 <= d6), c)
        put((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + (d2 / (d2 - d6))[:, None] * ac)
        w = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        put((va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0), b + w[:, None] * (c - b))
        den = dt(1) / (va + vb + vc)
        put(np.ones(len(p), bool), a + (vb * den)[:, None] * ab + (vc * den)[:, None] * ac)
    return np.sqrt(((p - out) ** 2).sum(-1))


# ---------------------------------------------------------------------------------------------------------------
# closed forms on the triangle (0,0,0) (1,0,0) (0,1,0)
# ---------------------------------------------------------------------------------------------------------------
UNIT_TRIANGLE = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
_R2 = np.sqrt(2.0)
# (region, query in the plane, in-plane distance): one per Voronoi region of the triangle
UNIT_REGIONS = (
    ("inside", (0.25, 0.25), 0.0),
    ("edge ab", (0.5, -0.75), 0.75),
    ("edge ca", (-0.5, 0.25), 0.5),
    ("edge bc", (1.0, 1.0), 1.0 / _R2),
    ("corner a", (-0.75, -1.0), 1.25),
    ("corner b", (2.0, -0.25), np.hypot(1.0, 0.25)),
    ("corner c", (-0.5, 2.5), np.hypot(0.5, 1.5)),
)
UNIT_HEIGHTS = (0.0, 0.5, -0.5)     # in the plane, above, below
# exactly 0: on a corner, on an edge, in the interior
UNIT_ZEROS = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0.5, 0, 0), (0, 0.25, 0), (0.5, 0.5, 0), (0.25, 0.25, 0), (0.125, 0.5, 0))

# degenerate triangles: (name, corners, the segment [s0, s1] they are)
DEGENERATE = (
    ("collinear", [[0, 0, 0], [2, 0, 0], [1, 0, 0]], ([0, 0, 0], [2, 0, 0])),
    ("collinear, oblique", [[0, 0, 0], [0.5, 0.5, 1], [1.5, 1.5, 3]], ([0, 0, 0], [1.5, 1.5, 3])),
    ("two coincident (a = b)", [[1, 1, 0], [1, 1, 0], [1, 3, 0]], ([1, 1, 0], [1, 3, 0])),
    ("two coincident (b = c)", [[0, 0, 1], [2, 0, 1], [2, 0, 1]], ([0, 0, 1], [2, 0, 1])),
    ("two coincident (c = a)", [[0, 0, 1], [0, 2, 1], [0, 0, 1]], ([0, 0, 1], [0, 2, 1])),
    ("three coincident", [[0.5, -1, 2], [0.5, -1, 2], [0.5, -1, 2]], ([0.5, -1, 2], [0.5, -1, 2])),
)
DEGENERATE_QUERIES = ((0, 0, 0), (1, 2, 0), (3, -1, 0.5), (-1, -1, -1), (0.5, 0.5, 1), (1, 1, 0), (2, 0, 1), (0.5, -1, 2),
                      (0.75, 0.75, 1.5))


def segment_dist(p, s0, s1):
    return np.sqrt(_seg2(np.asarray(p, np.float64), np.asarray(s0, np.float64), np.asarray(s1, np.float64)))


# ---------------------------------------------------------------------------------------------------------------
# refusals: every rule of smalfit_plan.h::mesh_score_args_refusal in its order
# ---------------------------------------------------------------------------------------------------------------
MAX_MESHES, MAX_POINTS = 3, 130
SIZE_TEXT = "smalfit_mesh_score_args.struct_size does not match this library (built against another smalfit.h?)"


def valid_args(N=2, S=70, T=3, distances=True):
    """a block every rule accepts (pointers are dummies: the rules only ask whether they are given)"""
    a = _lib.MeshScoreArgs()
    a.num_meshes, a.verts, a.sums = N, 0x1000, 0x2000
    if S:
        a.points, a.num_points = 0x3000, S
        a.point_dist = 0x4000 if distances else None
    a.vert_dist = 0x5000 if distances else None
    a.num_thresholds = T
    for i in range(T):
        a.thresholds[i] = 0.01 * (i + 1)
    a.within = 0x6000 if T else None
    return a


def _set(**kw):
    def change(a):
        for k, v in kw.items():
            setattr(a, k, v)
    change.fields = frozenset(kw)
    return change


def _threshold(i, value):
    def change(a):
        a.thresholds[i] = value
    change.fields = frozenset(["thresholds"])
    return change


# (name, change to a valid block, targets' mesh count or None = num_meshes, text) in the order of the rules: a block that
# breaks rules i and j > i is refused with the text of rule i
REFUSALS = (
    ("struct_size", _set(struct_size=C.sizeof(_lib.MeshScoreArgs) - 8), None, SIZE_TEXT),
    ("num_meshes zero", _set(num_meshes=0), None, "num_meshes exceeds the objective's max_meshes"),
    ("num_meshes above capacity", _set(num_meshes=MAX_MESHES + 1), MAX_MESHES + 1, "num_meshes exceeds the objective's max_meshes"),
    ("target count", _set(), 1, "number of target meshes differs from num_meshes"),
    ("verts missing", _set(verts=None), None, "verts / sums missing"),
    ("sums missing", _set(sums=None), None, "verts / sums missing"),
    ("num_points without points", _set(points=None, point_dist=None), None, "num_points must be 0 without points"),
    ("point_dist without points", _set(points=None, num_points=0), None, "point_dist given without points"),
    ("num_points zero", _set(num_points=0), None, "points need 1 <= num_points <= max_points"),
    ("num_points above capacity", _set(num_points=MAX_POINTS + 1), None, "points need 1 <= num_points <= max_points"),
    ("num_thresholds negative", _set(num_thresholds=-1), None, "num_thresholds must be 0..8"),
    ("num_thresholds nine", _set(num_thresholds=9), None, "num_thresholds must be 0..8"),
    ("threshold zero", _threshold(1, 0.0), None, "every threshold must be finite and > 0"),
    ("threshold negative", _threshold(0, -0.5), None, "every threshold must be finite and > 0"),
    ("threshold inf", _threshold(2, float("inf")), None, "every threshold must be finite and > 0"),
    ("threshold nan", _threshold(2, float("nan")), None, "every threshold must be finite and > 0"),
    ("within without thresholds", _set(num_thresholds=0), None, "within given with num_thresholds = 0"),
)
RULE_ORDER = tuple(dict.fromkeys(r[3] for r in REFUSALS))


# ---------------------------------------------------------------------------------------------------------------
# meshes of the GPU cases
# ---------------------------------------------------------------------------------------------------------------
def soup(F, seed, extent=1.0, size=0.3):
    """F unconnected triangles around the unit ribbon: (3F, 3) float32 vertices, (F, 3) faces.  Every fifth triangle is a
    sliver (its third corner almost on the line of the other two) and, from 8 faces on, one is collinear"""
    rs = np.random.RandomState(seed)
    a = rs.uniform(-extent, extent, (F, 3))
    b = a + rs.uniform(-size, size, (F, 3))
    c = a + rs.uniform(-size, size, (F, 3))
    sl = np.arange(F) % 5 == 4
    c[sl] = a[sl] + 0.7 * (b[sl] - a[sl]) + 1e-5 * rs.randn(int(sl.sum()), 3)
    v = np.stack([a, b, c], 1).astype(np.float32)
    if F >= 8:
        v[7, 2] = (v[7, 0] + (v[7, 1] - v[7, 0]) * np.float32(0.5))
        v[7, 1] = v[7, 0] + (v[7, 2] - v[7, 0]) * np.float32(2.0)        # collinear up to rounding: zero or near-zero normal
    return v.reshape(-1, 3), np.arange(3 * F, dtype=np.int32).reshape(F, 3)


def points_near(verts, faces, S, seed, sigma=0.02):
    """S float32 points around the surface: barycentric samples of random faces plus noise"""
    rs = np.random.RandomState(seed)
    v, f = np.asarray(verts, np.float64), np.asarray(faces)
    fi = rs.randint(0, len(f), S)
    w = rs.dirichlet((1.0, 1.0, 1.0), S)
    p = (w[:, :, None] * v[f[fi]]).sum(1)
    return (p + sigma * rs.randn(S, 3)).astype(np.float32)


CUBE_VERTS = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)     # index = 4x + 2y + z
CUBE_FACES = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6],
                       [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)
CUBE_SHIFT = np.array([0.25, 0.5, -0.125], np.float32)       # dyadic: the translated copy is exact in float32


CUBE_SHIFTS = (CUBE_SHIFT, np.array([-0.5, 0.25, 1.5], np.float32))


def scanned_counts(chunk):
    """triangle counts that reach every branch of the scan: waves with an empty quarter, one chunk short, full, one over, and
    a third chunk"""
    return (1, 2, 3, 5, chunk - 1, chunk, chunk + 1, 2 * chunk + 3)


QUERY_COUNTS = (1, 63, 64, 65, 130)


def ribbon(V, seed):
    return mf.ribbon(V, seed)
