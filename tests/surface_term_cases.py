"""The expected values and the cases of the point-to-surface term (smalfit_mesh_surface_eval, smalfit_fit3d_step_surface), shared
by tests/test_surface_term_cpu.py (the host shim) and tests/test_gpu_surface_term.py (HIP through the C-ABI).  Nothing here asserts
or needs a GPU.  Test infrastructure, not the library: a numpy brute force written from the definition include/smalfit.h words,

  d^2(p, (a, b, c)) = the least of the three squared point-to-segment distances (parameter clamped to [0, 1], a zero-length
                      segment being its end point) and, when n = (b - a) x (c - a) != 0 and the three edge functions against n
                      are >= 0, the squared plane distance;
  the closest point = the first of (ab, bc, ca, plane) to reach that least value: barycentrics (1 - t, t, 0) on the edge of a
                      segment, (s1, s2, s0) / (s0 + s1 + s2) for the plane; residual r = p - q from the winner's own terms;
  nearest face      = the lowest face index among equal d^2;
  L_ps, L_vs, the term and its gradient by the envelope theorem (2/(N V) r at a vertex; -2/(N S) b_i r at the corners of a
  point's winning face),

evaluated in float64 (the oracle) or, by the same code, in float32 (the yardstick: what ANY float32 evaluation of these formulas
may be expected to deviate by; the device differs from it in fma contraction and summation order only).

The conditioning rule of every comparison of q or r: with delta = 89 ulp(L) (the device bar of the distance: mesh_score_cases'
DEVICE_FACTOR_OVER_SHIM x the recorded 22.3, rounded as the issue states it), a float32 answer may pick any surface point within
d + delta, which on the convex side lies within sqrt(2 d delta + delta^2) of q.  A query is FLAGGED when float64 finds a face at
distance <= d + delta whose closest point is farther than 2 sqrt(2 d delta + delta^2) from q (a second local minimum: medial
axis, or a bowl); unflagged queries must meet |q_got - q_64| <= 2 sqrt(2 d delta + delta^2) + delta, flagged ones only the
distance bar, and at most 2 % of a case's queries may be flagged.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from smalify_amd import _lib
from tests import mesh_score_cases as mc

DELTA_ULP = 89.0                   # ulp(L): the device bar of a distance
FLAG_CAP = 0.02
STANDIN_NOISE = (0.002, 0.02, 0.1)  # x L: the normal noise of the stand-in queries
STANDIN_QUERIES = 1024
WHOLE_GRADIENT_FACTOR = 4.0        # x the float32 yardstick's deviation
WHOLE_GRADIENT_RATCHET = 3.0       # x the device's own recorded deviation


# ---------------------------------------------------------------------------------------------------------------
# one point against one triangle, any broadcastable shapes
# ---------------------------------------------------------------------------------------------------------------
def _seg(p, s, e):
    d, ev = p - s, e - s
    l2 = (ev * ev).sum(-1)
    one = l2.dtype.type(1)
    with np.errstate(all="ignore"):
        inv = np.where(l2 > 0, one / np.where(l2 > 0, l2, one), l2.dtype.type(0))
    t = np.clip((d * ev).sum(-1) * inv, l2.dtype.type(0), one)
    r = d - t[..., None] * ev
    return t, r, (r * r).sum(-1)


def closest(p, a, b, c, dtype=np.float64):
    """-> dict(d2, bary (...,3), q (...,3), r (...,3), winner (0 ab, 1 bc, 2 ca, 3 plane)) in `dtype`"""
    p, a, b, c = np.broadcast_arrays(*(np.asarray(x, dtype) for x in (p, a, b, c)))
    zero, one = dtype(0), dtype(1)
    t0, r0, d0 = _seg(p, a, b)
    t1, r1, d1 = _seg(p, b, c)
    t2, r2, d2c = _seg(p, c, a)
    dseg = np.minimum(np.minimum(d0, d1), d2c)
    n = np.cross(b - a, c - a)
    nn = (n * n).sum(-1)
    s0 = (np.cross(b - a, p - a) * n).sum(-1)
    s1 = (np.cross(c - b, p - b) * n).sum(-1)
    s2 = (np.cross(a - c, p - c) * n).sum(-1)
    inside = (nn > 0) & (s0 >= 0) & (s1 >= 0) & (s2 >= 0)
    h = ((p - a) * n).sum(-1)
    with np.errstate(all="ignore"):
        inv_nn = np.where(nn > 0, one / np.where(nn > 0, nn, one), zero)
        dp = h * h * inv_nn
        k1 = d1 < d0
        sel = np.where(k1, d1, d0)
        k2 = d2c < sel
        sel = np.where(k2, d2c, sel)
        ssum = s0 + s1 + s2
        kp = inside & (dp < sel) & (ssum > 0)
        isum = np.where(kp, one / np.where(kp, ssum, one), zero)
    k = (h * inv_nn)[..., None]
    z = np.zeros_like(t0)
    bary_seg = np.where(k2[..., None], np.stack([t2, z, one - t2], -1),
                        np.where(k1[..., None], np.stack([z, one - t1, t1], -1), np.stack([one - t0, t0, z], -1)))
    r_seg = np.where(k2[..., None], r2, np.where(k1[..., None], r1, r0))
    bary = np.where(kp[..., None], np.stack([s1, s2, s0], -1) * isum[..., None], bary_seg)
    r = np.where(kp[..., None], k * n, r_seg)
    d2 = np.where(inside, np.minimum(dp, dseg), dseg)
    winner = np.where(kp, 3, np.where(k2, 2, np.where(k1, 1, 0)))
    return dict(d2=d2.astype(dtype), bary=bary.astype(dtype), q=(p - r).astype(dtype), r=r.astype(dtype), winner=winner)


def region_walk_closest(p, a, b, c):
    """the closest point by Voronoi region (Ericson, Real-Time Collision Detection 5.1.5) in float64: another road to q than
    `closest`, which shares its candidates and their order with the library.  Only a cross-check of the oracle: in float32 this
    form loses slivers (tests/mesh_score_cases.py), in float64 it is good to ~1e-11 of the coordinates on the same pairs"""
    p, a, b, c = (np.asarray(x, np.float64) for x in (p, a, b, c))
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
        den = 1.0 / (va + vb + vc)
        put(np.ones(len(p), bool), a + (vb * den)[:, None] * ab + (vc * den)[:, None] * ac)
    return out


def point_from(verts, faces, face, bary):
    """the surface point a (face, barycentrics) pair names, in float64"""
    v = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)[np.asarray(face, np.int64)]]
    return (np.asarray(bary, np.float64)[..., None] * v).sum(-2)


# ---------------------------------------------------------------------------------------------------------------
# queries against a mesh
# ---------------------------------------------------------------------------------------------------------------
def nearest(q, verts, faces, dtype=np.float64, delta=None, pair_budget=1 << 19):
    """every query against every face -> dict(d2, face, bary, q, r) of the winners; with delta (float64 only) also `flagged`
    by the conditioning rule above"""
    qs = np.asarray(q, dtype).reshape(-1, 3)
    v = np.asarray(verts, dtype).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b, c = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
    step = max(1, pair_budget // max(len(f), 1))
    out = dict(d2=np.empty(len(qs), dtype), face=np.empty(len(qs), np.int64), bary=np.empty((len(qs), 3), dtype),
               q=np.empty((len(qs), 3), dtype), r=np.empty((len(qs), 3), dtype))
    if delta is not None:
        out["flagged"] = np.zeros(len(qs), bool)
    for s in range(0, len(qs), step):
        o = closest(qs[s:s + step, None, :], a, b, c, dtype)
        win = np.argmin(o["d2"], 1)                                  # the first among equal values: the lowest face index
        rows = np.arange(len(win))
        out["face"][s:s + step] = win
        for k in ("d2", "bary", "q", "r"):
            out[k][s:s + step] = o[k][rows, win]
        if delta is not None:
            d = np.sqrt(o["d2"][rows, win])
            reach = 2.0 * np.sqrt(2.0 * d * delta + delta * delta)
            near = np.sqrt(o["d2"]) <= (d + delta)[:, None]
            far = np.sqrt(((o["q"] - o["q"][rows, win][:, None, :]) ** 2).sum(-1)) > reach[:, None]
            out["flagged"][s:s + step] = (near & far).any(1)
    return out


def reach(d, delta):
    """how far from q64 an unflagged float32 answer may lie"""
    return 2.0 * np.sqrt(2.0 * d * delta + delta * delta) + delta


def face_dist(q, verts, faces, face):
    """float64 distance from every query to the ONE face named for it"""
    v = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)[np.asarray(face, np.int64)]]
    return mc.point_triangle_dist(np.asarray(q, np.float64), v[:, 0], v[:, 1], v[:, 2])


# ---------------------------------------------------------------------------------------------------------------
# the term and its gradient
# ---------------------------------------------------------------------------------------------------------------
def term(verts, faces, targets, points, w_ps, w_vs, dtype=np.float64):
    """verts (N,V,3), faces (F,3) of the fitted topology, targets: list of N (verts, faces) or None, points (N,S,3) or None
    -> dict(L_ps, L_vs, term, rows (N,2), dverts (N,V,3), dtrans (N,3), point / vert: per mesh the `nearest` dicts)"""
    verts = np.asarray(verts, dtype)
    N, V = verts.shape[:2]
    f = np.asarray(faces, np.int64)
    rows = np.zeros((N, 2), dtype)
    g = np.zeros((N, V, 3), dtype)
    hits_p, hits_v = [], []
    two = dtype(2)
    if w_ps > 0:
        S = np.asarray(points).shape[1]
        for n in range(N):
            o = nearest(points[n], verts[n], f, dtype)
            hits_p.append(o)
            rows[n, 0] = o["d2"].sum(dtype=dtype)
            coef = dtype(w_ps) * two / (dtype(S) * dtype(N))
            for i in range(3):
                np.add.at(g[n], f[o["face"], i], -coef * o["bary"][:, i:i + 1] * o["r"])
    if w_vs > 0:
        for n in range(N):
            o = nearest(verts[n], targets[n][0], targets[n][1], dtype)
            hits_v.append(o)
            rows[n, 1] = o["d2"].sum(dtype=dtype)
            g[n] += dtype(w_vs) * two / (dtype(V) * dtype(N)) * o["r"]
    L_ps = rows[:, 0].sum(dtype=dtype) / dtype(N * np.asarray(points).shape[1]) if w_ps > 0 else dtype(0)
    L_vs = rows[:, 1].sum(dtype=dtype) / dtype(N * V) if w_vs > 0 else dtype(0)
    return dict(L_ps=L_ps, L_vs=L_vs, term=dtype(max(w_ps, 0)) * L_ps + dtype(max(w_vs, 0)) * L_vs, rows=rows, dverts=g,
                dtrans=g.sum(1, dtype=dtype), point=hits_p, vert=hits_v)


def central_difference(verts, faces, targets, points, w_ps, w_vs, u, h=1e-6):
    """(term(verts + h u) - term(verts - h u)) / 2h in float64"""
    v = np.asarray(verts, np.float64)
    up = term(v + h * u, faces, targets, points, w_ps, w_vs)["term"]
    dn = term(v - h * u, faces, targets, points, w_ps, w_vs)["term"]
    return (up - dn) / (2.0 * h)


def smooth_directions(verts, count, seed):
    """`count` smooth random displacement fields over the vertices: low-frequency sines of the coordinates, unit maximum"""
    rs = np.random.RandomState(seed)
    v = np.asarray(verts, np.float64)
    out = []
    for _ in range(count):
        k = rs.uniform(-3, 3, (3, 3))
        ph = rs.uniform(0, 2 * np.pi, 3)
        u = np.sin(v @ k.T + ph) * rs.uniform(0.5, 1.0, 3)
        out.append(u / np.abs(u).max())
    return out


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
def standin_mesh():
    d = np.load(os.path.join(os.path.dirname(_lib.__file__), "data", "synth_mesh.npz"))
    return np.asarray(d["verts"], np.float32), np.asarray(d["faces"], np.int32)


def standin_queries(noise, count=STANDIN_QUERIES, seed=0):
    """barycentric samples of random faces of the stand-in mesh displaced along the face normal by noise x L x a normal draw"""
    v, f = standin_mesh()
    rs = np.random.RandomState(seed)
    L = float(np.abs(v).max())
    fi = rs.randint(0, len(f), count)
    w = rs.dirichlet((1.0, 1.0, 1.0), count)
    tri = v.astype(np.float64)[f[fi]]
    p = (w[:, :, None] * tri).sum(1)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-30)
    return (p + noise * L * rs.randn(count, 1) * n).astype(np.float32)


def region_queries():
    """the seven regions of the unit triangle x three heights -> (names, queries (21,3), closed-form q (21,3))"""
    closed = {"inside": None, "edge ab": (0.5, 0.0), "edge ca": (0.0, 0.25), "edge bc": (0.5, 0.5), "corner a": (0.0, 0.0),
              "corner b": (1.0, 0.0), "corner c": (0.0, 1.0)}
    names, qs, want = [], [], []
    for name, (x, y), _ in mc.UNIT_REGIONS:
        for z in mc.UNIT_HEIGHTS:
            names.append("%s z=%g" % (name, z))
            qs.append((x, y, z))
            cx, cy = (x, y) if closed[name] is None else closed[name]
            want.append((cx, cy, 0.0))
    return names, np.array(qs, np.float32), np.array(want, np.float64)


CORNER_ORDERS = ((0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2))

# ---------------------------------------------------------------------------------------------------------------
# refusals: every rule of smalfit_plan.h::surface_term_args_refusal in its order
# ---------------------------------------------------------------------------------------------------------------
MAX_MESHES, MAX_POINTS = 3, 130
SIZE_TEXT = "smalfit_surface_term_args.struct_size does not match this library (built against another smalfit.h?)"


def valid_args(N=2, S=70, step=False):
    """a block every rule accepts (pointers are dummies: the rules only ask whether they are given)"""
    a = _lib.SurfaceTermArgs()
    a.num_meshes, a.w_point_surface, a.w_vert_surface = N, 1.0, 0.5
    a.losses, a.rows, a.dverts, a.dtrans = 0x1000, 0x2000, 0x3000, 0x4000
    a.point_face, a.point_bary, a.vert_face, a.vert_bary = 0x5000, 0x6000, 0x7000, 0x8000
    a.point_residual, a.vert_residual, a.step_total = 0xB000, 0xC000, 0xD000
    if not step:
        a.verts, a.points, a.num_points = 0x9000, 0xA000, S
    return a


def facts(targets=True, target_meshes=2, step=False, step_meshes=2, step_points=70, step_has_points=False):
    return dict(max_meshes=MAX_MESHES, max_points=MAX_POINTS, targets=targets, target_meshes=target_meshes, step=step,
                step_meshes=step_meshes, step_points=step_points, step_has_points=step_has_points)


def _set(**kw):
    def change(a):
        for k, v in kw.items():
            setattr(a, k, v)
    return change


# (name, step?, change to a valid block, changed facts, text) in the order of the rules
REFUSALS = (
    ("struct_size", False, _set(struct_size=C.sizeof(_lib.SurfaceTermArgs) - 8), {}, SIZE_TEXT),
    ("num_meshes zero", False, _set(num_meshes=0), {}, "num_meshes exceeds the objective's max_meshes"),
    ("num_meshes above capacity", False, _set(num_meshes=MAX_MESHES + 1), dict(target_meshes=MAX_MESHES + 1),
     "num_meshes exceeds the objective's max_meshes"),
    ("step of another batch", True, _set(), dict(step_meshes=3), "num_meshes differs from the step's"),
    ("no targets", False, _set(), dict(targets=False), "the vertex-surface term needs the target meshes"),
    ("target count", False, _set(), dict(target_meshes=1), "number of target meshes differs from num_meshes"),
    ("losses missing", False, _set(losses=None), {}, "losses missing"),
    ("verts in a step", True, _set(verts=0x9000), {}, "verts and points must be NULL in a step: it uses its own"),
    ("points in a step", True, _set(points=0xA000), {}, "verts and points must be NULL in a step: it uses its own"),
    ("step without points", True, _set(), dict(step_points=0), "the point-surface term needs 1 <= num_points <= max_points"),
    ("step above capacity", True, _set(), dict(step_points=MAX_POINTS + 1), "the point-surface term needs 1 <= num_points <= max_points"),
    ("step with nothing to sample", True, _set(w_vert_surface=0.0), dict(targets=False), "neither target points nor target meshes given"),
    ("step sampling another batch", True, _set(w_vert_surface=0.0), dict(target_meshes=1), "number of target meshes differs from num_meshes"),
    ("verts missing", False, _set(verts=None), {}, "verts missing"),
    ("points missing", False, _set(points=None), {}, "the point-surface term needs 1 <= num_points <= max_points points"),
    ("num_points zero", False, _set(num_points=0), {}, "the point-surface term needs 1 <= num_points <= max_points points"),
    ("num_points above capacity", False, _set(num_points=MAX_POINTS + 1), {},
     "the point-surface term needs 1 <= num_points <= max_points points"),
    ("point_bary alone", False, _set(point_face=None), {}, "point_bary given without point_face"),
    ("vert_bary alone", False, _set(vert_face=None), {}, "vert_bary given without vert_face"),
    ("point_residual alone", False, _set(point_face=None, point_bary=None), {}, "point_residual given without point_face"),
    ("vert_residual alone", False, _set(vert_face=None, vert_bary=None), {}, "vert_residual given without vert_face"),
)
# accepted edges: (name, step?, change, changed facts)
ACCEPTED = (
    ("as is", False, _set(), {}),
    ("a step", True, _set(), {}),
    ("full capacity", False, _set(num_meshes=MAX_MESHES, num_points=MAX_POINTS), dict(target_meshes=MAX_MESHES)),
    ("one point", False, _set(num_points=1), {}),
    ("points only, no targets", False, _set(w_vert_surface=0.0), dict(targets=False)),
    ("points only, targets of another batch", False, _set(w_vert_surface=0.0), dict(target_meshes=1)),
    ("vertices only, no points", False, _set(w_point_surface=0.0, points=None, num_points=0), {}),
    ("both off", False, _set(w_point_surface=0.0, w_vert_surface=-1.0, points=None, num_points=0), dict(targets=False)),
    ("no optional output", False, _set(rows=None, dverts=None, dtrans=None, point_face=None, point_bary=None, vert_face=None,
                                       vert_bary=None, point_residual=None, vert_residual=None, step_total=None), {}),
    ("faces alone", False, _set(point_bary=None, vert_bary=None, point_residual=None, vert_residual=None), {}),
    ("a step with the caller's points, no targets", True, _set(w_vert_surface=0.0), dict(targets=False, step_has_points=True)),
    ("a step without the point term and without points", True, _set(w_point_surface=0.0), dict(step_points=0)),
)


# ---------------------------------------------------------------------------------------------------------------
# the slice rule, restated (kSurfaceTargetBlocks, kSurfaceMinSlice of smalfit_plan.h)
# ---------------------------------------------------------------------------------------------------------------
CUS = 256


def slice_boundaries(faces, slices):
    """first triangle of every slice but the first"""
    span = -(-faces // slices)
    return [k * span for k in range(1, slices) if k * span < faces]
