"""The 3-D mesh kernels away from the unit box: the cases, the restated windows and the references of
tests/test_mesh3d_value_forms_cpu.py (the host shims) and tests/test_gpu_mesh3d_value_forms.py (HIP through eng.MeshObjective,
eng.MeshTargets and the C ABI).  Nothing here asserts or needs a GPU.

  A  scale   the same problem at scale 1 and at 2^k: every length among the arguments scales (coordinates, max_dist_*, sigma_*,
             the score thresholds), cosines do not.  A float32 result of degree p in the lengths is then 2^(p k) times the
             unscaled BITS, as long as no intermediate leaves the normal range: `window` restates, from float64 magnitudes of
             the named intermediates of an entry point and their degrees, the k for which that holds.  The normal term is not
             homogeneous (kCosEps2 = 1e-16 is a length^8): it is bit-equal only between scales with the same set of clamped
             pairs, and is held to the float64 reference (the clamp restated, mesh3d_forms.reference) wherever the set changes.
  B  place   geometry on multiples of 2^-7 of extent ~4, shifted by o (1, -1, 0.5), o in 16, 1024, 65536: every shifted input is
             exact in float32, every difference the kernels form is the unshifted one, so whatever is built from differences
             keeps its bits.  The sampler interpolates absolute coordinates: held to float64 under the YARD rule.
  C  coincidence and collapse   closed forms: a fit on its target, vertices made coincident or a face folded by deform_verts.

The float64 references are those of mesh3d_forms (objective), surface_term_cases / surface_gate_cases / robust_cases (surface
term), chamfer_gate_cases (chamfer matches) and mesh_score_cases (distances)."""
from __future__ import annotations

import math
from dataclasses import dataclass, replace

import numpy as np

from oracle import mesh3d_oracle as mo
from tests import chamfer_gate_cases as cgc
from tests import mesh3d_cases as m3
from tests import mesh3d_forms as mf
from tests import mesh_score_cases as msc
from tests import robust_cases as rc
from tests import surface_gate_cases as sgc
from tests import surface_term_cases as stc
from tests import template_cases as tc

SCALES = (-12, -7, 3, 10)                 # k of the GPU test
OFFSETS = (16, 1024, 65536)               # o of the GPU test
DIRECTION = np.array([1.0, -1.0, 0.5])
LATTICE = 2.0 ** -7
FLT_MIN, FLT_MAX = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)
EPS32 = float(np.finfo(np.float32).eps)
# one k outside the window of each entry point (CPU only): the whole result, not only its smallest intermediate, has left the
# normal range there -- d^2 of the chamfer term, the plane product h h / |n|^2 and |n|^2 of the surface distance, a coordinate,
# w1 w2 of the normal term (beyond its window's upper edge r^3 underflows first: that costs the gradient, not the value)
OUTSIDE = {"eval": -80, "surface_dist": (-24, 40), "sample": -140, "normal": 20}
V_RIBBON, S_RIBBON = 130, 70
TARGET_FACES = {1: (513,), 3: (7, 513, 64)}          # the ragged batch: one short chunk, one past the chunk, one block
CLAMP_MARGIN = 4.0                        # no pair of a normal-term case within this factor of kCosEps2
YARD, RATCHET, FLOOR_VALUE, FLOOR_GRAD = 2.0, 3.0, 1e-6, 1e-5      # the project's YARD rule (tests/value_forms.py)
SAMPLER_BAR = 1e-6                        # tests/test_gpu_mesh3d_forms.py: the sampler against the shim, absolute at extent 1
LOSS_BAR, DVERTS_BAR = 2e-5, mf.DVERTS_TOL

# ---- what a result is multiplied by under a scale 2^k: key -> degree p (None: identical, an index, a flag, a cosine or a weight)
# one-hot weights of MeshObjective.eval: term -> (weights, index into losses, degree of the loss, degree of dverts and dtrans)
ONE_HOT = {"chamfer": ((1.0, 0.0, 0.0, 0.0), 0, 2, 1), "edge": ((0.0, 1.0, 0.0, 0.0), 1, 2, 1),
           "laplacian": ((0.0, 0.0, 0.0, 1.0), 3, 1, 0), "normal": ((0.0, 0.0, 1.0, 0.0), 2, 0, -1)}
SURFACE_DEGREES = dict(losses=2, rows=2, dverts=1, dtrans=1, point_face=None, point_bary=None, point_residual=1, vert_face=None,
                       vert_bary=None, vert_residual=1, kept=None, point_kept=None, vert_kept=None, vert_normals=None,
                       surface_weight_sums=None, point_weights=None, vert_weights=None)
GATED_EVAL_DEGREES = dict(losses=2, dverts=1, dtrans=1, verts=1, kept=None, point_kept=None, vert_kept=None, point_nn=None, vert_nn=None,
                          chamfer_weight_sums=None, point_weights=None, vert_weights=None)
SCORE_DEGREES = dict(vert_dist=1, point_dist=1, sums=(1, 2, 1), within=None)        # sums: sum d, sum d^2, max d along the last axis
QUERY_DEGREES = dict(face=None, kept=None, d2=2, bary=None, r=1, rho=2, w=None)     # the per-query outputs of the host shims

# lengths among the arguments (float32 values: exact under a power of two)
GATES = dict(max_dist_point=0.25, max_dist_vert=0.375, min_cos_point=0.0, min_cos_vert=-0.25, reject_boundary=True)
SIGMAS = rc.scales(sigma_chamfer_point=0.125, sigma_chamfer_vert=0.25, sigma_surface_point=0.125, sigma_surface_vert=0.25)
THRESHOLDS = (0.0625, 0.25, 1.0)
# (name, gates, robust): plain, each gate, robust, everything
SURFACE_VARIANTS = (("plain", None, None),
                    ("max_dist", dict(max_dist_point=GATES["max_dist_point"], max_dist_vert=GATES["max_dist_vert"]), None),
                    ("min_cos", dict(min_cos_point=GATES["min_cos_point"], min_cos_vert=GATES["min_cos_vert"]), None),
                    ("boundary", dict(reject_boundary=True), None),
                    ("robust", None, SIGMAS),
                    ("all", GATES, SIGMAS))
CHAMFER_GATES = dict(max_dist_point=GATES["max_dist_point"], max_dist_vert=GATES["max_dist_vert"])


def ldexp32(a, e):
    """a 2^e in float32, exact unless it leaves the normal range"""
    with np.errstate(over="ignore", under="ignore"):
        return np.ldexp(np.asarray(a, np.float32), int(e)).astype(np.float32)


def times(a, degree, k):
    """what the unscaled result `a` must be, bit for bit, at scale 2^k: a 2^(degree k); degree None: a itself; a tuple: one degree
    per entry of the last axis"""
    a = np.asarray(a)
    if degree is None:
        return a
    if isinstance(degree, tuple):
        return np.stack([ldexp32(a[..., i], d * k) for i, d in enumerate(degree)], -1)
    return ldexp32(a, degree * k)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def scaled_lengths(d, k, keys):
    """the dict with its lengths (keys) times 2^k, as Python floats holding float32 values"""
    return None if d is None else {key: (float(ldexp32(v, k)) if key in keys else v) for key, v in d.items()}


def scaled_gates(g, k):
    return scaled_lengths(g, k, ("max_dist_point", "max_dist_vert"))


def scaled_sigmas(s, k):
    return scaled_lengths(s, k, rc.KEYS)


# ---------------------------------------------------------------------------------------------------------------
# problems
# ---------------------------------------------------------------------------------------------------------------
@dataclass
class Problem:
    """N fitted meshes of one topology (composed as mesh3d_compose_kernel does: lbs + trans + deform), S points with the unit
    normal and the boundary byte of the target face each lies on, and the N target meshes"""
    name: str
    faces: np.ndarray                 # (F,3) int32
    lbs: np.ndarray                   # (N,V,3) float32
    trans: np.ndarray                 # (N,3) float32
    deform: np.ndarray | None         # (N,V,3) float32
    points: np.ndarray                # (N,S,3) float32
    point_normals: np.ndarray | None  # (N,S,3) float32
    point_boundary: np.ndarray | None  # (N,S) uint8
    targets: list | None              # N (verts float32, faces int32)

    @property
    def N(self):
        return self.lbs.shape[0]

    @property
    def V(self):
        return self.lbs.shape[1]

    @property
    def S(self):
        return self.points.shape[1]

    @property
    def verts(self):
        with np.errstate(over="ignore"):
            v = self.lbs + self.trans[:, None, :]
            return v + self.deform if self.deform is not None else v

    def case(self, weights):
        """the mesh3d_forms.Case of the same inputs"""
        return mf.Case(self.name, self.faces, self.lbs, self.trans, self.deform, self.points, tuple(weights))


def scale(p, k):
    """the problem in another unit of length: every coordinate times 2^k"""
    s = lambda a: None if a is None else ldexp32(a, k)
    return replace(p, name="%s*2^%d" % (p.name, k), lbs=s(p.lbs), trans=s(p.trans), deform=s(p.deform), points=s(p.points),
                   targets=None if p.targets is None else [(s(v), f) for v, f in p.targets])


def shift_vector(o):
    return (o * DIRECTION).astype(np.float32)


def shift(p, o):
    """the problem at another place: the fitted meshes through `trans`, the targets and the points through their coordinates"""
    t = shift_vector(o)
    return replace(p, name="%s+%d" % (p.name, o), trans=p.trans + t, points=p.points + t,
                   targets=None if p.targets is None else [(v + t, f) for v, f in p.targets])


def shift_is_exact(p, o):
    """every input of shift(p, o), and every composed vertex, is the float64 sum: nothing was rounded"""
    q, t = shift(p, o), o * DIRECTION
    ok = np.array_equal(q.trans.astype(np.float64), p.trans.astype(np.float64) + t)
    ok &= np.array_equal(q.points.astype(np.float64), p.points.astype(np.float64) + t)
    for (v, _), (w, _) in zip(p.targets or [], q.targets or []):
        ok &= np.array_equal(w.astype(np.float64), v.astype(np.float64) + t)
    exact = q.lbs.astype(np.float64) + q.trans.astype(np.float64)[:, None] + (0 if q.deform is None else q.deform.astype(np.float64))
    return bool(ok and np.array_equal(q.verts.astype(np.float64), exact))


def on_lattice(a, extent=None):
    a = np.asarray(a, np.float64)
    return bool(np.array_equal(np.round(a / LATTICE) * LATTICE, a) and (extent is None or np.abs(a).max() <= extent))


def _snap(a, factor=2.0):
    return (np.round(np.asarray(a, np.float64) * factor / LATTICE) * LATTICE).astype(np.float32)


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def ribbon_problem(N, lattice=False):
    """N ribbons of 130 vertices against soups of TARGET_FACES[N] faces, 70 points on each soup.  lattice: twice the size (extent
    ~4) with every coordinate snapped to a multiple of 2^-7 -- the normals and boundary bytes are then those of the snapped soups"""
    def make():
        rs = np.random.RandomState(11 + N)
        base, faces = mf.ribbon(V_RIBBON, seed=5)
        lbs = (base[None] + 0.004 * rs.randn(N, V_RIBBON, 3)).astype(np.float32)
        trans = (0.02 * rs.randn(N, 3)).astype(np.float32)
        deform = (0.002 * rs.randn(N, V_RIBBON, 3)).astype(np.float32)
        targets = [msc.soup(F, seed=40 + n) for n, F in enumerate(TARGET_FACES[N])]
        if lattice:
            lbs, trans, deform = _snap(lbs), _snap(trans), _snap(deform)
            targets = [(_snap(v), f) for v, f in targets]
        pts, pn, pb = [], [], []
        for v, f in targets:
            a, b, c, _ = cgc.sample_on(v, f, S_RIBBON, rs)
            pts.append(_snap(a, 1.0) if lattice else a), pn.append(b), pb.append(c)
        return Problem("ribbon_N%d%s" % (N, "_lattice" if lattice else ""), faces, lbs, trans, deform, np.stack(pts), np.stack(pn),
                       np.stack(pb), targets)
    return _cached(("ribbon", N, lattice), make)


def standin_problem():
    """the stand-in (V 3889) against 200 points: the objective only (no target mesh)"""
    def make():
        md, lbs, trans, dfm, pts = m3.objective_problem(1, 200, seed=9)
        return Problem("standin", np.asarray(md.faces, np.int32), lbs, trans, dfm, pts, None, None, None)
    return _cached("standin", make)


def template_problem():
    """the SMAL template (tests/golden/smal_template_mesh.npz), bent, against 200 points near the normalised template"""
    def make():
        tv, tf = tc.target_mesh()
        fit = tc.bent_template()[None]
        pts = msc.points_near(tv, tf, 200, seed=4, sigma=0.01)[None]
        return Problem("template", tf, fit, np.zeros((1, 3), np.float32), None, pts, None, None, None)
    return _cached("template", make)


# ---------------------------------------------------------------------------------------------------------------
# A. windows: the k for which no named intermediate leaves the normal range
# ---------------------------------------------------------------------------------------------------------------
def window(items, finite_only=()):
    """items: (magnitudes, degree) of float32 intermediates at scale 1 -> (lo, hi): for lo <= k <= hi every nonzero one stays
    normal at scale 2^k (m 2^(degree k) in [FLT_MIN, FLT_MAX]).  finite_only: items that need only stay finite (a term whose
    weight is 0 is still evaluated: its underflow is multiplied away, its overflow is 0 x inf in the gradient)"""
    lo, hi = -10 ** 6, 10 ** 6
    for mags, deg in finite_only:
        m = np.abs(np.asarray(mags, np.float64)).ravel()
        m = m[(m > 0) & np.isfinite(m)]
        if deg > 0 and len(m):
            hi = min(hi, math.floor((math.log2(FLT_MAX) - math.log2(m.max())) / deg))
    for mags, deg in items:
        m = np.abs(np.asarray(mags, np.float64)).ravel()
        m = m[(m > 0) & np.isfinite(m)]
        if deg == 0 or not len(m):
            continue
        a = (math.log2(FLT_MIN) - math.log2(m.min())) / deg
        b = (math.log2(FLT_MAX) - math.log2(m.max())) / deg
        if deg < 0:
            a, b = b, a
        lo, hi = max(lo, math.ceil(a)), min(hi, math.floor(b))
    return lo, hi


def _ring_differences(verts, faces):
    e = mo.unique_edges(faces)
    v = np.asarray(verts, np.float64)
    return v[:, e[:, 0]] - v[:, e[:, 1]]


def eval_items(p):
    """nearest_scan: every component difference and its square, every d^2; vertex_ring: the ring's differences, their squares, the
    residual and its squared length; the gradient's coefficient times a difference"""
    v, x = p.verts.astype(np.float64), p.points.astype(np.float64)
    d = v[:, :, None, :] - x[:, None, :, :]
    ring = _ring_differences(v, p.faces)
    lap, _ = mf.laplacian_residual(v, p.faces)
    coef = 2.0 / (max(p.V, p.S) * p.N)
    return [(d, 1), (d * d, 2), ((d * d).sum(-1), 2), (ring, 1), (ring * ring, 2), (lap, 1), ((lap * lap).sum(-1), 2), (coef * d, 1),
            (coef / len(mo.unique_edges(p.faces)) * p.V * ring, 1)]


def surface_items(q, verts, faces):
    """point_scan_tri_dist2 over every (query, face): the segments' d^2 (2), the edge functions and |n|^2 (4), its reciprocal
    (-4), and where the plane candidate is taken the plane product h = distance x twice the area, squared (6)"""
    qs = np.asarray(q, np.float64).reshape(-1, 1, 3)
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    a, b, c = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
    n = np.cross(b - a, c - a)
    nn = (n * n).sum(-1)
    s = [(np.cross(e1 - e0, qs - e0) * n).sum(-1) for e0, e1 in ((a, b), (b, c), (c, a))]
    inside = (nn > 0) & (s[0] >= 0) & (s[1] >= 0) & (s[2] >= 0)
    h = ((qs - a) * n).sum(-1)
    o = stc.closest(qs, a, b, c)
    with np.errstate(divide="ignore"):
        inv = np.where(nn > 0, 1.0 / np.where(nn > 0, nn, 1.0), 0.0)
    return [(o["d2"], 2), (np.stack(s), 4), (nn, 4), (inv, -4), (np.where(inside, h * h, 0.0), 6), (np.where(inside, h, 0.0), 3)]


def surface_term_items(p):
    out = []
    v = p.verts
    for n in range(p.N):
        out += surface_items(p.points[n], v[n], p.faces) + surface_items(v[n], *p.targets[n])
    sig = [rc.s2_of(s) for s in SIGMAS.values()] + [float(np.float32(GATES[k])) ** 2 for k in ("max_dist_point", "max_dist_vert")]
    return out + [(np.array(sig, np.float64), 2)]


def normal_items(verts, faces):
    """face_pair_eval: |n0|^2, |n1|^2, <n0, n1> (4), their product (8), r^2 (-8), r^3 (-12)"""
    pr = mo.face_pairs(faces)
    v = np.asarray(verts, np.float64)
    v0, v1, a, b = (v[:, pr[:, i]] for i in range(4))
    n0, n1 = np.cross(v1 - v0, a - v0), np.cross(b - v0, v1 - v0)
    w1, w2, w12 = (n0 * n0).sum(-1), (n1 * n1).sum(-1), (n0 * n1).sum(-1)
    prod = w1 * w2
    with np.errstate(divide="ignore"):
        r = np.where(prod > 0, 1.0 / np.sqrt(np.where(prod > 0, prod, 1.0)), 0.0)
    return [(w1, 4), (w2, 4), (w12, 4), (prod, 8), (r * r, -8), (r ** 3, -12), (r ** 3 * np.abs(w12), -8)]


def normal_finite_items(verts, faces):
    """what of face_pair_eval must stay finite for a gradient that multiplies it by a zero weight: |n0|^2, |n1|^2, <n0, n1>"""
    return [it for it in normal_items(verts, faces)[:3]]


def eval_window(p):
    """MeshObjective.eval with one-hot weights: the three homogeneous terms normal, the normal term finite"""
    return window(eval_items(p), finite_only=normal_finite_items(p.verts, p.faces))


def sample_items(verts):
    """barycentric_sample: a coordinate, and a coordinate times the smallest nonzero weight -- sqrt(u) (1 - v) >= 2^-12 2^-24 with
    u and v multiples of 2^-24"""
    v = np.asarray(verts, np.float64)
    return [(v, 1), (v * 2.0 ** -36, 1)]


# ---- the normal term: which pairs the clamp holds ----------------------------------------------------------------------------
def clamped_pairs(verts, faces):
    """(pairs under the clamp, pairs, smallest and largest factor between a pair's product and kCosEps2, min product): float64"""
    prod = mf.normal_pair_products(verts, mo.face_pairs(faces))
    with np.errstate(divide="ignore"):
        ratio = np.maximum(prod / mf.COS_EPS2, mf.COS_EPS2 / np.where(prod > 0, prod, 1e-300))
    return int((prod <= mf.COS_EPS2).sum()), prod.size, float(ratio.min()), float(prod.min())


def normal_base_scale(p, lo=-4, hi=12):
    """the least j for which p at 2^j has no clamped pair and min(prod) > 4e-16"""
    for j in range(lo, hi + 1):
        if clamped_pairs(scale(p, j).verts, p.faces)[3] > CLAMP_MARGIN * mf.COS_EPS2:
            return j
    raise ValueError("no scale without a clamped pair")


MIXED_PATCH = 40


def normal_mixed_problem(p):
    """pairs on both sides of the clamp, none within CLAMP_MARGIN of it.  On a real mesh the pair products form a continuum over
    ten decades and every unit of length leaves some pair at the clamp, so the mix is made the way a fit makes it: p without a
    clamped pair, with the MIXED_PATCH vertices nearest vertex 0 collapsed onto it -- every face with two of them has area 0
    exactly, its pairs sit under the clamp with a product of 0, every other pair keeps the base's margin"""
    base = scale(p, normal_base_scale(p) + 2)
    v = base.verts.copy()
    for n in range(p.N):
        near = np.argsort(((v[n].astype(np.float64) - v[n, 0]) ** 2).sum(-1))[:MIXED_PATCH]
        v[n, near] = v[n, 0]
    return replace(base, name=p.name + "_mixed", lbs=v, trans=np.zeros((p.N, 3), np.float32), deform=None)


# ---------------------------------------------------------------------------------------------------------------
# B. the sampler against float64 (it interpolates absolute coordinates)
# ---------------------------------------------------------------------------------------------------------------
def sampler_reference(verts, faces, chosen, u, v, dtype=np.float64):
    """pytorch3d's barycentric map on the faces the sampler chose, u and v its two 24-bit uniforms"""
    vv = np.asarray(verts, dtype)[np.asarray(faces, np.int64)[chosen]]
    su = np.sqrt(np.asarray(u, dtype))
    w0, w1, w2 = dtype(1) - su, su * (dtype(1) - np.asarray(v, dtype)), su * np.asarray(v, dtype)
    return (w0[:, None] * vv[:, 0] + w1[:, None] * vv[:, 1] + w2[:, None] * vv[:, 2]).astype(dtype)


def shim_sample(shim, verts, faces, S, seed, iteration, mesh_index):
    """hm3_sample of tests/host_mesh3d_shim.cpp (shim = host_shim.mesh3d()) -> (points (S,3) float32, chosen faces (S,))"""
    import ctypes as C
    v, f = np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(faces, np.int32)
    pts, chosen = np.zeros((S, 3), np.float32), np.zeros(S, np.int32)
    rc_ = shim.hm3_sample(len(v), v.ctypes.data_as(C.c_void_p), len(f), f.ctypes.data_as(C.c_void_p), S, C.c_ulonglong(seed), iteration,
                          mesh_index, pts.ctypes.data_as(C.c_void_p), chosen.ctypes.data_as(C.c_void_p))
    if rc_ != 0:
        raise ValueError("hm3_sample refused the mesh")
    return pts, chosen


def sampler_uniforms(shim, S, seed, iteration, mesh_index):
    """the two uniforms of every sample as the kernel draws them: words 1 and 2 of Philox(counter (i, mesh, iteration, 0), key seed),
    their top 24 bits over 2^24 -> (u, v) float64 holding float32 values"""
    import ctypes as C
    u, v = np.zeros(S), np.zeros(S)
    key = (C.c_uint32 * 2)(seed & 0xFFFFFFFF, seed >> 32)
    for i in range(S):
        out = (C.c_uint32 * 4)()
        shim.hm3_philox((C.c_uint32 * 4)(i, mesh_index, iteration, 0), key, out)
        u[i], v[i] = (out[1] >> 8) / 16777216.0, (out[2] >> 8) / 16777216.0
    return u, v


def sampler_deviation(got, want64, extent):
    """max |got - want| over the extent of the mesh (its own size, not its distance from the origin)"""
    return float(np.abs(np.asarray(got, np.float64) - want64).max() / extent)


def bound(bar, yard):
    return max(bar, YARD * yard)


# ---------------------------------------------------------------------------------------------------------------
# C. coincidence and collapse
# ---------------------------------------------------------------------------------------------------------------
def coincident_problem():
    """the lattice ribbon with one target point exactly on every vertex (S = V, in another order)"""
    p = ribbon_problem(1, lattice=True)
    order = np.random.RandomState(3).permutation(p.V)
    return replace(p, name="coincident", points=p.verts[:, order].copy(), point_normals=None, point_boundary=None)


def self_target_problem():
    """the lattice ribbon against itself as the target mesh, its own vertices (reversed) as the points"""
    p = ribbon_problem(1, lattice=True)
    v = p.verts
    return replace(p, name="self_target", lbs=v.copy(), trans=np.zeros((1, 3), np.float32), deform=None, points=v[:, ::-1].copy(),
                   point_normals=None, point_boundary=None, targets=[(v[0].copy(), p.faces)])


# a strip of 8 vertices on the lattice (faces as mesh3d_forms.ribbon winds them), collapsed by deform_verts
STRIP = np.array([[0, 0, 0], [0, 1, 0.25], [1, 0, 0.5], [1, 1, 0], [2, 0, 0.25], [2, 1, 0.5], [3, 0, 0], [3, 1, 0.25]], np.float32)
STRIP_FACES = np.array([(i, i + 1, i + 2) if i % 2 == 0 else (i + 1, i, i + 2) for i in range(6)], np.int32)
COLLAPSES = {
    # vertex 3 moved onto vertex 2 (joined by an edge): a zero-length edge, two faces of zero area, a designed tie 2 < 3
    "coincident_vertices": {3: STRIP[2]},
    # vertex 3 moved to the middle of the edge (2, 4): face (3, 2, 4) is a segment
    "face_to_segment": {3: (STRIP[2] + STRIP[4]) / 2},
    # vertices 3 and 4 moved onto vertex 2: face (3, 2, 4) is a point
    "face_to_point": {3: STRIP[2], 4: STRIP[2]},
}


COLLAPSE_WEIGHTS = mf.HAND_WEIGHTS["collinear"]       # a clamped pair's gradient is ~1e8 |n| |e| per vertex: see mesh3d_forms


def collapsed_problem(name):
    """-> (problem, the collapsed vertices (lowest index first), a target point index equidistant from them by design)"""
    moved = COLLAPSES[name]
    deform = np.zeros((1, 8, 3), np.float32)
    for i, to in moved.items():
        deform[0, i] = np.asarray(to, np.float32) - STRIP[i]
    rs = np.random.RandomState(len(name))
    trans = np.array([[0.5, -0.25, 1.0]], np.float32)
    verts = STRIP[None] + trans[:, None] + deform
    pts = (verts[0, rs.randint(0, 8, 12)] + _snap(0.3 * rs.randn(12, 3), 1.0)).astype(np.float32)
    pts[0] = verts[0, 2] + np.array([0.125, -0.25, 0.125], np.float32)             # nearest the coincident vertices: a tie where they are
    return Problem(name, STRIP_FACES, STRIP[None].copy(), trans, deform, pts[None], None, None, None), sorted({2, *moved}), 0


def zero_ring_mesh():
    """mesh3d_forms' fan with its centre on the mean of its ring: unit 0 exactly"""
    return mf.HAND_MESHES["fan"]


# two faces on the edge (v0, v1) = ((0,0,0), (1,0,0)): coplanar and unfolded (1 - cos = 0), folded flat onto each other (2)
PAIR_FACES = np.array([[0, 1, 2], [1, 0, 3]], np.int32)
PAIR_MESHES = {"coplanar": (np.array([[0, 0, 0], [1, 0, 0], [0.25, 0.75, 0], [0.5, -0.5, 0]], np.float32), 0.0),
               "flat_fold": (np.array([[0, 0, 0], [1, 0, 0], [0.25, 0.75, 0], [0.5, 0.5, 0]], np.float32), 2.0)}
PAIR_EPS = 8 * EPS32
