"""The reference's SMAL template mesh (tests/golden/smal_template_mesh.npz: 3889 vertices, 7774 faces, face areas spread over a
factor of 4750) as a rasteriser and 3-D workload: the views, the rigid model that carries it, and -- per view -- the pixels whose
value float32 cannot decide.  Shared by tests/test_template_cases_cpu.py (which proves the regimes each view reaches and that the
rule below is enough: the float32 ORACLE agrees with the float64 one on what it keeps) and tests/test_gpu_template_mesh.py (the
HIP kernels against the float64 oracle).  Nothing here needs a GPU or reads anything outside the repository.

A view is (name, S, base rotation, added rotation vector, tz, scale); the world vertices are
    to_f32(scale * (v - v.mean(0)) @ R(rv).T + (0.03, -0.02, tz)).

The ambiguity rule, computed from the float64 twin (tests/raster_forms.py: pairs) alone.  The oracle and the kernels interpolate a
face's depth with barycentrics over (area + 1e-8), which scales it by area / (area + 1e-8): for this mesh's smallest faces that
is a per-cent of the depth, far more than the gap between neighbouring faces, so the twin's depth is scaled the same way before
anything is ranked (oracle_depth).

  silhouette  a pixel is left out when
    blur      a face of its box has its nearest edge within BLUR_MARGIN (NDC) of the blur radius: the face enters or leaves the
              candidates with p = 1e-4, and moves the K-cut when there are more than K
    cull      a face within a factor of 2 of the cull threshold |area| = 1e-8 is (or would be, if it lived) a candidate there
    edge      a candidate among the K nearest, on a pixel that is not saturated (1 - sil above TIE_WEIGHT), has an edge whose
              squared length is within a factor of 2 of 1e-8, where the oracle and the kernels switch from the distance to the
              segment to the distance to its end point
    cut       it has more than K candidates and a candidate among the K nearest and one beyond them have depths closer than the
              sum of their float32 uncertainties.  The uncertainty of a depth (Analysis.pair_zerr) is the larger of DEPTH_ULPS
              float32 epsilons of the products behind the three barycentrics times the corners' depths -- the barycentrics of a
              sliver face reach hundreds at a pixel a blur radius away, and the three terms cancel -- and JITTER_SAFETY x what
              the depth moves by when every NDC coordinate moves by two float32 epsilons: a face seen edge-on has a depth plane
              so steep that the rounding of its corners turns it
    sign      a face that reaches the pixel (inside, or within the blur radius) has a depth within that uncertainty of 0: the
              `pz >= 0` test decides whether it is a candidate at all.  This is what decides the one pixel of native_far-128 on
              which the two oracles are 1.2e-3 apart: a face of area -2.7e-8 seen edge-on, depth -0.016 in float64 and +0.001 in
              float32 a blur radius from it
  gradient    additionally when
    tie       a candidate among the K nearest whose weight in the gradient, (1 - sil) p, is above TIE_WEIGHT has two edges nearer
              than TIE_MARGIN (NDC) to equally near, with different nearest points: which edge takes the gradient is a coin toss
  hard mask   (fit_metrics) a centre within EDGE_MARGIN (NDC) of an edge of a live face, or inside a face near the cull threshold

A pixel centre near an EDGE does not make the silhouette or its gradient ambiguous: the signed squared distance and its
derivative are continuous through 0 there.
"""
from __future__ import annotations

import functools
import math
import os

import numpy as np

from tests import raster_anchors as ra
from tests import raster_forms as rf

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "smal_template_mesh.npz")
V, F = 3889, 7774
K = rf.K
K_EPS = 1e-8
EPS32 = float(np.finfo(np.float32).eps)
OFFSET = (0.03, -0.02)
TILT = (0.3, -0.4, 0.2)

# (name, S, base, added rotation vector, tz, scale)
VIEWS = (("init_far", 64, "init", None, 0.0, 1.0),
         ("native_far", 64, "native", None, 0.0, 1.0),
         ("init_tilt", 64, "init", TILT, 0.6, 1.0),
         ("native_far", 128, "native", None, 0.0, 1.0),
         ("init_near", 128, "init", None, 1.3, 1.0),
         ("init_far", 256, "init", None, 0.0, 1.0),
         ("init_near", 256, "init", None, 1.3, 1.0),
         ("init_tiny", 64, "init", None, -3.0, 1.0))
VIEW_IDS = tuple("%s-%d" % (v[0], v[1]) for v in VIEWS)
# the views held to the tight comparison; init_tiny (the whole animal on 70 pixels, 50 of them past the K cut) keeps the loose one
LOOSE_ONLY = ("init_tiny-64",)
TIGHT_IDS = tuple(v for v in VIEW_IDS if v not in LOOSE_ONLY)

# ---- the rule's constants: float32 places an NDC coordinate of size ~1 to 6e-8 and a nearest-edge distance to a few of those
BLUR_MARGIN = 2e-6          # NDC: ~30 float32 epsilons of a coordinate
TIE_MARGIN = 2e-6           # NDC, between the distances to two edges
EDGE_MARGIN = 2e-6          # NDC, hard coverage only
DEPTH_ULPS = 4.0            # depth_error: DEPTH_ULPS float32 epsilons of the products behind the three barycentrics, or
JITTER_TRIALS = 8           # JITTER_SAFETY x what moving every NDC coordinate by two float32 epsilons (random signs, so many
JITTER_SAFETY = 2.0         # trials) moves the depth by, whichever is larger
TIE_WEIGHT = 1e-7           # (1 - sil) p below which a candidate's nearest edge cannot matter to 1e-4 of the gradient
SIL_CAP, GRAD_CAP = 0.15, 0.35          # largest share of the covered pixels the rule may leave out
SIL_BAR, GRAD_BAR = 1e-5, 1e-4          # float32 oracle against float64 oracle on what it keeps


def view(view_id):
    return VIEWS[VIEW_IDS.index(view_id)]


@functools.lru_cache(maxsize=None)
def template():
    """(verts (3889,3) float32, faces (7774,3) int64) of the fixture"""
    d = np.load(GOLDEN)
    verts, faces = d["verts"], d["faces"].astype(np.int64)
    assert verts.dtype == np.float32 and verts.shape == (V, 3) and faces.shape == (F, 3)
    return verts, faces


def rotation_vector(view_id):
    from smalify_amd import model_io
    _, _, base, add, _, _ = view(view_id)
    rv = np.asarray(model_io.initial_global_rotation(), np.float64).reshape(3) if base == "init" else np.zeros(3)
    return rv + (np.zeros(3) if add is None else np.asarray(add, np.float64))


def rotation(rv):
    import torch
    from oracle import smal_oracle as so
    return so.rodrigues(torch.from_numpy(np.asarray(rv, np.float64).reshape(1, 3)))[0].numpy()


@functools.lru_cache(maxsize=None)
def world(view_id):
    """(3889,3) float64 holding float32 values: the scene as both sides see it"""
    _, _, _, _, tz, scale = view(view_id)
    v = template()[0].astype(np.float64)
    return rf.to_f32(scale * (v - v.mean(0)) @ rotation(rotation_vector(view_id)).T + np.array([OFFSET[0], OFFSET[1], tz]))


def size(view_id):
    return view(view_id)[1]


# ---- the model ---------------------------------------------------------------------------------------------------------------
def centred_template():
    v = template()[0].astype(np.float64)
    return (v - v.mean(0)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def model_data():
    """tests/test_gpu_raster_forms._model_data with the (centred) template as v_template and as the first shape direction:
    arbitrary topology over V_PAD slots, rigid skinning on the root, betas[0] scales the mesh by 1 + betas[0].  The unused slots
    (the root joint among them) stay where _pad_np puts them whatever betas[0] is."""
    from tests import test_gpu_raster_forms as grf
    t = grf._pad_np(centred_template())
    sd = np.zeros((grf.V_PAD, 3), np.float64)
    sd[grf.SLOTS[:V]] = centred_template()
    return grf._model_data(template()[1], t, sd.reshape(-1))


def pose_of(view_id):
    """(global_rotation (3,), trans (3,)) float32 with which model_data() at betas = 0 renders (nearly) world(view_id): the model
    turns about its root joint, the slot every unused vertex shares"""
    from tests import test_gpu_raster_forms as grf
    _, _, _, _, tz, scale = view(view_id)
    assert scale == 1.0
    rv = rotation_vector(view_id)
    R = rotation(rv.astype(np.float32).astype(np.float64))
    pivot = grf._pad_np(np.zeros((0, 3), np.float32))[0].astype(np.float64)
    t = np.array([OFFSET[0], OFFSET[1], tz]) - (pivot - R @ pivot)
    return rv.astype(np.float32), t.astype(np.float32)


@functools.lru_cache(maxsize=None)
def engine_face_order():
    """(7774,) the engine's face order (Morton order, smal_model_pack.h) as indices into the fixture's faces"""
    from tests import host_plan
    from tests import test_gpu_raster_forms as grf
    _, tables, _, _ = host_plan.load().pack_model(model_data())
    packed = np.frombuffer(tables["faces_int"], np.int32).reshape(-1, 3)[:F]
    slot_to_vertex = {int(s): i for i, s in enumerate(grf.SLOTS[:V])}
    index = {tuple(int(x) for x in f): i for i, f in enumerate(template()[1])}
    order = np.array([index[tuple(slot_to_vertex[int(s)] for s in row)] for row in packed], np.int64)
    assert sorted(order.tolist()) == list(range(F))
    return order


# ---- the float64 twin of one view ----------------------------------------------------------------------------------------------
def face_areas(verts, faces):
    x, y, _ = rf.project(verts)
    fx, fy = x[faces], y[faces]
    return (fx[:, 2] - fx[:, 0]) * (fy[:, 1] - fy[:, 0]) - (fy[:, 2] - fy[:, 0]) * (fx[:, 1] - fx[:, 0])


def oracle_depth(x, y, z, f, px, py):
    """the interpolated depth of faces f (n,3) at the points (px, py), as oracle.smal_oracle.soft_silhouette and make_face_rec
    form it: three barycentrics, each over (area + 1e-8), times the corners' depths; and sum_i (|product| + |product|) |z_i| / |area
    + 1e-8| over the two products of each edge function: what one float32 rounding of every product is worth"""
    ax, ay, bx, by, cx, cy = x[f[:, 0]], y[f[:, 0]], x[f[:, 1]], y[f[:, 1]], x[f[:, 2]], y[f[:, 2]]
    den = (cx - ax) * (by - ay) - (cy - ay) * (bx - ax) + K_EPS
    den = np.where(den == 0.0, 1.0, den)
    terms = (((px - bx) * (cy - by), (py - by) * (cx - bx), z[f[:, 0]]), ((px - cx) * (ay - cy), (py - cy) * (ax - cx), z[f[:, 1]]),
             ((px - ax) * (by - ay), (py - ay) * (bx - ax), z[f[:, 2]]))
    pz = sum((p - q) / den * zz for p, q, zz in terms)
    return pz, sum((np.abs(p) + np.abs(q)) * np.abs(zz) for p, q, zz in terms) / np.abs(den)


def _as_live(verts, faces, ids, S):
    """the pixels the culled faces `ids` would reach if they lived (a handful of tiny faces, pixel by pixel): -> [(face, pix)]"""
    x, y, z = rf.project(verts)
    out = []
    for f in ids:
        i = faces[f]
        tri = [(x[j], y[j]) for j in i]
        xs, ys = [p[0] for p in tri], [p[1] for p in tri]
        c0 = max(int(math.ceil((1.0 - (max(xs) + rf.R_BLUR)) * S / 2.0 - 0.5)), 0)
        c1 = min(int(math.floor((1.0 - (min(xs) - rf.R_BLUR)) * S / 2.0 - 0.5)), S - 1)
        r0 = max(int(math.ceil((1.0 - (max(ys) + rf.R_BLUR)) * S / 2.0 - 0.5)), 0)
        r1 = min(int(math.floor((1.0 - (min(ys) - rf.R_BLUR)) * S / 2.0 - 0.5)), S - 1)
        if max(z[j] for j in i) < 0:
            continue
        for r in range(r0, r1 + 1):
            for c in range(c0, c1 + 1):
                p = ra.pixel_centre(r, c, S)
                d = math.sqrt(ra.tri_dist2(p, tri))
                # the face is degenerate: its own inside test is meaningless, its reach is the blur radius (plus the margin)
                if d < rf.R_BLUR + BLUR_MARGIN:
                    out.append((int(f), r * S + c))
    return out


class Analysis:
    """what the float64 twin says about one view.  Per candidate (sorted by pixel, then oracle depth): pix, face, z, rank,
    p (its probability), zerr; per pixel (S*S,): count, covered, logalpha (over the K nearest), and the masks of the rule."""

    def __init__(self, view_id):
        self.view_id, self.S = view_id, size(view_id)
        S = self.S
        verts, faces = world(view_id), template()[1]
        self.verts, self.faces = verts, faces
        x, y, z = rf.project(verts)
        area = face_areas(verts, faces)
        self.area = area
        self.culled = np.abs(area) <= K_EPS
        self.near_cull = (np.abs(area) > 0.5 * K_EPS) & (np.abs(area) <= 2.0 * K_EPS)
        P = rf.pairs(verts, faces, S)
        self.P = P
        fid = P["face"]
        # the depth as the oracle and the kernels interpolate it, and its float32 uncertainty
        px, py = 1.0 - (2.0 * (P["pix"] % S) + 1.0) / S, 1.0 - (2.0 * (P["pix"] // S) + 1.0) / S
        f = faces[fid]
        self.pair_z, products = oracle_depth(x, y, z, f, px, py)
        self.pair_zerr = DEPTH_ULPS * EPS32 * products
        rs = np.random.RandomState(5)
        for _ in range(JITTER_TRIALS):
            sx, sy, sz = (np.where(rs.rand(V) < 0.5, -1.0, 1.0) for _ in range(3))
            zj, _ = oracle_depth(x * (1.0 + 2.0 * EPS32 * sx), y * (1.0 + 2.0 * EPS32 * sy), z * (1.0 + EPS32 * sz), f, px, py)
            self.pair_zerr = np.maximum(self.pair_zerr, JITTER_SAFETY * np.abs(zj - self.pair_z))
        # edges at the degenerate-edge switch
        e2 = np.stack([(x[faces[:, i]] - x[faces[:, j]]) ** 2 + (y[faces[:, i]] - y[faces[:, j]]) ** 2 for i, j in ((0, 1), (0, 2), (1, 2))], 1)
        self.edge_switch = np.any((e2 > 0.5 * K_EPS) & (e2 <= 2.0 * K_EPS), 1)
        self.short_edge = np.any(e2 <= K_EPS, 1)
        # candidates, by pixel and depth
        c = np.nonzero(P["cand"])[0]
        order = c[np.lexsort((self.pair_z[c], P["pix"][c]))]
        self.pair = order
        self.pix, self.face, self.z, self.zerr = P["pix"][order], fid[order], self.pair_z[order], self.pair_zerr[order]
        d = np.where(P["inside"][order], -1.0, 1.0) * P["dist"][order] ** 2
        self.log1mp = -np.logaddexp(0.0, -d / ra.SIGMA)                       # log(1 - p) = log sigmoid(d / sigma)
        self.p = 1.0 / (1.0 + np.exp(np.clip(d / ra.SIGMA, -700, 700)))
        first = np.ones(len(order), bool)
        first[1:] = self.pix[1:] != self.pix[:-1]
        start = np.maximum.accumulate(np.where(first, np.arange(len(order)), 0))
        self.rank = np.arange(len(order)) - start
        npx = S * S
        self.count = np.bincount(self.pix, minlength=npx)
        self.covered = self.count > 0
        near = self.rank < K
        self.logalpha = np.bincount(self.pix[near], weights=self.log1mp[near], minlength=npx)
        self.sil = -np.expm1(self.logalpha)
        self._rule()

    def _flag(self, pixels):
        m = np.zeros(self.S * self.S, bool)
        m[np.asarray(pixels, np.int64)] = True
        return m

    def _rule(self):
        P, S = self.P, self.S
        to_ndc = 2.0 / S
        live_pair = ~self.culled[P["face"]]
        self.blur = self._flag(P["pix"][live_pair & (P["blur_margin"] * to_ndc < BLUR_MARGIN)])
        as_live = _as_live(self.verts, self.faces, np.nonzero(self.near_cull & self.culled)[0], S)
        near_live = self.near_cull[self.face]
        self.cull = self._flag([p for _, p in as_live]) | self._flag(self.pix[near_live])
        self.cull_inside = self._flag(P["pix"][self.near_cull[P["face"]] & P["inside"]]) | self._flag([p for _, p in as_live])
        alpha = np.exp(self.logalpha)[self.pix]
        self.edge = self._flag(self.pix[self.edge_switch[self.face] & (self.rank < K) & (alpha > TIE_WEIGHT)])
        # the K cut: the largest z + zerr among the K nearest against the smallest z - zerr beyond them
        npx = S * S
        hi_in = np.full(npx, -np.inf)
        lo_out = np.full(npx, np.inf)
        near = self.rank < K
        np.maximum.at(hi_in, self.pix[near], (self.z + self.zerr)[near])
        np.minimum.at(lo_out, self.pix[~near], (self.z - self.zerr)[~near])
        self.cut = (self.count > K) & (hi_in >= lo_out)
        reach = live_pair & (P["inside"] | (P["dist"] ** 2 < ra.BLUR))
        self.sign = self._flag(P["pix"][reach & (np.abs(self.pair_z) <= self.pair_zerr)])
        self.sil_excluded = self.blur | self.cull | self.edge | self.cut | self.sign
        weight = np.exp(self.logalpha)[self.pix] * self.p
        tie = near & (weight > TIE_WEIGHT) & (P["tie_margin"][self.pair] * to_ndc < TIE_MARGIN)
        self.tie = self._flag(self.pix[tie])
        self.grad_excluded = self.sil_excluded | self.tie
        self.mask = self._flag(P["pix"][P["cand"] & P["inside"]])
        self.mask_excluded = self._flag(P["pix"][live_pair & (P["edge_margin"] * to_ndc < EDGE_MARGIN)]) | self.cull_inside

    # ---- shares and regimes
    def shares(self):
        n = max(int(self.covered.sum()), 1)
        return float((self.sil_excluded & self.covered).sum()) / n, float((self.grad_excluded & self.covered).sum()) / n

    def image(self, flat):
        return flat.reshape(self.S, self.S)

    def never_near(self):
        """vertex ids used only by faces that are among no pixel's K nearest"""
        used = np.unique(self.faces[np.unique(self.face[self.rank < K])])
        return np.setdiff1d(np.arange(V), used)

    def vertices_of_pixels(self, pixel_mask):
        """vertex ids of the faces among the K nearest of the flagged pixels"""
        sel = (self.rank < K) & pixel_mask[self.pix]
        return np.unique(self.faces[np.unique(self.face[sel])])

    def formats(self):
        """per face in the ENGINE's order: the hand-off format of its wave of four (rf.wave_formats)"""
        boxes, _ = rf.face_boxes(self.verts, self.faces, self.S)
        cnt, _ = rf.per_face(self.P, F)
        order = engine_face_order()
        return rf.wave_formats(rf.box_pixels(boxes)[order].tolist(), cnt[order].tolist())


@functools.lru_cache(maxsize=None)
def analysis(view_id):
    return Analysis(view_id)


# ---- the two oracles -------------------------------------------------------------------------------------------------------
def upstream(view_id):
    """(S,S) float32 upstream gradient of the silhouette"""
    S = size(view_id)
    return np.random.RandomState(VIEW_IDS.index(view_id) + 7).randn(S, S).astype(np.float32)


_ORACLE = {}


def oracle(view_id, dtype="float64", keep=None):
    """(sil (S,S), d/d verts (3889,3)) of oracle.smal_oracle.soft_silhouette in `dtype`, as float64 arrays; the upstream
    weights are upstream(view_id), zeroed outside `keep` ((S,S) bool) when given.  Computed once per argument set."""
    import torch
    from oracle import smal_oracle as so
    key = (view_id, dtype, None if keep is None else keep.tobytes())
    if key not in _ORACLE:
        S = size(view_id)
        w = upstream(view_id).astype(np.float64) * (1.0 if keep is None else keep.reshape(S, S))
        dt = torch.float64 if dtype == "float64" else torch.float32
        v = torch.from_numpy(world(view_id)).to(dt)[None].requires_grad_(True)
        sil = so.soft_silhouette(v, template()[1], S)
        (sil * torch.from_numpy(w).to(dt)).sum().backward()
        _ORACLE[key] = (sil[0].detach().double().numpy(), v.grad[0].double().numpy())
    return _ORACLE[key]


def rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def worst_row(a, b):
    """the largest single-vertex deviation relative to the largest row of b"""
    return float(np.linalg.norm(a - b, axis=1).max() / max(np.linalg.norm(b, axis=1).max(), 1e-30))


# ---- the template as a 3-D target mesh -------------------------------------------------------------------------------------
def normalised(verts):
    """centred and scaled as the 3-D fitter does with its targets: minus the mean, over the largest coordinate magnitude"""
    v = np.asarray(verts, np.float64)
    v = v - v.mean(0)
    return (v / np.abs(v).max()).astype(np.float32)


@functools.lru_cache(maxsize=None)
def target_mesh():
    """(verts (3889,3) float32, faces (7774,3) int32): the one target mesh"""
    return normalised(template()[0]), template()[1].astype(np.int32)


@functools.lru_cache(maxsize=None)
def bent_template():
    """a fitted mesh of the template's own topology that is not a fit: the target shrunk by 2 % and bent by a smooth field of
    2 % of its size, so that every distance is some 1e-2 and the nearest triangle is rarely the vertex's own"""
    v = target_mesh()[0].astype(np.float64)
    rs = np.random.RandomState(19)
    u = np.sin(v @ rs.uniform(-3, 3, (3, 3)).T + rs.uniform(0, 2 * np.pi, 3))
    return (0.98 * v + 0.02 * u).astype(np.float32)


def small_fit(count=256, seed=3, sigma=0.01):
    """(verts (count,3) float32, faces) a strip of `count` vertices scattered within ~sigma of the target's surface"""
    from tests import mesh_score_cases as msc
    tv, tf = target_mesh()
    return msc.points_near(tv, tf, count, seed, sigma=sigma), msc.ribbon(count, seed)[1]


def sampler_intervals(verts, faces):
    """(thr (F,) the sampler's cumulative-area thresholds, share (F,) the part of the 2^32 draws that picks each face): the
    rule of mesh3d_topology.h::area_thresholds and mesh3d_math.h::sample_face, restated in float64"""
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64)
    area = 0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)
    cum = np.cumsum(area)
    last = int(np.nonzero(area > 0)[0].max())
    x = np.floor(cum / cum[-1] * 4294967296.0)
    thr = np.where((np.arange(len(f)) >= last) | (x >= 4294967295.0), 4294967295.0, x)
    edges = np.concatenate([[0.0], thr[:-1], [4294967296.0]])
    return thr, np.diff(edges) / 4294967296.0, area
