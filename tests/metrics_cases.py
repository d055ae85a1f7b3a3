"""Inputs and expected values of the fit metrics (smalfit_fit_metrics: silhouette counts and PCK per frame), shared by
tests/test_metrics_cpu.py and tests/test_gpu_metrics.py.  Nothing here needs a GPU or calls rendering code of the project.

  refusals     every rule of smalfit_plan.h::metrics_args_refusal in its order, with the text include/smalfit.h's readers see
  scenes       a handful of faces whose covered pixel set follows from their construction: a pixel is covered when its centre
               lies strictly inside a projected triangle (2-D barycentrics in float64, tests/raster_anchors.py), and every
               centre keeps MARGIN_PX pixels from every edge, so that float32 cannot move one across
  pck inputs   targets placed at known multiples of threshold x sqrt(area) from the projections
"""
from __future__ import annotations

import numpy as np

from tests import raster_anchors as ra

# ---- refusals ----------------------------------------------------------------------------------------------------------
SIZE_TEXT = "smalfit_metrics_args.struct_size does not match this library (built against another smalfit.h?)"
FRAMES_TEXT = "num_frames exceeds the engine's max_frames"
REQUIRED_TEXT = "verts / sil_counts missing"
TARGET_TEXT = "target_sil missing (give target_sil or target_sil_u8)"
PARTIAL_TEXT = "give all of proj_joints, target_joints and target_visibility, or none of them"
OUTPUTS_TEXT = "keypoint_dist / pck_counts given without the keypoint inputs"
COUNT_TEXT = "num_thresholds must be 1..8"
VALUE_TEXT = "every threshold must be finite and > 0"
RULE_ORDER = (SIZE_TEXT, FRAMES_TEXT, REQUIRED_TEXT, TARGET_TEXT, PARTIAL_TEXT, OUTPUTS_TEXT, COUNT_TEXT, VALUE_TEXT)
NO_KEYPOINTS = dict(proj_joints=None, target_joints=None, target_visibility=None, keypoint_dist=None, pck_counts=None)
NAN, INF = float("nan"), float("inf")

# name -> (fields changed on a valid block of MAX frames with one threshold 0.15 and every pointer given; "thresholds": the
# leading values; the text, None: accepted)
MAX = 3
REFUSALS = {
    "valid": ({}, None),
    "struct_size": (dict(struct_size=8), SIZE_TEXT),
    "frames 0": (dict(num_frames=0), FRAMES_TEXT),
    "frames -1": (dict(num_frames=-1), FRAMES_TEXT),
    "frames max + 1": (dict(num_frames=MAX + 1), FRAMES_TEXT),
    "frames 1": (dict(num_frames=1), None),
    "verts": (dict(verts=None), REQUIRED_TEXT),
    "sil_counts": (dict(sil_counts=None), REQUIRED_TEXT),
    "no target": (dict(target_sil=None, target_sil_u8=None), TARGET_TEXT),
    "float target only": (dict(target_sil_u8=None), None),
    "byte target only": (dict(target_sil=None), None),
    "mask_out optional": (dict(mask_out=None), None),
    "partial: no proj": (dict(proj_joints=None), PARTIAL_TEXT),
    "partial: no target_joints": (dict(target_joints=None), PARTIAL_TEXT),
    "partial: no visibility": (dict(target_visibility=None), PARTIAL_TEXT),
    "partial: proj alone": (dict(target_joints=None, target_visibility=None, keypoint_dist=None, pck_counts=None), PARTIAL_TEXT),
    "dist without inputs": (dict(NO_KEYPOINTS, keypoint_dist=1), OUTPUTS_TEXT),
    "pck without inputs": (dict(NO_KEYPOINTS, pck_counts=1), OUTPUTS_TEXT),
    "silhouette only": (dict(NO_KEYPOINTS), None),
    "silhouette only ignores thresholds": (dict(NO_KEYPOINTS, num_thresholds=0, thresholds=(NAN,)), None),
    "keypoint outputs optional": (dict(keypoint_dist=None, pck_counts=None), None),
    "T 0": (dict(num_thresholds=0), COUNT_TEXT),
    "T 9": (dict(num_thresholds=9), COUNT_TEXT),
    "T -1": (dict(num_thresholds=-1), COUNT_TEXT),
    "T 1": (dict(num_thresholds=1, thresholds=(0.15,)), None),
    "T 8": (dict(num_thresholds=8, thresholds=(0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.4, 0.5)), None),
    "threshold nan": (dict(thresholds=(NAN,)), VALUE_TEXT),
    "threshold 0": (dict(thresholds=(0.0,)), VALUE_TEXT),
    "threshold negative": (dict(thresholds=(-0.1,)), VALUE_TEXT),
    "threshold inf": (dict(thresholds=(INF,)), VALUE_TEXT),
    "threshold smallest": (dict(thresholds=(1e-45,)), None),
    "last threshold nan": (dict(num_thresholds=3, thresholds=(0.1, 0.2, NAN)), VALUE_TEXT),
    "a value past T is not read": (dict(num_thresholds=2, thresholds=(0.1, 0.2, NAN)), None),
    # the first fault is the one reported
    "order: size before frames": (dict(struct_size=8, num_frames=0), SIZE_TEXT),
    "order: frames before verts": (dict(num_frames=0, verts=None), FRAMES_TEXT),
    "order: verts before target": (dict(verts=None, target_sil=None, target_sil_u8=None), REQUIRED_TEXT),
    "order: target before partial": (dict(target_sil=None, target_sil_u8=None, proj_joints=None), TARGET_TEXT),
    "order: partial before T": (dict(proj_joints=None, num_thresholds=0), PARTIAL_TEXT),
    "order: T before value": (dict(num_thresholds=9, thresholds=(NAN,)), COUNT_TEXT),
}
POINTERS = ("verts", "target_sil", "target_sil_u8", "sil_counts", "mask_out", "proj_joints", "target_joints", "target_visibility",
            "keypoint_dist", "pck_counts")


def block(fields, pointers, num_frames=MAX):
    """smalify_amd._lib.MetricsArgs: the valid block with `fields` changed.  pointers: name -> address (int); a field value of 1
    stands for "given" and takes the name's address"""
    from smalify_amd import _lib
    a = _lib.MetricsArgs()
    a.num_frames, a.num_thresholds = num_frames, 1
    a.thresholds[0] = 0.15
    for k in POINTERS:
        setattr(a, k, pointers[k])
    for k, v in fields.items():
        if k == "thresholds":
            for i, t in enumerate(v):
                a.thresholds[i] = t
        elif k in POINTERS:
            setattr(a, k, pointers[k] if v == 1 else v)
        else:
            setattr(a, k, v)
    return a


# ---- closed-form coverage ------------------------------------------------------------------------------------------------
MARGIN_PX = 1e-3
SIZES = (16, 50, 51)


def ndc(col, row, S):
    """continuous pixel coordinates (pixel (r, c) has its centre at (c, r)) -> NDC, the map of ra.pixel_centre"""
    return 1.0 - (2.0 * col + 1.0) / S, 1.0 - (2.0 * row + 1.0) / S


def _world(tri_px, S, z_view=2.0):
    return np.stack([ra.world_from_ndc(*ndc(c, r, S), z_view) for c, r in tri_px])


def inside(tri_px, S):
    """-> ((S,S) bool: pixel centre strictly inside the triangle, the smallest distance in pixels of a centre to an edge line
    among the pixels of the triangle's box grown by two)"""
    cols, rows = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64))
    (ax, ay), (bx, by), (cx, cy) = [(float(c), float(r)) for c, r in tri_px]
    den = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
    w1 = ((cols - ax) * (cy - ay) - (rows - ay) * (cx - ax)) / den
    w2 = ((bx - ax) * (rows - ay) - (by - ay) * (cols - ax)) / den
    w0 = 1.0 - w1 - w2
    pts = np.array([(ax, ay), (bx, by), (cx, cy)])
    dist = np.full((S, S), np.inf)
    for i, j in ((0, 1), (1, 2), (2, 0)):
        e = pts[j] - pts[i]
        dist = np.minimum(dist, np.abs((cols - pts[i][0]) * e[1] - (rows - pts[i][1]) * e[0]) / np.hypot(*e))
    near = (cols >= pts[:, 0].min() - 2) & (cols <= pts[:, 0].max() + 2) & (rows >= pts[:, 1].min() - 2) & (rows <= pts[:, 1].max() + 2)
    return (w0 > 0) & (w1 > 0) & (w2 > 0), float(dist[near].min()) if near.any() else np.inf


def scene(name, S):
    """-> dict(verts (V,3) float64 world, faces (F,3), mask (S,S) bool expected coverage, margin: pixels, target (S,S) bool)
    Triangles are given in continuous pixel coordinates as fractions of S with irrational-looking offsets."""
    f = float(S)
    tris, extra_verts, extra_faces, z = [], [], [], []
    if name == "single":
        tris = [[(0.153 * f, 0.091 * f), (0.791 * f, 0.207 * f), (0.322 * f, 0.863 * f)]]
    elif name == "overlap":                      # two triangles sharing a region: a pixel of both is counted once
        tris = [[(0.153 * f, 0.091 * f), (0.791 * f, 0.207 * f), (0.322 * f, 0.863 * f)],
                [(0.413 * f, 0.133 * f), (0.907 * f, 0.611 * f), (0.208 * f, 0.574 * f)]]
        z = [2.0, 1.6]
    elif name == "clipped":                      # one triangle through each border, one over a corner
        tris = [[(-0.413 * f, 0.307 * f), (0.193 * f, 0.213 * f), (0.121 * f, 0.489 * f)],      # left
                [(0.823 * f, 0.517 * f), (1.391 * f, 0.603 * f), (0.877 * f, 0.791 * f)],       # right
                [(0.438 * f, -0.377 * f), (0.619 * f, 0.172 * f), (0.341 * f, 0.143 * f)],      # top
                [(0.451 * f, 0.853 * f), (0.687 * f, 0.871 * f), (0.533 * f, 1.443 * f)],       # bottom
                [(0.771 * f, -0.213 * f), (1.313 * f, 0.187 * f), (0.853 * f, 0.233 * f)]]      # top right corner
    elif name == "nothing":                      # entirely off screen | degenerate | behind the camera
        tris = []
    else:
        raise KeyError(name)
    verts, faces = [], []
    mask, margin = np.zeros((S, S), bool), np.inf
    for k, t in enumerate(tris):
        verts.append(_world(t, S, z[k] if z else 2.0))
        faces.append([3 * k, 3 * k + 1, 3 * k + 2])
        m, d = inside(t, S)
        mask |= m
        margin = min(margin, d)
    if name == "nothing":
        off = _world([(1.2 * f, 0.3 * f), (1.7 * f, 0.4 * f), (1.4 * f, 0.8 * f)], S)             # every x_ndc below -1
        p, q = _world([(0.3 * f, 0.3 * f), (0.7 * f, 0.6 * f)], S)
        degenerate = np.stack([p, q, q])                                                        # two corners coincide: area exactly 0
        behind = _world([(0.2 * f, 0.2 * f), (0.8 * f, 0.3 * f), (0.4 * f, 0.8 * f)], S, z_view=-1.0)     # world z = 3.7, past the camera
        verts, faces = [off, degenerate, behind], [[0, 1, 2], [3, 4, 5], [6, 7, 8]]
    target = np.zeros((S, S), bool)
    target[int(0.3 * S):int(0.7 * S) + 1, int(0.1 * S):int(0.55 * S)] = True                    # a hand-placed rectangle
    return dict(verts=np.concatenate(verts), faces=np.asarray(faces, np.int32), mask=mask, margin=margin, target=target)


SCENES = ("single", "overlap", "clipped", "nothing")


def counts(mask, target):
    """(..., S, S) bool x 2 -> (..., 4) int64: intersection, union, rendered, target"""
    m, t = np.asarray(mask, bool), np.asarray(target, bool)
    return np.stack([(m & t).sum((-2, -1)), (m | t).sum((-2, -1)), m.sum((-2, -1)), t.sum((-2, -1))], -1).astype(np.int64)


# ---- target binarisation -------------------------------------------------------------------------------------------------
FLOAT_VALUES = np.array([0.5, np.nextafter(np.float32(0.5), np.float32(1.0)), 0.0, 1.0], np.float32)
BYTE_VALUES = np.array([127, 128, 0, 255], np.uint8)


def pattern(M, S, seed=11):
    """(M,S,S) indices 0..3 into the value tables: a fixed draw, every frame another arrangement"""
    return np.random.RandomState(seed).randint(0, 4, (M, S, S)).astype(np.int64)


# ---- PCK -----------------------------------------------------------------------------------------------------------------
THRESHOLDS = {1: (0.15,), 3: (0.05, 0.15, 0.37), 8: (0.05, 0.08, 0.11, 0.15, 0.21, 0.26, 0.37, 0.5)}
RATIOS = (0.0, 0.5, 0.999, 1.001, 2.0)
PCK_CLEARANCE = 1e-3 - 1e-5       # 0.999 / 1.001 sit at 1e-3 by construction; float32 rounding of the targets moves them by ~1e-7


def pck_inputs(M, S, areas, thresholds, seed=5):
    """-> proj, target (M,25,2) float32.  Keypoint k of frame n sits RATIOS[...] x thresholds[...] x sqrt(area_n) from its
    projection along a fixed unit vector; frames of area 0 get a displacement of a few pixels."""
    rs = np.random.RandomState(seed)
    proj = (5.0 + (S - 10.0) * rs.rand(M, 25, 2)).astype(np.float32)
    ang = 0.7 + 2.399963 * np.arange(25)                                   # fixed directions
    u = np.stack([np.cos(ang), np.sin(ang)], -1)
    T = len(thresholds)
    target = np.zeros((M, 25, 2), np.float64)
    for n in range(M):
        for k in range(25):
            thr = thresholds[(k + n) % T]
            r = RATIOS[((k + n) // T + k) % len(RATIOS)]
            scale = np.sqrt(areas[n]) if areas[n] > 0 else 20.0
            target[n, k] = proj[n, k].astype(np.float64) + r * thr * scale * u[k]
    return proj, target.astype(np.float32)


def pck_expected(proj, target, vis, areas, thresholds):
    """float64 on the float32 inputs -> (dist (M,25), counts (M,1+T), the smallest |dist / threshold - 1| over keypoints of
    frames with a target)"""
    d = np.hypot(*np.moveaxis(proj.astype(np.float64) - target.astype(np.float64), -1, 0))
    areas = np.asarray(areas, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        dist = np.where(areas[:, None] > 0, d / np.sqrt(np.float32(areas).astype(np.float64))[:, None], np.inf)
    thr = np.array([np.float32(t) for t in thresholds], np.float64)
    v = np.asarray(vis) > 0
    ok = v[:, :, None] & (dist[:, :, None] <= thr)
    rows = np.concatenate([v.sum(1)[:, None], ok.sum(1)], 1).astype(np.int64)
    finite = dist[areas > 0]
    clearance = float(np.abs(finite[:, :, None] / thr - 1.0).min()) if finite.size else np.inf
    return dist, rows, clearance


def visibility(M, kind, seed=9):
    if kind == "all":
        return np.ones((M, 25), np.float32)
    if kind == "none":
        return np.zeros((M, 25), np.float32)
    v = (np.random.RandomState(seed).rand(M, 25) < 0.6).astype(np.float32)
    v[:, 0], v[:, 1] = 1.0, 0.0
    return v * np.array([1.0, 0.5, 2.0, 1.0, 1.0] * 5, np.float32)            # visible means > 0, not == 1
