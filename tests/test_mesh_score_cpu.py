"""CPU: the parts of smalfit_mesh_score that need no GPU.

  maths     smalify_amd/csrc/mesh3d_math.h::point_triangle_dist2 through tests/host_mesh_score_shim.cpp: closed forms on the
            unit triangle in all seven regions, exact zeros, degenerate triangles, and the accuracy over 2 M near-surface
            pairs against float64 on the same float32 inputs.  tests/golden/hip_mesh_score_measured.json records the shim's
            worst deviation in ulp(L); the bar is twice that and never above 64 ulp(L) -- the condition that keeps a
            region-walk implementation out
  rules     every rule of smalfit_plan.h::mesh_score_args_refusal with its text and its place in the order, the accepted
            edge of each, the struct's size and offsets against gcc's
  summary   smalify_amd/metrics.py::summarise_mesh_score by hand on two meshes
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from smalify_amd import _lib, metrics
from tests import host_mesh_score as hms
from tests import mesh_score_cases as mc

MEASURED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hip_mesh_score_measured.json")


@pytest.fixture(scope="module")
def shim():
    return hms.load()


def recorded():
    assert os.path.exists(MEASURED), "tests/golden/hip_mesh_score_measured.json is missing"
    return json.load(open(MEASURED))


# ---- closed forms -------------------------------------------------------------------------------------------------
def test_unit_triangle_regions(shim):
    a, b, c = mc.UNIT_TRIANGLE
    for region, (x, y), flat in mc.UNIT_REGIONS:
        for h in mc.UNIT_HEIGHTS:
            want = np.hypot(flat, h)
            got = hms.point_triangle_dist(shim, [[x, y, h]], [a], [b], [c])[0]
            assert abs(float(got) - want) <= 2.0 ** -22, (region, h, got, want)       # coordinates <= 2.5: two ulp(L)
            # the float64 reference is the same definition
            assert abs(float(mc.point_triangle_dist([x, y, h], a, b, c)) - want) < 1e-15, (region, h)
    # every cyclic order and both orientations of the corners give the same regions
    for order in ((1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2)):
        t = mc.UNIT_TRIANGLE[list(order)]
        for region, (x, y), flat in mc.UNIT_REGIONS:
            got = hms.point_triangle_dist(shim, [[x, y, -0.5]], [t[0]], [t[1]], [t[2]])[0]
            assert abs(float(got) - np.hypot(flat, 0.5)) <= 2.0 ** -22, (order, region)


def test_exact_zeros(shim):
    a, b, c = mc.UNIT_TRIANGLE
    q = np.array(mc.UNIT_ZEROS, np.float32)
    n = len(q)
    got = hms.point_triangle_dist(shim, q, np.tile(a, (n, 1)), np.tile(b, (n, 1)), np.tile(c, (n, 1)))
    assert (got == 0.0).all(), got
    # a corner of ANY triangle is at distance exactly 0 (it starts one of the three segments: parameter 0, residual 0)
    p, ta, tb, tc = mc.near_surface_pairs(5000, seed=3)
    for corner in (ta, tb, tc):
        assert (hms.point_triangle_dist(shim, corner, ta, tb, tc) == 0.0).all()


def test_degenerate_triangles_are_their_segments(shim):
    q = np.array(mc.DEGENERATE_QUERIES, np.float32)
    for name, corners, (s0, s1) in mc.DEGENERATE:
        t = np.array(corners, np.float32)
        got = hms.point_triangle_dist(shim, q, *(np.tile(t[i], (len(q), 1)) for i in range(3)))
        want = mc.segment_dist(q, s0, s1)
        assert np.isfinite(got).all(), name
        assert np.abs(got.astype(np.float64) - want).max() <= 2.0 ** -22 * 3.0, (name, got, want)
        assert np.abs(mc.point_triangle_dist(q, t[0], t[1], t[2]) - want).max() < 1e-15, name


# ---- accuracy -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def accuracy_pairs():
    p, a, b, c = mc.accuracy_pairs()
    return (p, a, b, c), mc.point_triangle_dist(p, a, b, c), mc.pair_ulp(p, a, b, c)


def test_accuracy_over_near_surface_pairs(shim, accuracy_pairs):
    (p, a, b, c), want, ulp = accuracy_pairs
    assert len(p) == mc.ACCURACY_PAIRS and np.abs(np.stack([a, b, c])).max() <= 2.0 and np.abs(p).max() <= 3.5
    got = hms.point_triangle_dist(shim, p, a, b, c)
    assert np.isfinite(got).all()
    worst = float((np.abs(got.astype(np.float64) - want) / ulp).max())
    print("shim: worst deviation %.2f ulp(L) over %d pairs" % (worst, len(p)))
    path = os.environ.get("SMALFIT_WRITE_MESH_SCORE_MEASURED")
    if path:
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc["shim/near_surface_ulp"] = worst
        json.dump(doc, open(path, "w"), indent=1, sort_keys=True)
    rec = recorded()["shim/near_surface_ulp"]
    assert worst <= mc.REGION_WALK_FLOOR, worst
    assert worst <= mc.SHIM_BAR_FACTOR * rec, (worst, rec)


def test_the_bar_keeps_a_region_walk_out(accuracy_pairs):
    (p, a, b, c), want, ulp = accuracy_pairs
    k = 200_000
    worst = float((np.abs(mc.region_walk_dist32(p[:k], a[:k], b[:k], c[:k]).astype(np.float64) - want[:k]) / ulp[:k]).max())
    assert worst > 4 * mc.REGION_WALK_FLOOR, worst          # (553 ulp(L) on this fifth of the pairs; 3e4 over all of them)


def test_surface_scan_is_the_pairwise_minimum(shim):
    verts, faces = mc.soup(37, seed=5)
    q = mc.points_near(verts, faces, 50, seed=6)
    got = hms.surface_dist(shim, q, verts, faces)
    v = verts[faces]
    pair = np.stack([hms.point_triangle_dist(shim, q, *(np.tile(v[f, i], (len(q), 1)) for i in range(3))) for f in range(len(faces))])
    assert (got == pair.min(0)).all()
    want = mc.surface_dist(q, verts, faces)
    assert mc.deviation_ulp(got, want, mc.ulp_l(q, verts)) <= mc.SHIM_BAR_FACTOR * recorded()["shim/near_surface_ulp"]


def test_the_references_agree():
    verts, faces = mc.soup(600, seed=9)
    q = mc.points_near(verts, faces, 300, seed=10, sigma=0.05)
    assert (mc.surface_dist_culled(q, verts, faces, block=64) == mc.surface_dist(q, verts, faces)).all()
    rv, rf = mc.ribbon(130, seed=2)
    assert (mc.surface_dist_culled(rv, verts, faces) == mc.surface_dist(rv, verts, faces)).all()
    # the cube against its translated copy: the brute force gives the closed form
    for shift in mc.CUBE_SHIFTS:
        want = mc.box_surface_dist(mc.CUBE_VERTS, shift, shift + 1.0)
        assert np.abs(mc.surface_dist(mc.CUBE_VERTS, mc.CUBE_VERTS + shift, mc.CUBE_FACES) - want).max() < 1e-15
    np.testing.assert_allclose(mc.box_surface_dist(mc.CUBE_VERTS[[0, 6]], mc.CUBE_SHIFT, mc.CUBE_SHIFT + 1.0),
                               [np.hypot(0.25, 0.5), 0.125])


# ---- rules --------------------------------------------------------------------------------------------------------
def _refusal(shim, a, target_meshes=None):
    return hms.refusal(shim, a, mc.MAX_MESHES, mc.MAX_POINTS, a.num_meshes if target_meshes is None else target_meshes)


def test_every_rule_and_its_text(shim):
    assert _refusal(shim, mc.valid_args()) is None
    for name, change, targets, text in mc.REFUSALS:
        a = mc.valid_args()
        change(a)
        assert _refusal(shim, a, targets) == text, name
    src = open(os.path.join(os.path.dirname(MEASURED), "..", "..", "smalify_amd", "csrc", "smalfit_plan.h")).read()
    body = src[src.index("inline const char* mesh_score_args_refusal"):]
    body = body[:body.index("\n}\n")]
    texts = [t for t in mc.RULE_ORDER]
    # every text the function can return is one of the table's, in the table's order
    pos = [body.index('"%s"' % t) for t in texts]
    assert pos == sorted(pos)
    assert body.count('return "') == len(texts)


POINT_FIELDS = frozenset(["points", "num_points", "point_dist"])
THRESHOLD_FIELDS = frozenset(["num_thresholds", "thresholds", "within"])


def test_rule_order(shim):
    first = {}
    for name, change, targets, text in mc.REFUSALS:
        first.setdefault(text, (change, targets))
    texts = list(first)
    checked = 0
    for i, ti in enumerate(texts):
        for tj in texts[i + 1:]:
            (ci, gi), (cj, gj) = first[ti], first[tj]
            # (the fields of the second direction are judged together, and so are those of the thresholds: changes to two of a group are one change)
            fi, fj = ci.fields, cj.fields
            for group in (POINT_FIELDS, THRESHOLD_FIELDS):
                fi, fj = (f | group if f & group else f for f in (fi, fj))
            if fi & fj or (gi is not None and gj is not None):
                continue
            a = mc.valid_args()
            cj(a)
            ci(a)
            g = gi if gi is not None else gj
            assert _refusal(shim, a, g) == ti, (ti, tj)
            checked += 1
    assert checked >= 20


def test_accepted_edges(shim):
    # T = 0 with within NULL
    a = mc.valid_args(T=0)
    assert a.within is None and _refusal(shim, a) is None
    # T = 8, and T > 0 without within (the counts are optional)
    assert _refusal(shim, mc.valid_args(T=8)) is None
    a = mc.valid_args(T=2)
    a.within = None
    assert _refusal(shim, a) is None
    # points NULL with S = 0: one direction only
    a = mc.valid_args(S=0)
    assert a.points is None and a.num_points == 0 and a.point_dist is None and _refusal(shim, a) is None
    # S = 1 and S = max_points; the distances are optional
    for S in (1, mc.MAX_POINTS):
        assert _refusal(shim, mc.valid_args(S=S)) is None
    assert _refusal(shim, mc.valid_args(distances=False)) is None
    # N = 1 and N = max_meshes
    for N in (1, mc.MAX_MESHES):
        assert _refusal(shim, mc.valid_args(N=N)) is None
    # the smallest positive threshold
    a = mc.valid_args(T=1)
    a.thresholds[0] = np.float32(1e-45)
    assert _refusal(shim, a) is None


def test_struct_layout_and_binding(shim):
    cls = _lib.MeshScoreArgs
    assert shim.hms_sizeof_args() == C.sizeof(cls)
    assert hms.offsets(shim) == [getattr(cls, f).offset for f, _ in cls._fields_]
    assert shim.hms_max_thresholds() == _lib.MAX_SCORE_THRESHOLDS == 8
    assert "smalfit_mesh_score" in _lib.SIGNATURES and "smalfit_mesh_score" in _lib.LAZY_SYMBOLS
    assert cls().struct_size == C.sizeof(cls)


def test_record_and_grids(shim):
    chunk = hms.surface_chunk()
    assert shim.hms_sizeof_scan_tri() == 64 and chunk * 64 == 32768         # four 16-byte rows; 32 KB staged
    assert shim.hms_queries() == mc.QUERIES
    for q, N in ((1, 1), (63, 2), (64, 1), (65, 3), (130, 1), (3889, 32), (3000, 32)):
        assert hms.grid2(shim.hms_surface_dist_grid, q, N) == ((q + 63) // 64, N)
    assert hms.grid2(shim.hms_surface_dist_grid, 3889, 1) == (61, 1)
    assert hms.grid2(shim.hms_score_reduce_grid, 5) == (2, 5)
    assert mc.scanned_counts(chunk) == (1, 2, 3, 5, 511, 512, 513, 1027)


# ---- the summary ---------------------------------------------------------------------------------------------------
def test_summarise_mesh_score_by_hand():
    # mesh 0: 4 vertices at distances 0, 1, 1, 2 and 2 points at 3, 4; mesh 1: 4 vertices all at 0.5, direction 1 as mesh 0's
    sums = np.array([[[4.0, 6.0, 2.0], [7.0, 25.0, 4.0]],
                     [[2.0, 1.0, 0.5], [7.0, 25.0, 4.0]]], np.float32)
    within = np.array([[[1, 3], [0, 0]],
                       [[4, 4], [0, 1]]], np.int32)           # thresholds 0.5, 3.0 (mesh 0: d <= .5: 1 vertex, <= 3: ... )
    s = metrics.summarise_mesh_score(sums, within, num_verts=4, num_points=2, thresholds=(0.5, 3.0))
    np.testing.assert_allclose(s["vert_mean"], [1.0, 0.5])
    np.testing.assert_allclose(s["vert_rms"], [np.sqrt(1.5), 0.5])
    np.testing.assert_allclose(s["vert_max"], [2.0, 0.5])
    np.testing.assert_allclose(s["point_mean"], [3.5, 3.5])
    np.testing.assert_allclose(s["point_rms"], [np.sqrt(12.5), np.sqrt(12.5)])
    np.testing.assert_allclose(s["point_max"], [4.0, 4.0])
    np.testing.assert_allclose(s["hausdorff"], [4.0, 4.0])
    np.testing.assert_allclose(s["chamfer_l2"], [1.5 + 12.5, 0.25 + 12.5])
    np.testing.assert_allclose(s["precision"], [[0.25, 0.75], [1.0, 1.0]])
    np.testing.assert_allclose(s["recall"], [[0.0, 0.0], [0.0, 0.5]])
    # harmonic mean; 0 when both are 0
    np.testing.assert_allclose(s["fscore"], [[0.0, 0.0], [0.0, 2 * 1.0 * 0.5 / 1.5]])
    assert s["fscore"][0, 1] == 0.0 and s["fscore"][0, 0] == 0.0
    b = s["batch"]
    assert b["meshes"] == 2
    np.testing.assert_allclose(b["vert_mean"], 0.75)
    np.testing.assert_allclose(b["hausdorff"], 4.0)
    np.testing.assert_allclose(b["fscore"], [0.0, np.mean([0.0, 2 / 3])])
    assert b["worst_mesh"] in (0, 1)

    # one direction only: everything of direction 1 is nan, and so are the figures that need both
    sums1, within1 = sums.copy(), within.copy()
    sums1[:, 1], within1[:, 1] = 0, 0                        # what the device writes without points
    one = metrics.summarise_mesh_score(sums1, within1, num_verts=4, num_points=0, thresholds=(0.5, 3.0))
    np.testing.assert_allclose(one["vert_mean"], [1.0, 0.5])
    np.testing.assert_allclose(one["precision"], [[0.25, 0.75], [1.0, 1.0]])
    for k in ("point_mean", "point_rms", "point_max", "recall", "fscore", "chamfer_l2", "hausdorff"):
        assert np.isnan(one[k]).all(), k
    # no thresholds: the threshold tables are empty, the rest stands
    none = metrics.summarise_mesh_score(sums, None, num_verts=4, num_points=2)
    assert none["precision"].shape == (2, 0) and none["fscore"].shape == (2, 0)
    np.testing.assert_allclose(none["hausdorff"], [4.0, 4.0])
    # the report is plain json with one entry per mesh
    doc = metrics.mesh_score_report(s, (0.5, 3.0), ["a.obj", "b.obj"])
    back = json.loads(json.dumps(doc))
    assert list(back["meshes"]) == ["a.obj", "b.obj"] and back["meshes"]["b.obj"]["fscore"][1] == pytest.approx(2 / 3)
    assert back["thresholds"] == [0.5, 3.0]
