"""CPU: the host side of the fit metrics (smalfit_fit_metrics; tests/test_gpu_metrics.py runs the kernels).

  rules     every rule of smalfit_plan.h::metrics_args_refusal through tests/host_metrics_shim.cpp: its text, its place in the
            order, the accepted edge beside it
  grids     the three launches' grids as literal numbers
  summarise IoU and PCK from hand-written counts
  binding   the symbol is exported; the ctypes mirror has the header's size
  scenes    the closed forms of tests/metrics_cases.py keep their margins; the PCK inputs keep theirs
  cap       on the oracle alone: the relaxed and the strict coverage of every whole-mesh input differ in at most 3 % of the
            relaxed set's pixels -- the room the GPU test's `strict <= mask <= relaxed` leaves
"""
import ctypes as C
import math

import numpy as np
import pytest

from smalify_amd import _lib, metrics as met
from tests import host_metrics as hm
from tests import metrics_cases as mc


@pytest.fixture(scope="module")
def shim():
    return hm.load()


# ---- rules -------------------------------------------------------------------------------------------------------------
def _pointers():
    return {k: 0x1000 + 0x100 * i for i, k in enumerate(mc.POINTERS)}


@pytest.mark.parametrize("name", list(mc.REFUSALS))
def test_rule(shim, name):
    fields, text = mc.REFUSALS[name]
    assert hm.refusal(shim, mc.block(fields, _pointers()), mc.MAX) == text


def test_every_rule_is_reached_and_worded_once():
    texts = [t for _, t in mc.REFUSALS.values() if t is not None]
    assert set(texts) == set(mc.RULE_ORDER) and len(set(mc.RULE_ORDER)) == 8
    # each "order:" case breaks two rules and names the earlier one
    for name, (fields, text) in mc.REFUSALS.items():
        if name.startswith("order:"):
            assert text in mc.RULE_ORDER[:-1]


def test_order_of_the_rules(shim):
    """break rule i together with every later rule: rule i's text"""
    breakers = [dict(struct_size=8), dict(num_frames=0), dict(sil_counts=None), dict(target_sil=None, target_sil_u8=None),
                dict(target_visibility=None), None, dict(num_thresholds=9), dict(thresholds=(mc.NAN,))]
    for i, first in enumerate(breakers):
        if first is None:
            continue
        for j in range(i + 1, len(breakers)):
            if breakers[j] is None:
                continue
            fields = dict(breakers[j])
            fields.update(first)
            assert hm.refusal(shim, mc.block(fields, _pointers()), mc.MAX) == mc.RULE_ORDER[i], (i, j)
    # the sixth rule (outputs without inputs) excludes the fifth by construction; it comes before the thresholds are looked at
    fields = dict(mc.NO_KEYPOINTS, keypoint_dist=1, num_thresholds=9, thresholds=(mc.NAN,))
    assert hm.refusal(shim, mc.block(fields, _pointers()), mc.MAX) == mc.OUTPUTS_TEXT


def test_threshold_count_edges(shim):
    ok = (0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.4, 0.5, 0.6)
    got = {T: hm.refusal(shim, mc.block(dict(num_thresholds=T, thresholds=ok[:max(T, 0)][:8]), _pointers()), mc.MAX) for T in range(-1, 11)}
    assert got == {T: (None if 1 <= T <= 8 else mc.COUNT_TEXT) for T in range(-1, 11)}
    assert shim.hm_max_thresholds() == 8 == _lib.MAX_PCK_THRESHOLDS
    for T in (1, 8):                       # every position is looked at
        for bad in (mc.NAN, 0.0, -1.0, mc.INF, -mc.INF):
            for at in range(T):
                thr = list(ok[:T])
                thr[at] = bad
                assert hm.refusal(shim, mc.block(dict(num_thresholds=T, thresholds=thr), _pointers()), mc.MAX) == mc.VALUE_TEXT


def test_frame_count_edges(shim):
    for cap in (1, 3, 9):
        got = [hm.refusal(shim, mc.block({}, _pointers(), num_frames=M), cap) for M in (0, 1, cap, cap + 1)]
        assert got == [mc.FRAMES_TEXT, None, None, mc.FRAMES_TEXT]


# ---- grids -------------------------------------------------------------------------------------------------------------
def test_grids_are_these_numbers(shim):
    assert shim.hm_sil_count_pixels() == 16
    cover = {(F, M): hm.grid2(shim.hm_cover_grid, F, M) for F in (15, 16, 17) for M in (1, 3, 9)}
    assert cover == {(15, 1): (1, 1), (15, 3): (1, 3), (15, 9): (1, 9), (16, 1): (1, 1), (16, 3): (1, 3), (16, 9): (1, 9),
                     (17, 1): (2, 1), (17, 3): (2, 3), (17, 9): (2, 9)}
    assert hm.grid2(shim.hm_cover_grid, 7774, 64) == (486, 64)             # SMAL's faces
    slabs = {(S, M): hm.grid2(shim.hm_sil_counts_grid, S, M) for S in (16, 50, 51) for M in (1, 3, 9)}
    assert slabs == {(16, 1): (1, 1), (16, 3): (1, 3), (16, 9): (1, 9), (50, 1): (1, 1), (50, 3): (1, 3), (50, 9): (1, 9),
                     (51, 1): (1, 1), (51, 3): (1, 3), (51, 9): (1, 9)}
    # one slab holds 256 threads x 16 pixels = 4096 pixels = 64^2; the sizes the GPU tests and the fitters use
    more = {S: hm.grid2(shim.hm_sil_counts_grid, S, 2)[0] for S in (1, 64, 65, 128, 256, 512, 1024)}
    assert more == {1: 1, 64: 1, 65: 2, 128: 4, 256: 16, 512: 64, 1024: 256}
    assert [shim.hm_pck_grid(M) for M in (1, 3, 9, 64)] == [1, 3, 9, 64]


# ---- summarise ---------------------------------------------------------------------------------------------------------
def test_keypoint_groups():
    assert met.KEYPOINT_GROUPS == {"legs": tuple(range(12)), "tail": (12, 13, 24), "ears": (14, 15, 18, 19),
                                   "face": (16, 17, 20, 21), "torso": (22, 23)}
    assert sorted(i for g in met.KEYPOINT_GROUPS.values() for i in g) == list(range(25)) and len(met.KEYPOINT_NAMES) == 25


def test_summarise_by_hand():
    counts = np.array([[30, 60, 40, 50], [0, 0, 0, 0], [0, 7, 7, 0], [5, 5, 5, 5]])
    vis = np.zeros((4, 25), np.float32)
    dist = np.full((4, 25), 9.0, np.float32)
    vis[0, :20] = 1.0                     # frame 0: 20 visible, 10 of them within 0.15, 15 within 0.3; nothing visible on the tail (24)
    dist[0, :10], dist[0, 10:15] = 0.1, 0.2
    vis[1, [22, 23]] = 0.5                # frame 1: 2 visible (torso), both within; visibility is "> 0"
    dist[1, [22, 23]] = 0.0
    dist[2] = np.inf                      # frame 2: empty target, 3 visible keypoints, none can be within
    vis[2, [0, 12, 16]] = 1.0
    dist[3, 5] = np.nan                   # frame 3: nothing visible; a nan distance is within nothing
    s = met.summarise(counts, dist, vis, (0.15, 0.3))
    assert s["iou"][0] == 0.5 and math.isnan(s["iou"][1]) and s["iou"][2] == 0.0 and s["iou"][3] == 1.0
    assert s["visible"].tolist() == [20, 2, 3, 0] and s["correct"].tolist() == [[10, 15], [2, 2], [0, 0], [0, 0]]
    assert s["pck"][:3].tolist() == [[0.5, 0.75], [1.0, 1.0], [0.0, 0.0]] and np.isnan(s["pck"][3]).all()
    # groups: legs of frame 0 are keypoints 0..11 (10 within 0.15, all 12 within 0.3); its tail has keypoints 12, 13 visible, 24 not
    assert s["pck_groups"]["legs"][0].tolist() == [10 / 12, 1.0]
    assert s["pck_groups"]["tail"][0].tolist() == [0.0, 1.0]
    assert np.isnan(s["pck_groups"]["torso"][0]).all()                      # a group without a visible keypoint
    assert s["pck_groups"]["torso"][1].tolist() == [1.0, 1.0] and np.isnan(s["pck_groups"]["legs"][1]).all()
    seq = s["sequence"]
    assert seq["iou"] == (0.5 + 0.0 + 1.0) / 3 and seq["frames_with_iou"] == 3          # the nan frame is left out, not counted as 0
    assert seq["visible"] == 25 and seq["pck"].tolist() == [12 / 25, 17 / 25]
    frame_mean = np.nanmean(s["pck"], 0)
    assert frame_mean.tolist() == [0.5, (0.75 + 1.0) / 3] and not np.allclose(seq["pck"], frame_mean)    # micro-average, not the frames' mean
    assert seq["pck_groups"]["torso"].tolist() == [1.0, 1.0] and seq["pck_groups"]["ears"].tolist() == [0.0, 0.25]
    # silhouette only; every frame empty
    s = met.summarise(np.zeros((2, 4), np.int32))
    assert np.isnan(s["iou"]).all() and math.isnan(s["sequence"]["iou"]) and "pck" not in s


def test_thresholds_are_compared_as_float32():
    """the device compares float32 with float32: a distance equal to float32(0.15) is within 0.15"""
    d = np.full((1, 25), np.float32(0.15), np.float32)
    assert float(d[0, 0]) > 0.15
    s = met.summarise([[1, 1, 1, 1]], d, np.ones((1, 25)), (0.15,))
    assert s["correct"].tolist() == [[25]]


def test_report_round_trips_through_json(tmp_path):
    s = met.summarise([[1, 2, 1, 2], [0, 0, 0, 0]], np.zeros((2, 25), np.float32), np.ones((2, 25)), (0.15,))
    path = tmp_path / "metrics.json"
    met.write_report(str(path), s, (0.15,), ["a.png", "b.png"])
    import json
    doc = json.load(open(path))
    assert doc["thresholds"] == [0.15] and list(doc["frames"]) == ["a.png", "b.png"]
    assert doc["frames"]["a.png"]["iou"] == 0.5 and math.isnan(doc["frames"]["b.png"]["iou"]) and doc["frames"]["a.png"]["pck"] == [1.0]
    assert doc["sequence"]["iou"] == 0.5 and doc["sequence"]["pck"] == [1.0]
    assert "IoU 0.5000 over 1 frame(s)" in met.summary_line(s, (0.15,)) and "PCK@0.15 1.0000" in met.summary_line(s, (0.15,))


# ---- binding -----------------------------------------------------------------------------------------------------------
def test_symbol_and_struct(shim):
    if _lib.needs_rebuild():
        _lib.build_library()
    lib = _lib.load()
    assert hasattr(lib, "smalfit_fit_metrics") and "smalfit_fit_metrics" in _lib.SIGNATURES
    assert C.sizeof(_lib.MetricsArgs) == shim.hm_sizeof_metrics_args()
    assert _lib.MetricsArgs.thresholds.offset == shim.hm_offsetof_thresholds()
    assert _lib.MetricsArgs().struct_size == C.sizeof(_lib.MetricsArgs)
    assert lib.smalfit_version() == _lib.ABI_VERSION == 6                  # a new entry point, not a new version


# ---- the GPU tests' inputs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", mc.SIZES)
@pytest.mark.parametrize("name", mc.SCENES)
def test_scene_keeps_its_margin(name, S):
    sc = mc.scene(name, S)
    assert sc["margin"] > mc.MARGIN_PX, sc["margin"]
    assert sc["target"].sum() > 0 and len(sc["verts"]) == 3 * len(sc["faces"])
    if name == "nothing":
        assert not sc["mask"].any()
        return
    c = mc.counts(sc["mask"], sc["target"])
    assert 0 < c[0] < c[2] < c[1] and c[0] < c[3], c                        # the four numbers say four things
    if name == "clipped":                                                  # every border has covered pixels
        m = sc["mask"]
        assert m[:, 0].any() and m[:, -1].any() and m[0].any() and m[-1].any() and m[0, -1]
    if name == "overlap":
        a = mc.inside([(0.153 * S, 0.091 * S), (0.791 * S, 0.207 * S), (0.322 * S, 0.863 * S)], S)[0]
        assert (sc["mask"] & a).sum() == a.sum() and 0 < a.sum() < sc["mask"].sum()


def test_binarisation_values():
    assert (mc.FLOAT_VALUES > 0.5).tolist() == [False, True, False, True] and (mc.BYTE_VALUES >= 128).tolist() == [False, True, False, True]
    p = mc.pattern(3, 51)
    assert sorted(np.unique(p)) == [0, 1, 2, 3] and not np.array_equal(p[0], p[1])


@pytest.mark.parametrize("T", sorted(mc.THRESHOLDS))
def test_pck_inputs_keep_clear_of_the_thresholds(T):
    thr = mc.THRESHOLDS[T]
    areas = [700, 0, 331, 1200]
    proj, tgt = mc.pck_inputs(4, 50, areas, thr)
    dist, rows, clearance = mc.pck_expected(proj, tgt, mc.visibility(4, "all"), areas, thr)
    assert clearance >= mc.PCK_CLEARANCE, clearance
    assert np.isinf(dist[1]).all() and rows[1].tolist() == [25] + [0] * T
    assert (np.diff(rows[:, 1:], axis=1) >= 0).all()                       # wider thresholds hold more
    assert 0 < rows[0, 1] and rows[0, T] < 25                              # neither all nor none
    none = mc.pck_expected(proj, tgt, mc.visibility(4, "none"), areas, thr)[1]
    assert not none.any()


# ---- the cap of the whole-mesh GPU test ---------------------------------------------------------------------------------------
def test_strict_and_relaxed_coverage_differ_in_at_most_three_percent():
    from oracle import smal_oracle as so
    from tests import color_cases as cc
    for view, S in cc.INPUTS:
        md, v = cc.view(view)
        w = so.hard_phong_winners(v, np.asarray(md.faces), S)
        relaxed, gap = int(w["relaxed"].sum()), int((w["relaxed"] & ~w["strict"]).sum())
        assert relaxed > 0 and gap <= 0.03 * relaxed, (view, S, gap, relaxed)
        assert not (w["strict"] & ~w["relaxed"]).any()
