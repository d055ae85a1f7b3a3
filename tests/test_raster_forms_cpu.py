"""The crafted scenes of tests/test_gpu_raster_forms.py reach every branch of the rasteriser they are named for, and
tests/raster_forms.py still restates the kernels' capacities and decisions (no GPU needed)."""
import math
import os
import re

import numpy as np
import pytest

from tests import host_plan
from tests import raster_forms as rf

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "smalify_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _const(src, name):
    m = re.search(r"constexpr (?:int|float|unsigned char) %s = ([0-9.]+)f?;" % name, src)
    assert m, name
    return float(m.group(1))


def test_the_constants_are_the_kernels():
    r = _src("kernels_raster.inc")
    assert _const(_src("smalfit_math.h"), "kFacesPerPixel") == rf.K
    for name, val in (("kListCap", rf.LIST_CAP), ("kListLds", rf.LIST_LDS), ("kMaskRounds", rf.MASK_ROUNDS),
                      ("kAccWin", rf.ACC_WIN),
                      ("kBandCap", rf.BAND_CAP), ("kBandFill", rf.BAND_FILL), ("kBandHalf", rf.BAND_HALF),
                      ("kBandTries", rf.BAND_TRIES), ("kCandCap", rf.CAND_CAP), ("kHitCap", rf.HIT_CAP),
                      ("kCoverCap", rf.COVER_CAP)):
        assert _const(r, name) == val, name
    for name, val in (("kSweepFaces", rf.SWEEP_FACES), ("kRectFaces", rf.RECT_FACES)):      # the constants a launch is sized by
        assert _const(_src("smalfit_plan.h"), name) == val, name
    assert "constexpr int kBandFillWide = %d, kBandFillNarrow = %d;" % (rf.BAND_FILL_WIDE, rf.BAND_FILL_NARROW) in r
    assert "constexpr float kBoxSlack = 1.0f / 64.0f;" in r
    assert host_plan.load().MAX_IMAGE_SIZE == rf.MAX_S          # smalfit_engine_create refuses larger images


def test_the_decisions_are_the_kernels():
    r = _src("kernels_raster.inc")
    # sweep -> backward hand-off: per-face list / mask / walk, one format per wave of four
    assert "const bool listed = npx <= %d;" % rf.LIST_BOX in r
    assert "const bool has_list = npx2 <= %d && cnt <= kListLds;" % rf.LIST_BOX in r
    assert re.search(r"if \(__ballot\(!has_list\) == 0ull\) \{.*?\} else if \(npx2 <= 16 \* kMaskRounds\) \{\s*flag = kMaskList;.*?"
                     r"\} else \{\s*flag = kNoList;", r, re.S)
    assert "const bool clip = rw > kAccWin || rh > kAccWin;" in r
    # resolve
    assert re.search(r"if \(saturated\) act = 0;\s*else if \(!\(zb\.x < kInf\)\) act = \(c <= K\) \? 0 : 1;\s*"
                     r"else if \(need < 0 \|\| b > kBandCap\) act = 1;\s*else if \(need == 0\) zthr = zb\.x;[^\n]*\n\s*"
                     r"else if \(need > b\) act = \(zb\.y < kInf\) \? 1 : \(b == 0 \? 0 : 2\);[^\n]*\n\s*else act = 2;", r)
    assert "(26ull << 24)" in r
    assert "(bs[s] > %d ? (int)0x80000000 : 0)" % rf.BAND_WIDE in r
    # selection: half-widths, band choice, short-miss marking
    assert "const float delta0 = (nc > K) ? kBandHalf * (zk - zmn) * (1.0f / (float)K) : 0.f;" in r
    assert "if (!chosen && cbs[i] <= fill && zk - delta < zk) {" in r
    assert "blo = zk - delta; bhi = (zmx > thi[i]) ? zk + delta : kInf; chosen = true;" in r
    assert "if (hi_old < kInf && zk > hi_old) {" in r
    assert "if (z > hi_old && z <= zk) pc[L.fids[i]] = kNoList;" in r
    assert "bool compact = (nh <= kHitCap) && (ncov <= kCoverCap) && (F <= 65536);" in r
    assert "const bool cached = nc <= kCandCap;" in r
    # the band kernel's miss-rate rule and the selection's agree with the fill the cold call uses
    assert "(miss > 0.12f) ? kBandFillWide : ((miss > 0.02f) ? kBandFill : kBandFillNarrow)" in r


def test_rule_boundaries():
    assert rf.face_format(256, 128) == rf.LIST and rf.face_format(256, 129) == rf.MASKS
    assert rf.face_format(257, 10) == rf.MASKS and rf.face_format(1024, 600) == rf.MASKS
    assert rf.face_format(1025, 10) == rf.NOLIST
    assert rf.wave_formats([20, 20, 20, 300], [5, 5, 5, 5]) == [rf.MASKS] * 4
    assert rf.wave_formats([20, 20, 20, 2000], [5, 5, 5, 5]) == [rf.MASKS] * 3 + [rf.NOLIST]
    zs = rf.Z0 + rf.GAP * np.arange(101.0)
    lo, hi, zk, delta = rf.select_bounds(zs)
    assert zk == zs[99] and hi == math.inf and abs(delta - 3.96 * rf.GAP) < 1e-12
    assert rf.resolve_action(zs, math.inf, math.inf) == "fresh_select"
    assert rf.resolve_action(zs[:100], math.inf, math.inf) == "fresh_done"


def _pairs(verts, faces):
    v = rf.to_f32(verts)
    P = rf.pairs(v, faces)
    assert rf.margins_ok(P), "a pixel centre lies too close to an edge or to the blur radius"
    return v, P


def test_format_faces_land_in_their_classes():
    verts, faces, names = rf.format_faces()
    v, P = _pairs(verts, faces)
    boxes, bm = rf.face_boxes(v, faces)
    assert bm.min() > rf.BOX_SLACK + rf.MARGIN_PX                    # box sizes are unambiguous
    npx = rf.box_pixels(boxes)
    cnt, qmax = rf.per_face(P, len(faces))
    fmt = rf.wave_formats(npx, cnt)
    want = {"list": rf.LIST, "list_full": rf.LIST, "masks_by_wave": rf.MASKS, "masks_list_overflow": rf.MASKS,
            "masks_big_box": rf.MASKS, "masks_1024": rf.MASKS, "nolist_1040": rf.NOLIST, "nolist_big_box": rf.NOLIST}
    for i, name in enumerate(names):
        if name in want:
            assert fmt[i] == want[name], (i, name, npx[i], cnt[i], fmt[i])
    i = names.index("list_full")
    assert npx[i] == rf.LIST_BOX and cnt[i] == rf.LIST_LDS                          # the list's last entry in use
    i = names.index("masks_list_overflow")
    assert npx[i] == rf.LIST_BOX and cnt[i] == rf.LIST_LDS + 1                      # one entry too many
    i = names.index("masks_big_box")
    assert rf.LIST_BOX < npx[i] < 16 * rf.MASK_ROUNDS
    i = names.index("masks_1024")
    assert npx[i] == 16 * rf.MASK_ROUNDS and qmax[i] == npx[i] - 1                  # a candidate in the masks' last round
    i = names.index("nolist_1040")
    assert npx[i] == 16 * (rf.MASK_ROUNDS + 1) and qmax[i] >= 16 * rf.MASK_ROUNDS   # candidates past the masks' last round
    assert npx[names.index("nolist_big_box")] > 2 * 16 * rf.MASK_ROUNDS
    # the three list faces of a wave with a mask face would have had lists on their own
    assert any(n == "masks_by_wave" and rf.face_format(npx[i], cnt[i]) == rf.LIST for i, n in enumerate(names))
    # a block of 32 small faces wider and taller than the LDS window; its faces hold lists
    f0 = names.index("clip_block")
    assert f0 % rf.SWEEP_FACES == 0 and names[f0:f0 + rf.SWEEP_FACES] == ["clip_block"] * rf.SWEEP_FACES
    w, h = rf.block_rect(boxes, f0)
    assert w > rf.ACC_WIN and h > rf.ACC_WIN
    assert all(fmt[i] == rf.LIST for i in range(f0, f0 + rf.SWEEP_FACES))
    # no depth ties between overlapping faces
    zz, _, _ = rf.per_pixel(P)
    assert all(len(np.unique(z)) == len(z) for z in zz.values())


def test_list_edge_faces():
    verts, faces, names = rf.list_edge_faces()
    v, P = _pairs(verts, faces)
    boxes, bm = rf.face_boxes(v, faces)
    assert bm.min() > rf.BOX_SLACK + rf.MARGIN_PX
    npx = rf.box_pixels(boxes)
    cnt, _ = rf.per_face(P, len(faces))
    assert rf.wave_formats(npx, cnt) == [rf.LIST] * 4 + [rf.MASKS] * 4
    assert list(npx[[3, 7]]) == [rf.LIST_BOX] * 2 and list(cnt[[3, 7]]) == [rf.LIST_LDS, rf.LIST_LDS + 1]
    zz, _, ll = rf.per_pixel(P)
    assert all(len(z) == 1 for z in zz.values())                                   # no overlaps
    # the last 16 box pixels' candidates (the last round the sweep walks) are not saturated: they carry gradient
    for f in (3, 7):
        sel = P["cand"] & (P["face"] == f) & (P["q"] >= npx[f] - 16)
        assert sel.any() and all(ll[int(p)].sum() < 20.0 for p in P["pix"][sel])


@pytest.mark.parametrize("n", rf.STACK_COUNTS)
def test_stacks_reach_their_candidate_counts(n):
    verts, faces = rf.count_stack(n)
    v, P = _pairs(verts, faces)
    boxes, bm = rf.face_boxes(v, faces)
    assert bm.min() > rf.BOX_SLACK + rf.MARGIN_PX
    zz, ff, _ = rf.per_pixel(P)
    counts = np.array([len(z) for z in zz.values()])
    assert counts.max() == n and np.sum(counts == n) >= 10          # the full pixels see every layer
    # distinct depths: the K cut is a pure rank, at least GAP / 2 wide
    for z in zz.values():
        assert np.all(np.diff(z) > 0.5 * rf.GAP)
    # the layers' shifts differ among the K nearest and the rest: the cut changes the silhouette
    if n > rf.K:
        full = [p for p, z in zz.items() if len(z) == n][0]
        near, far = ff[full][:rf.K], ff[full][rf.K:]
        sh = rf.mixed_shifts(n, n)
        assert len(set(sh[near])) > 1 and len(set(sh[far])) >= 1
    cnt, _ = rf.per_face(P, n)
    assert rf.box_pixels(boxes).max() <= rf.LIST_BOX and cnt.max() <= rf.LIST_LDS    # every layer holds a list


def test_cover_stack_passes_the_cover_cap_only():
    verts, faces = rf.cover_stack()
    v, P = _pairs(verts, faces)
    boxes, _ = rf.face_boxes(v, faces)
    zz, _, _ = rf.per_pixel(P)
    covered = []
    for p, z in zz.items():
        r, c = divmod(p, rf.S0)
        cover = np.sum((boxes[:, 0] <= c) & (c <= boxes[:, 1]) & (boxes[:, 2] <= r) & (r <= boxes[:, 3]))
        if cover > rf.COVER_CAP and rf.K < len(z) <= rf.CAND_CAP:
            covered.append(p)
    assert covered
    ub = rf.union_boxes(boxes)
    assert all(rf.covering(ub, *divmod(p, rf.S0)) <= rf.HIT_CAP for p in covered)     # the union-box list still fits


def test_hit_stack_passes_the_union_box_cap_only():
    verts, faces = rf.hit_stack()
    v, P = _pairs(verts, faces)
    boxes, bm = rf.face_boxes(v, faces)
    assert bm.min() > rf.BOX_SLACK + rf.MARGIN_PX
    r, c = rf.HIT_PIXEL
    assert rf.covering(rf.union_boxes(boxes), r, c) > rf.HIT_CAP                   # stage A's list overflows ...
    assert rf.covering(boxes, r, c) <= rf.COVER_CAP                                # ... while the faces covering the pixel
    zz, _, _ = rf.per_pixel(P)
    assert rf.K < len(zz[r * rf.S0 + c]) <= rf.CAND_CAP                            # and its candidates would fit
    assert len(faces) <= 65536 and len(verts) <= 8192 - 64


def test_cache_sequences_force_their_transitions():
    want = {"band_narrow": "band_narrow", "band_wide": "band_wide", "band_overflow_65": "band_overflow",
            "band_overflow": "band_overflow", "need_lt_0": "need_lt_0", "need_eq_0": "need_eq_0", "short_miss": "short",
            "band_tie": "band_narrow", "fresh_select": "fresh_select", "all_band": "all_band", "all_done": "all_done"}
    seqs = rf.cache_sequences()
    assert set(seqs) == set(want)
    seen = set()
    for name, seq in seqs.items():
        out, margin = rf.transitions(seq)
        assert margin > 0.05, (name, margin)          # no depth near any bound the first call could have chosen
        hits = [o for o in out.values() if o["action"] == want[name]]
        assert hits, name
        seen |= {o["action"] for o in out.values()}
        if name == "band_overflow_65":
            assert any(o["b"] == rf.BAND_CAP + 1 for o in hits)
        if name == "band_wide":
            assert all(rf.BAND_WIDE < o["b"] <= rf.BAND_CAP for o in hits)
        if name == "short_miss":
            assert all(o["hi"] < math.inf and o["zk"] > o["hi"] for o in hits)
        if name == "band_tie":
            assert all(o["tie_at_cut"] for o in out.values() if o["n"] > rf.K)
            assert any(o["tie_at_cut"] for o in hits)
        if name in ("all_band", "all_done"):
            assert all(o["hi"] == math.inf for o in hits)
    assert {"saturated", "fresh_done"} <= seen


def test_image_sizes():
    assert max(rf.SIZES) == rf.MAX_S and min(rf.SIZES) == 1
    verts, faces, S, checks = rf.big_triangle_1024()
    assert S == rf.MAX_S and any(0.0 < exp < 1.0 for _, _, exp in checks) and any(exp == 0.0 for _, _, exp in checks)
