"""What a wave of raster_bwd_kernel does once, whatever its faces: the face-keyed loads (32-bit offsets from the frame's base), the
two peeled list rounds and the first rolled one, the reduce-scatter of the six sums and the six stores.  Crafted 64 x 64 scenes
through smalfit_render_backward against the oracle's autograd, on the models and with the tolerances of
tests/test_gpu_raster_forms.py (each face has three vertices of its own, so a face's adjoint row is its vertices' gradient).

The scene: twelve list-class faces in three aligned waves -- candidate lists of 0 (a box without a candidate, and a face without a
box), 1, 15, 16, 17, 31, 32, 33, 49, 100 and 128 entries, the edges of the rounds -- and a last, ragged wave of 1, 2 or 3 faces
(F % 4): candidate masks, a box that is walked whole, a small face that takes masks with its wave.  From frame to frame the list
shapes move on by one slot (a load from another frame's base shows), the ragged wave by a pixel.  The lengths are asserted from
the engine's own hand-off (smalfit_engine_face_list_lengths), not only from the float64 count."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import raster_forms as rf                                                    # noqa: E402
from tests.test_gpu_raster_forms import GRAD_TOL, SIL_TOL, SLOTS, _model_data, _pad    # noqa: E402

S = rf.S0
MASK_LIST, NO_LIST = 254, 255           # kMaskList, kNoList of kernels_raster.inc (include/smalfit.h: smalfit_engine_face_list_lengths)
ROUND_EDGES = (0, 1, 15, 16, 17, 31, 32, 33)

# (w, h) of the wedge [(u, v - h), (u, v + h), (u - w, v + NUDGE)] with that many candidates (float64 count, margins kept;
# _expected_lengths asserts both), found by a scan over w and h
WEDGES = {15: (1.373, 1.853), 16: (1.2, 1.984), 17: (1.2, 2.115), 31: (1.2, 4.604), 32: (1.2, 4.735), 33: (1.2, 4.997),
          49: (2.065, 6.7), 100: (8.293, 6.831), 128: (11.58, 6.831)}
LIST_SHAPES = ("corner0", "corner1", 15, 16, 17, 31, 32, 33, 49, 100, 128, "offscreen")
TAIL = ("masks_big_box", "nolist_big_box", "masks_by_wave")
FU, FV = 0.137, 0.071                   # the wedges' offset from the pixel grid


def _wedge(cell, n, z):
    w, h = WEDGES[n]
    u, v = 14.0 + 16 * (cell % 4) + FU, 8.0 + 15 * (cell // 4) + FV
    return rf.world_face([(u, v - h), (u, v + h), (u - w, v + rf.NUDGE[0])], z)


def _list_face(shape, slot, z):
    if shape == "corner0":              # its box holds pixel (0, 0), 1.27 pixels from the face: an on-screen box without a candidate
        return rf.world_face([(-0.9, -0.93), (-3.0, -1.1), (-1.2, -3.0)], z)
    if shape == "corner1":              # the same corner from 0.67 pixels: a list of one
        return rf.world_face([(S - 1 + 0.45, -0.5), (S - 1 + 3.0, -0.6), (S - 1 + 0.6, -3.0)], z)
    if shape == "offscreen":            # no box at all
        return rf.layer_tri(-3 * S, 20.3, z)
    return _wedge(slot, shape, z)


def _tail_face(name, shift, z):
    # (below the three rows of list faces, and clear of each other: a pixel inside another face is saturated, and passes nothing on)
    if name == "masks_big_box":         # 40 x 8 pixels: too large for a list
        u0, v0, w, h = 2.5 + shift, 48.5, 40, 8
        return rf.world_face([(u0 + rf.NUDGE[2], v0), (u0 + w - rf.NUDGE[5], v0), (u0 + rf.NUDGE[2], v0 + h - rf.NUDGE[6])], z)
    if name == "nolist_big_box":        # 62 x 15, a box of 64 x 17: more than the masks cover
        u0, v0, w, h = 0.5, 47.5, 62, 15
        return rf.world_face([(u0 + w - rf.NUDGE[2], v0 + rf.NUDGE[3]), (u0 + w - rf.NUDGE[2], v0 + h), (u0 + rf.NUDGE[4], v0 + h)], z)
    return rf.small_face(49.5 + shift, 48.3, z)


def _frame(i, tail):
    """frame i of a scene with `tail` faces in its last wave: (3 F, 3) float64 vertices as float32 sees them"""
    n = len(LIST_SHAPES)
    tris = [_list_face(LIST_SHAPES[(slot + i) % n], slot, rf.Z0 + rf.GAP * ((5 * slot + i) % 17)) for slot in range(n)]
    tris += [_tail_face(TAIL[k], i % 3, rf.Z0 + 0.3 + 0.1 * ((k + i) % 3)) for k in range(tail)]
    return rf.to_f32(np.concatenate(tris))


def _faces(tail):
    F = len(LIST_SHAPES) + tail
    return np.arange(3 * F).reshape(F, 3)


def _expected_lengths(verts, faces):
    """the byte the sweep hands over per face, by the float64 count of tests/raster_forms.py; the scene keeps its margins"""
    P = rf.pairs(verts, faces)
    boxes, margin = rf.face_boxes(verts, faces)
    assert rf.margins_ok(P) and float(margin.min()) > rf.MARGIN_PX
    cnt, _ = rf.per_face(P, len(faces))
    fmt = rf.wave_formats(rf.box_pixels(boxes), cnt)
    return np.array([int(c) if f == rf.LIST else (MASK_LIST if f == rf.MASKS else NO_LIST) for c, f in zip(cnt, fmt)], np.uint8)


def _vertex_nearest_pixels(verts, faces):
    """pixels at which some face's nearest point is one of its vertices.  Both edges at that vertex are then equally near, to
    the last bit or not as the rounding falls, and only there do the two readings of the adjoint differ (an interior nearest
    point has t in (0, 1) either way): with the edge parameter unclamped the result depends on which of the two edges a
    rounding error picks, in float32 as in the oracle's float64.  The unclamped cases carry no upstream gradient there."""
    P = rf.pairs(verts, faces)
    x, y, _ = rf.project(verts)
    f = faces[P["face"]]
    px, py = rf.ndc_of_px(P["pix"] % S, P["pix"] // S)
    d = np.sort(np.stack([rf._seg(px, py, x[f[:, i]], y[f[:, i]], x[f[:, j]], y[f[:, j]])[0] for i, j in ((0, 1), (0, 2), (1, 2))]), 0)
    # (margins_ok: two edges with different nearest points are further apart than this)
    return np.unique(P["pix"][P["cand"] & (d[1] - d[0] < rf.MARGIN_PX * 2.0 / S)])


def _oracle(frames, faces, w, unclamped):
    from oracle import smal_oracle as so
    v = torch.from_numpy(np.stack(frames)).requires_grad_(True)
    so.EDGE_T_UNCLAMPED = unclamped
    try:
        sil = so.soft_silhouette(v, faces, S)
        (sil * torch.from_numpy(w).double()).sum().backward()
    finally:
        so.EDGE_T_UNCLAMPED = False
    return sil.detach().numpy(), v.grad.numpy()


_CACHE = {}


def _case(tail, M):
    """engine, frames, per option the upstream gradient and the oracle's (silhouette, d/d verts), the expected lengths --
    computed once per (tail, M)"""
    key = (tail, M)
    if key not in _CACHE:
        from smalify_amd import engine as eng
        faces = _faces(tail)
        frames = [_frame(i, tail) for i in range(M)]
        w = {False: np.random.RandomState(100 * tail + M).randn(M, S, S).astype(np.float32)}
        w[True] = w[False].copy()
        for n, fr in enumerate(frames):
            pix = _vertex_nearest_pixels(fr, faces)
            assert len(pix) > 30
            w[True][n].reshape(-1)[pix] = 0.0
        want = {u: _oracle(frames, faces, w[u], u) for u in (False, True)}
        e = eng.Engine(eng.DeviceModel(_model_data(faces)), M, S)
        _CACHE[key] = (e, frames, w, want, np.stack([_expected_lengths(f, faces) for f in frames]))
    return _CACHE[key]


def _run(e, frames, w, unclamped):
    """-> sil (M,S,S), d/d scene verts (M,3F,3) as float32 tensors on the host, the hand-off's lengths (M,F)"""
    e.reset_raster_cache()
    v = _pad(frames)
    sil, _ = e.render_forward(v)
    e.reset_raster_cache()
    e.set_option(e.OPT_UNCLAMPED_EDGE_T, int(unclamped))
    try:
        dv = e.render_backward(v, sil, torch.from_numpy(w).cuda())
    finally:
        e.set_option(e.OPT_UNCLAMPED_EDGE_T, 0)
    lengths = e.face_list_lengths(len(frames)).cpu().numpy()
    assert e.status() == 0
    return sil.cpu(), dv.cpu()[:, SLOTS[:len(frames[0])]], lengths


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.mark.parametrize("unclamped", (False, True), ids=("exact", "unclamped_t"))
@pytest.mark.parametrize("M", (1, 3, 9))
@pytest.mark.parametrize("tail", (1, 2, 3))
def test_wave_edges_against_the_oracle(tail, M, unclamped, capsys):
    e, frames, w, want, lengths_o = _case(tail, M)
    F = len(LIST_SHAPES) + tail
    assert F % 4 == tail
    w = w[unclamped]
    sil, dv, lengths = _run(e, frames, w, unclamped)
    # the lengths the scene is built for occur, by the engine's own count: every edge of the two peeled rounds and of the first
    # rolled one, a list past 48, masks, a whole box
    per_frame = [set(int(x) for x in row) for row in lengths]
    for row in per_frame:
        assert set(ROUND_EDGES) <= row and any(48 < x <= rf.LIST_CAP for x in row) and MASK_LIST in row, sorted(row)
        assert (NO_LIST in row) == (tail >= 2)
    assert np.array_equal(lengths, lengths_o), (lengths, lengths_o)
    assert all(int(np.sum(row == 0)) == 2 for row in lengths)          # the box without a candidate and the face without a box
    sil_o, dv_o = want[unclamped]
    sil, dv = sil.double().numpy(), dv.double().numpy()
    err_sil, err_all = float(np.abs(sil - sil_o).max()), _rel(dv, dv_o)
    worst = 0.0
    for n in range(M):
        for f in range(F):
            rows = slice(3 * f, 3 * f + 3)
            idle = not dv_o[n, rows].any()
            if not unclamped:                                           # a face without a candidate, and no other, gathers nothing
                assert idle == (lengths[n, f] == 0), (n, f)
            if idle:                                                    # (unclamped: or all of its pixels have a vertex nearest)
                assert not dv[n, rows].any(), (n, f)                    # exact zeros
                continue
            worst = max(worst, _rel(dv[n, rows], dv_o[n, rows]))
            assert _rel(dv[n, rows], dv_o[n, rows]) < GRAD_TOL, (n, f, int(lengths[n, f]), dv[n, rows], dv_o[n, rows])
    with capsys.disabled():
        print("\nF=%d M=%d %s: sil %.2e (<%.0e)  dverts %.2e, worst face %.2e (<%.0e)"
              % (F, M, "unclamped t" if unclamped else "exact", err_sil, SIL_TOL, err_all, worst, GRAD_TOL))
    assert err_sil < SIL_TOL and err_all < GRAD_TOL
    # vertices of no face (the padding, the frame's depth samples): the idle groups of the ragged wave stored nothing
    if unclamped is False:
        full = e.render_backward(_pad(frames), torch.from_numpy(sil).float().cuda(), torch.from_numpy(w).cuda()).cpu().numpy()
        used = np.zeros(full.shape[1], bool)
        used[SLOTS[:3 * F]] = True
        assert not full[:, ~used].any()


def test_the_options_differ_at_vertex_nearest_pixels_only():
    """what the unclamped cases above leave out is all there is to leave out: by the oracle, the two readings differ with the
    full upstream gradient and agree without the pixels whose nearest point is a vertex"""
    _, frames, w, want, _ = _case(3, 3)
    faces = _faces(3)
    assert _rel(_oracle(frames, faces, w[False], True)[1], want[False][1]) > 10 * GRAD_TOL
    assert _rel(want[True][1], _oracle(frames, faces, w[True], False)[1]) < 1e-12


@pytest.mark.parametrize("unclamped", (False, True), ids=("exact", "unclamped_t"))
def test_two_calls_give_identical_bits(unclamped):
    e, frames, w, _, _ = _case(3, 9)
    a, b = _run(e, frames, w[False], unclamped), _run(e, frames, w[False], unclamped)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert a[1].abs().max() > 0
