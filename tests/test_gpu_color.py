"""The hard-Phong colour render (kernels_color.inc: vnormal_kernel, color_zbuf_kernel, color_shade_kernel behind
smalfit_render_color; reference smal_fitter/p3d_renderer.py:41-59,70-72) pinned three ways (-m gpu):

  anchors     every closed form of tests/color_anchors.py through Engine.render_color, BAR = 1e-4 absolute per channel.
              Basis: the colour is (0.5 + 0.3 cos) c + 0.2 alpha^64; cos and alpha come out of three float32 normalisations and
              a few dot products of O(1) quantities, about 8 float32 epsilons = 1e-6, which the specular term amplifies by at
              most 0.2 x 64 = 12.8 to about 1.2e-5: 1e-4 leaves a factor of 8.  The back face, the white pixels, the
              reproducibility and one frame after three are exact statements.
  whole mesh  the inputs of tests/color_cases.py scored per pixel against the float64 oracle: on every DECIDED pixel
              (oracle.smal_oracle.hard_phong_winners: the same nearest face with weights and depths moved by 30 x their float32
              error) within the larger of BAR and YARD = 2 x the float32 oracle's own deviation on the same pixels; an undecided
              pixel white only if no face covers it by the strict margins and covered only if one does by the relaxed ones; the
              background exactly 1.0; at least 97 % of every input's covered pixels decided.
  collage     panels 2 and 5 of the fitters' st*_ep*.png are this render, byte for byte where no keypoint mark is drawn.

With tests/golden/hip_color_measured.json present every deviation also stays within RATCHET = 3 x what these kernels measured
when the file was written (floor 1e-5); SMALFIT_WRITE_COLOR_MEASURED=<path> writes it.  Every number is printed past the
capture."""
import json
import os
import struct
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from smalify_amd import config as cfg                # noqa: E402
from smalify_amd import engine as eng                # noqa: E402
from smalify_amd import model_io, synthetic          # noqa: E402
from tests import color_anchors as ca                # noqa: E402
from tests import color_cases as cc                  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
MEASURED = os.path.join(HERE, "golden", "hip_color_measured.json")
BAR, YARD, RATCHET, FLOOR = ca.DEVICE_BAR, 2.0, 3.0, 1e-5
FRAMES = 3             # capacity of every engine here: the multi-frame cases need no second one
V_PAD = 3100           # smalfit_model_create wants the SMAL landmark vertex ids (up to 3055) to exist


class Table:
    """the printed table of one test, its bound and ratchet checks, and the record of what was measured (the rule of
    tests/test_gpu_model_forms.py: Table, on a file of its own)"""

    def __init__(self, title):
        self.title, self.lines, self.bad, self.measured = title, [], [], {}
        self.recorded = json.load(open(MEASURED)) if os.path.exists(MEASURED) else {}

    def add(self, key, err, yard=None, note=""):
        limit = BAR if yard is None else max(BAR, YARD * yard)
        line = "%-34s hip %.2e  %sbound %.1e  %s" % (key, err, "" if yard is None else "(f32 oracle %.2e) " % yard, limit, note)
        self.lines.append(line)
        self.measured[key] = max(self.measured.get(key, 0.0), float(err))
        if not err <= limit:
            self.bad.append(line)
        if key in self.recorded and err > max(RATCHET * self.recorded[key], FLOOR):
            self.bad.append(line + "   [ratchet: %.1f x the recorded %.2e]" % (err / max(self.recorded[key], 1e-300), self.recorded[key]))

    def close(self, capsys):
        with capsys.disabled():
            print("\n[%s: HIP vs closed form / float64 oracle]\n" % self.title + "\n".join(self.lines))
        path = os.environ.get("SMALFIT_WRITE_COLOR_MEASURED")
        if path:
            doc = json.load(open(path)) if os.path.exists(path) else {}
            doc.update(self.measured)
            json.dump(doc, open(path, "w"), indent=1, sort_keys=True)
        assert not self.bad, "\n".join(self.bad)
        assert self.recorded, "tests/golden/hip_color_measured.json is missing: run this file with SMALFIT_WRITE_COLOR_MEASURED=<path> on a GPU box and commit the result"
        missing = [k for k in self.measured if k not in self.recorded]
        assert not missing, "not in tests/golden/hip_color_measured.json: %s" % missing


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """a device error ends the session: nothing more is started on a GPU that has just faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:
        pytest.exit("device error, stopping: %s" % exc, returncode=3)


# ---- anchors ---------------------------------------------------------------------------------------------------------
def _anchor_engine(faces, S, _cache={}):
    """one engine per topology and image size (tests/test_gpu_anchors.py::_engine, with room for FRAMES frames): `faces` over V_PAD
    free vertices, no blend shapes, rigid skinning"""
    key = (np.asarray(faces).tobytes(), S)
    if key not in _cache:
        base = synthetic.synthetic_model(seed=0, shape_family_id=1)
        w = np.zeros((V_PAD, 35), np.float32)
        w[:, 0] = 1.0
        jr = np.zeros((V_PAD, 35), np.float32)
        jr[np.arange(35), np.arange(35)] = 1.0
        md = model_io.SMALModelData(
            v_template=np.zeros((V_PAD, 3), np.float32), shapedirs=np.zeros((41, 3 * V_PAD), np.float32),
            posedirs=np.zeros((306, 3 * V_PAD), np.float32), J_regressor=jr, weights=w, parents=base.parents,
            faces=np.ascontiguousarray(faces, np.int32), left_inds=np.zeros(0, np.int64), right_inds=np.zeros(0, np.int64),
            center_inds=np.zeros(0, np.int64))
        _cache[key] = eng.Engine(eng.DeviceModel(md), FRAMES, S)
    return _cache[key]


def _pad(verts):
    """(frames, v, 3) -> (frames, V_PAD, 3) float32 on the device; no face references the added vertices"""
    out = np.zeros((len(verts), V_PAD, 3), np.float32)
    out[:, :, 2] = -50.0
    out[:, :verts.shape[1]] = verts
    return torch.from_numpy(out).cuda()


def _render(e, verts, colour):
    img = e.render_color(verts, colour)
    assert e.status() == 0
    assert img.dtype == torch.float32 and tuple(img.shape) == (verts.shape[0], 3, e.image_size, e.image_size)
    return img.cpu().numpy()


def _anchor_image(case, frames=None):
    v = case.verts if frames is None else case.verts[frames]
    return _render(_anchor_engine(case.faces, case.S), _pad(v), case.colour)


@pytest.mark.parametrize("name", sorted(ca.all_cases()))
def test_anchor(name, capsys):
    c = ca.all_cases()[name]
    img = _anchor_image(c)
    assert np.isfinite(img).all() and img.min() >= 0.0 and img.max() <= 1.0
    table = Table("anchor %s, %d^2, %d frame(s)" % (name, c.S, len(c.verts)))
    worst = 0.0
    for n, r, col, rgb in c.checks:
        got = img[n, :, r, col]
        if tuple(rgb) == ca.WHITE:
            assert (got == np.float32(1.0)).all(), (name, n, r, col, got)
        elif c.exact:
            want = np.float32(ca.AMBIENT) * np.asarray(c.colour, np.float32)
            assert want.dtype == np.float32 and np.abs(want - rgb).max() < 1e-7
            assert got.tobytes() == want.tobytes(), (name, n, r, col, got, want)
        else:
            assert (got < 1.0).all(), (name, n, r, col, got)
            worst = max(worst, float(np.abs(got.astype(np.float64) - rgb).max()))
    if not c.exact and any(tuple(rgb) != ca.WHITE for _, _, _, rgb in c.checks):
        table.add("anchor/%s" % name, worst, note="%d pixels" % len(c.checks))
    for n in c.white_frames:
        assert (img[n] == np.float32(1.0)).all(), (name, n, int((img[n] != 1.0).sum()))
    for n in c.covered_frames:
        assert (img[n] < 1.0).any(0).all(), (name, n)
    for wname, rows in sorted(c.wrong.items()):                 # the regime proof makes this follow from the bar; say it anyway
        gap = min(float(np.abs(img[n, :, r, col].astype(np.float64) - rgb).max()) for n, r, col, rgb in rows)
        table.lines.append("%-34s the device is at least %.2e from it" % ("  not %s" % wname, gap))
        assert gap > ca.REGIME - BAR, (name, wname, gap)
    if table.measured:
        table.close(capsys)


def test_red_channel_of_a_redless_colour_is_the_specular_term(capsys):
    c = ca.all_cases()["colour_argument"]
    assert c.colour[0] == 0.0 and len(set(c.colour)) == 3
    img = _anchor_image(c)
    table = Table("colour argument: the red channel alone")
    worst = max(abs(float(img[n, 0, r, col]) - ca.specular_term(c.verts[n], c.faces, 0, r, col, c.S)) for n, r, col, _ in c.checks)
    table.add("anchor/colour_argument/specular", worst)
    table.close(capsys)


def test_frames_one_after_three_and_twice_the_same():
    """each frame of a three-frame call has its own z-buffer, normals and image; a one-frame call on the same engine afterwards
    gives that frame's bits (nothing of the earlier call survives); two identical calls give identical bits (the z-buffer's
    64-bit minimum does not depend on the order of the faces' updates)"""
    for name in ("frames", "depth_order", "camera_plane"):
        c = ca.all_cases()[name]
        three = _anchor_image(c)
        assert np.array_equal(three, _anchor_image(c)), name
        for n in reversed(range(len(c.verts))):
            one = _anchor_image(c, [n])
            assert one.shape[0] == 1 and one[0].tobytes() == three[n].tobytes(), (name, n)
    c = ca.all_cases()["frames"]                        # the frames are different images to begin with
    img = _anchor_image(c)
    assert all((img[a] != img[b]).any() for a, b in ((0, 1), (0, 2), (1, 2)))


# ---- the whole mesh, per pixel -----------------------------------------------------------------------------------------
def _mesh_engine(mname, S, _cache={}):
    if _cache.get("model") != mname:                    # the inputs come model by model: let the previous one go
        _cache.clear()
        _cache.update(model=mname, dm=eng.DeviceModel(cc.model(mname)))
    if S not in _cache:
        _cache[S] = eng.Engine(_cache["dm"], FRAMES, S)
    return _cache[S]


def score(got, sc, table, key):
    """got (N,3,S,S) device image as numpy; sc: tests/color_cases.py::scoring.  Adds the decided pixels' deviation to the
    table and asserts the statements about undecided pixels and the background.  -> decided share per frame"""
    got = np.asarray(got)
    white = (got == np.float32(1.0)).all(1)
    covered = (got < 1.0).any(1)
    assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 1.0 and np.array_equal(covered, ~white)
    share, cov_o = cc.decided_share(sc)
    assert (share >= cc.DECIDED_SHARE).all(), share                        # a cap on what this test may leave out
    D = sc["decided"]
    sel = np.broadcast_to(D[:, None], got.shape)
    err = np.abs(got.astype(np.float64) - sc["f64"])[sel]
    yard = np.abs(sc["f32"] - sc["f64"])[sel]
    assert D.sum() > 0 and not white[D].any()                              # no decided pixel is exempt
    table.add(key, float(err.max()), yard=float(yard.max()),
              note="%d decided of %d covered pixels, share %s" % (D.sum(), cov_o.sum(), "/".join("%.3f" % s for s in share)))
    # undecided (and every other) pixel: white only if no face covers it by the strict margins, covered only if one does by the
    # relaxed ones; where none does, exactly 1.0
    assert not (white & sc["strict"]).any(), int((white & sc["strict"]).sum())
    assert not (covered & ~sc["relaxed"]).any(), int((covered & ~sc["relaxed"]).sum())
    assert (got[np.broadcast_to(~sc["relaxed"][:, None], got.shape)] == np.float32(1.0)).all()
    return share


@pytest.mark.parametrize("view,S", cc.INPUTS, ids=["%s-%d" % i for i in cc.INPUTS])
def test_whole_mesh_per_pixel(view, S, capsys):
    md, v = cc.view(view)
    e = _mesh_engine(cc.VIEWS[view][0], S)
    assert 1 <= len(v) <= FRAMES
    dev = torch.from_numpy(v.astype(np.float32)).cuda()
    got = _render(e, dev, cc.COLOUR)
    assert np.array_equal(got, _render(e, dev, cc.COLOUR))                   # 7774 faces' atomics in any order: the same bits
    table = Table("whole mesh %s, %d^2, %d frame(s)" % (view, S, len(v)))
    score(got, cc.scoring(view, S), table, "mesh/%s-%d/decided" % (view, S))
    table.close(capsys)


# ---- the collage -------------------------------------------------------------------------------------------------------
def _png(path):
    blob = open(path, "rb").read()
    w, h = struct.unpack(">II", blob[16:24])
    n = struct.unpack(">I", blob[33:37])[0]
    return np.frombuffer(zlib.decompress(blob[41:41 + n]), np.uint8).reshape(h, 1 + 3 * w)[:, 1:].reshape(h, w, 3)


def _bytes(render):
    """(N,3,S,S) device render -> (N,S,S,3) bytes as the collage stores them"""
    return (np.transpose(render.cpu().numpy(), (0, 2, 3, 1)) * 255.0).astype(np.uint8)


def _unmarked(proj, vis, S):
    """(N,S,S) True where SMALFitter._draw_joints leaves a pixel alone: the same landmarks drawn on a constant image"""
    from smalify_amd.smal_fitter.smal_fitter import SMALFitter
    blank = torch.full((proj.shape[0], 3, S, S), -1.0)
    return (SMALFitter._draw_joints(blank, proj, vis).numpy() == -1.0).all(1)


def test_fit_sequence_collage_carries_the_colour_render(golden, tmp_path):
    """panels 2 and 5 of st10_ep0.png against render_color of the fitter's final snapshot and of the snapshot turned about its
    centre"""
    from smalify_amd.smal_fitter.optimize_to_joints import fit_sequence
    from tests.test_gpu_dropin import _data
    md = synthetic.synthetic_model(seed=0, shape_family_id=1)
    data, N, S = _data(golden)
    names = ["frame_%02d.png" % i for i in range(N)]
    f = fit_sequence(data, names, md, (golden["pose_prec"], golden["pose_mean"], golden["pose_mask"]),
                     (golden["unity_prec"], golden["unity_mean"]), output_dir=str(tmp_path), window_size=2, iters_scale=0.02)
    assert f.e.status() == 0
    colour = [c / 255.0 for c in cfg.MESH_COLOR]
    verts, _, proj = f.snapshot()
    front = _bytes(f.e.render_color(verts, colour))
    rot_y180 = torch.tensor([[-1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1.0]], device=verts.device)
    centre = verts.mean(dim=1, keepdim=True)
    back = _bytes(f.e.render_color(((verts - centre) @ rot_y180.T).contiguous(), colour))
    keep = _unmarked(proj, f.visibility_full, S)
    assert (front != 255).any(-1).mean() > 0.01 and (back != 255).any(-1).mean() > 0.01 and keep.mean() > 0.5
    for i in range(N):
        rows = _png(os.path.join(str(tmp_path), "frame_%02d" % i, "st10_ep0.png"))
        assert rows.shape == (S, 5 * S, 3)
        assert np.array_equal(rows[:, 4 * S:5 * S], back[i]), i
        assert np.array_equal(rows[:, S:2 * S][keep[i]], front[i][keep[i]]), i
        assert (rows[:, S:2 * S][~keep[i]] != front[i][~keep[i]]).any()          # the marks are there


def test_generate_visualization_collage_carries_the_colour_render(golden, tmp_path):
    """SMALFitter.generate_visualization: panels 2 and 5 against render_color of the vertices it hands its renderer, where
    _draw_joints draws nothing (this collage marks the turned view as well)"""
    from smalify_amd.smal_fitter.optimize_to_joints import ImageExporter
    from tests.test_gpu_dropin import _make_fitter
    md = synthetic.synthetic_model(seed=0, shape_family_id=1)
    f = _make_fitter(golden, md, 2)
    N, S = f.num_images, f.image_size
    calls = []
    forward = f.renderer.forward

    def spy(vertices, points, faces, render_texture=False):
        out = forward(vertices, points, faces, render_texture=render_texture)
        calls.append((vertices.detach().clone(), out[1].detach().clone()))
        return out

    f.renderer.forward = spy
    exporter = ImageExporter(str(tmp_path), ["%04d.png" % i for i in range(N)])
    exporter.stage_id, exporter.epoch_name = 10, 0
    f.generate_visualization(exporter)
    f.renderer.forward = forward
    assert len(calls) == 2 * ((N + 1) // 2)              # per window: the view and the turned view
    colour = [c / 255.0 for c in cfg.MESH_COLOR]
    e = eng.Engine(f.smal_model.device_model, FRAMES, S)          # an engine of the test's own
    i = 0
    for (verts, proj), (rev_verts, rev_proj) in zip(calls[0::2], calls[1::2]):
        assert verts.shape[0] <= FRAMES
        vis = f.target_visibility[i:i + verts.shape[0]]
        for panel, v, p in ((1, verts, proj), (4, rev_verts, rev_proj)):
            want = _bytes(e.render_color(v.contiguous().float(), colour))
            keep = _unmarked(p, vis, S)
            assert (want != 255).any(-1).mean() > 0.01 and keep.mean() > 0.5
            for b in range(verts.shape[0]):
                rows = _png(os.path.join(str(tmp_path), "%04d" % (i + b), "st10_ep0.png"))
                assert np.array_equal(rows[:, panel * S:(panel + 1) * S][keep[b]], want[b][keep[b]]), (i + b, panel)
        i += verts.shape[0]
    assert i == N
