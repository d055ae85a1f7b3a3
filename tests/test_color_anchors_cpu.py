"""The oracle's hard-Phong restatement against the closed forms of tests/color_anchors.py; the proof that every named wrong
answer of those cases lies at least ten device bars from the right one at every pixel where it is asserted; and the
condition under which tests/test_gpu_color.py may score the whole mesh per pixel (at least 97 % of every input's covered
pixels decided).  No GPU."""
import numpy as np
import pytest

from oracle import smal_oracle as so
from tests import color_anchors as ca
from tests import color_cases as cc

CASES = sorted(ca.all_cases())


def _render(case, dtype=np.float64):
    return so.hard_phong_render(case.verts, case.faces, case.S, case.colour, dtype=dtype)


def test_every_case_asserts_something():
    cases = ca.all_cases()
    assert len(cases) == len(ca.CASES)
    for c in cases.values():
        assert c.checks or c.white_frames, c.name
        asserted = {(n, r, col) for n, r, col, _ in c.checks}
        for name, rows in c.wrong.items():
            assert rows and {(n, r, col) for n, r, col, _ in rows} <= asserted, (c.name, name)
    named = {k for c in cases.values() for k in c.wrong}
    assert {"shininess_32", "light_at_camera", "perspective_correct", "unweighted_normals", "flat_normals", "other_face"} <= named
    assert len([k for k in named if k.startswith("weights_")]) == 5


@pytest.mark.parametrize("name", CASES)
def test_oracle_meets_the_anchor(name):
    c = ca.all_cases()[name]
    img = _render(c)
    for n, r, col, rgb in c.checks:
        assert np.abs(img[n, :, r, col] - rgb).max() < 1e-9, (name, n, r, col, img[n, :, r, col], rgb)
    for n in c.white_frames:
        assert (img[n] == 1.0).all(), (name, n)
    for n in c.covered_frames:
        assert (img[n] < 1.0).any(0).all(), (name, n)
    for n, r, col, rgb in c.checks:
        if tuple(rgb) == ca.WHITE:
            assert (img[n, :, r, col] == 1.0).all()


@pytest.mark.parametrize("name", [n for n in CASES if n != "depth_tie"])
def test_oracle_in_float32_stays_within_the_device_bar(name):
    """the float32 mode is the same arithmetic: on the anchors it stays within the bar the device is held to.  (Not the depth
    tie: the oracle sums three weighted depths per pixel, and in float32 rounding decides which of two equal sums is smaller;
    the kernels evaluate the depth as a plane whose coefficients are equal for the two faces, test_depth_tie_is_a_tie)"""
    c = ca.all_cases()[name]
    img = _render(c, np.float32)
    for n, r, col, rgb in c.checks:
        assert np.abs(img[n, :, r, col] - rgb).max() < ca.DEVICE_BAR, (name, n, r, col, img[n, :, r, col], rgb)
    for n in c.white_frames:
        assert (img[n] == 1.0).all(), (name, n)


@pytest.mark.parametrize("name", [n for n in CASES if ca.all_cases()[n].wrong])
def test_named_wrong_answers_are_ten_bars_away(name, capsys):
    c = ca.all_cases()[name]
    right = {(n, r, col): rgb for n, r, col, rgb in c.checks}
    lines = []
    for wname, rows in sorted(c.wrong.items()):
        gaps = [np.abs(rgb - right[(n, r, col)]).max() for n, r, col, rgb in rows]
        lines.append("%-14s %-20s %d pixels, smallest gap %.2e" % (name, wname, len(gaps), min(gaps)))
        assert min(gaps) >= ca.REGIME, lines[-1]
    with capsys.disabled():
        print("\n" + "\n".join(lines))


def test_depth_tie_is_a_tie():
    """case_depth_tie: mirrored coordinates are equal up to sign in float32 too, and the area is large enough for + kEpsilon to
    vanish there -- the two faces' records differ in signs only"""
    c = ca.all_cases()["depth_tie"]
    v = c.verts[0].astype(np.float32)
    assert np.array_equal(v[3:], v[:3] * np.array([-1, 1, 1], np.float32))
    zv = np.float32(so.CAM_DIST) - v[:, 2]
    iz = np.float32(1.7320508075688772) / zv
    xn, yn = -v[:, 0] * iz, v[:, 1] * iz
    assert np.array_equal(xn[3:], -xn[:3]) and np.array_equal(yn[3:], yn[:3]) and len(set(zv.tolist())) == 1
    area = (xn[2] - xn[0]) * (yn[1] - yn[0]) - (yn[2] - yn[0]) * (xn[1] - xn[0])
    assert area > 0.25 and np.float32(area + np.float32(1e-8)) == area and np.float32(-area + np.float32(1e-8)) == -area


def test_whole_mesh_front_view_is_the_visualisation_tests_mesh():
    """... rounded to float32, which is what the device is given"""
    from tests.test_visualisation_cpu import _posed_mesh
    _, _, verts = _posed_mesh(3)
    assert np.array_equal(cc.view("front")[1], verts.numpy().astype(np.float32).astype(np.float64))
    md, v = cc.view("valence_front")
    from tests import model_forms as mf
    f = mf.facts(md)
    assert f["valence_max"] == 40 and len(f["isolated"]) == 4


@pytest.mark.parametrize("view,S", cc.INPUTS, ids=["%s-%d" % i for i in cc.INPUTS])
def test_whole_mesh_inputs_are_decided(view, S, capsys):
    md, v = cc.view(view)
    w = so.hard_phong_winners(v, np.asarray(md.faces), S)
    share, covered = cc.decided_share(w)
    with capsys.disabled():
        print("\n%-14s %3d^2: covered %s, decided share %s" % (view, S, covered.reshape(len(v), -1).sum(1).tolist(), np.round(share, 4).tolist()))
    assert (covered.reshape(len(v), -1).sum(1) >= 5).all()
    assert (share >= cc.DECIDED_SHARE).all(), share
    # the sets are nested, and the exact set's winner is the image's: covered there, white elsewhere
    assert not (w["strict"] & ~w["exact"]).any() and not (w["exact"] & ~w["relaxed"]).any()
    img = so.hard_phong_render(v, np.asarray(md.faces), S, cc.COLOUR)
    assert np.array_equal((img < 1.0).any(1), w["exact"])
    assert (w["decided"] <= w["strict"]).all()
