"""Host side of tests/value_forms.py (no GPU): every case is in the regime it names, float32 arithmetic alone (the float32
ORACLE, which is the reference's formula) stays inside the fixed bars at every fused case, and the host build of
smalfit_math.h (tests/host_math_shim.cpp) passes the per-magnitude sweeps the device is held to in
tests/test_gpu_value_forms.py, under the same bound."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import value_forms as vf
from tests.test_host_math import _p, shim  # noqa: F401  (the module-scoped fixture that builds the shim)


@pytest.fixture(scope="module")
def cases():
    return vf.fused_cases()


def _norms(case):
    return np.linalg.norm(case["params"]["joint_rotations"].astype(np.float64), axis=2)          # (M, 34)


def test_angle_cases_hold_the_magnitudes_they_name(cases):
    assert tuple(cases) == vf.FUSED_NAMES
    p = cases["rest"]["params"]
    for k in ("global_rotation", "joint_rotations", "betas", "log_beta_scales"):
        assert not p[k].any(), k
    n = _norms(cases["decades"])
    for j in range(34):
        assert np.allclose(n[:, j], vf.DECADES[j % 7], rtol=1e-6), j
    assert {vf.DECADES[j % 7] for j in range(34)} == set(vf.DECADES) and vf.DECADES[0] == 1e-7 and vf.DECADES[-1] == 0.1
    d = cases["decades"]["params"]["joint_rotations"]
    assert np.abs(d[0] / np.linalg.norm(d[0], axis=1, keepdims=True) - d[1] / np.linalg.norm(d[1], axis=1, keepdims=True)).min(0).max() > 0.01
    assert np.allclose(_norms(cases["band"]), 3e-4, rtol=1e-6)
    a = cases["axis"]["params"]["joint_rotations"].reshape(-1, 3)
    assert ((a == 0).sum(1) == 2).all()                                       # two components exactly zero ...
    assert np.signbit(a[a == 0]).any() and not np.signbit(a[a == 0]).all()    # ... some of them -0.0
    nz = a[a != 0]
    assert (nz > 0).any() and (nz < 0).any()
    for m in vf.AXIS_MAGNITUDES:
        assert np.isclose(np.abs(nz), m, rtol=1e-6).sum() >= 20, m
    assert all(np.isclose(np.abs(nz), m, rtol=1e-6).any() for m in (1e-5, 3e-4, 0.2, math.pi))
    n = _norms(cases["near_pi"])
    for j, want in vf.NEAR_PI.items():
        assert np.allclose(n[:, j], want, rtol=0, atol=5e-7), (j, n[:, j])
    assert n[0, 3] < math.pi - 9e-4 and n[0, 14] > math.pi + 9e-4             # float32 keeps the two sides of pi apart
    assert abs(np.linalg.norm(cases["near_pi"]["params"]["global_rotation"][1].astype(np.float64)) - math.pi) < 5e-7


def test_shape_and_depth_cases_are_where_they_claim(cases):
    p = cases["big_shape"]["params"]
    assert np.array_equal(p["log_beta_scales"], np.array(vf.BIG_SCALES, np.float32))
    assert (np.abs(p["betas"]) == 2.0).all() and (p["betas"] > 0).any() and (p["betas"] < 0).any()
    assert vf.keypoint_depths(cases["big_shape"]).min() >= 0.05
    zv = vf.keypoint_depths(cases["near_plane"])
    assert (cases["near_plane"]["params"]["trans"][:, 2] == np.float32(vf.NEAR_PLANE_Z)).all()
    assert (zv > 0).any() and (zv < 0).any() and np.abs(zv).min() >= 0.02, (zv.min(), zv.max(), np.abs(zv).min())
    assert vf.keypoint_depths(cases["rest"]).min() > 0.5                      # every other case stays well in front of the camera


def test_visibility_case_holds_every_row_kind(cases):
    c = cases["visibility"]
    vis, tj = c["vis"], c["tj"]
    assert (vis[0] != 0).all() and not vis[1].any() and (vis[2, :3] != 0).all() and not vis[2, 3:].any()
    assert sorted(set(vis.reshape(-1).tolist())) == [0.0, 0.5, 1.0, 2.0]
    hidden = tj[vis == 0]
    assert (hidden == -1.0).any() and (hidden == 1e4).any() and (hidden == -1e4).any()
    seen = tj[vis != 0]
    assert np.abs(seen).max() > 900 and np.abs(seen).max() < 1200
    same = cases["identical"]["params"]
    for k in ("global_rotation", "joint_rotations", "trans"):
        assert np.array_equal(same[k][0], same[k][1]) and not np.array_equal(same[k][1], same[k][2])
    assert cases["one_frame"]["params"]["joint_rotations"].shape == (1, 34, 3) and cases["one_frame"]["tj"].shape == (1, 25, 2)


def test_limit_case_sits_on_and_one_ulp_off_the_table(cases):
    c = cases["limits"]
    x, kinds, lo, hi = vf.limit_placement()
    got = c["params"]["joint_rotations"]
    assert c["weights"][4] == 100.0 and np.array_equal(c["limits"][0], lo)
    for i, name in enumerate(vf.LIMIT_KINDS):
        sel = kinds == i
        assert sel.sum() >= 20, name
        g, l, h = got[sel], np.broadcast_to(lo, got.shape)[sel], np.broadcast_to(hi, got.shape)[sel]
        if name == "at_hi":
            assert (g == h).all()
        elif name == "at_lo":
            assert (g == l).all()
        elif name == "hi_in":
            assert (g < h).all() and (np.nextafter(g, np.float32(np.inf)) == h).all()
        elif name == "hi_out":
            assert (g > h).all() and (np.nextafter(g, np.float32(-np.inf)) == h).all()
        elif name == "lo_in":
            assert (g > l).all() and (np.nextafter(g, np.float32(-np.inf)) == l).all()
        elif name == "lo_out":
            assert (g < l).all() and (np.nextafter(g, np.float32(np.inf)) == l).all()
        elif name == "far_out":
            assert (np.isclose(g - h, 0.5, atol=1e-6) | np.isclose(l - g, 0.5, atol=1e-6)).all()
            assert (g > h).any() and (g < l).any()
        else:
            assert ((g > l) & (g < h)).all()
    # the correction that turns autograd's tie-splitting into the kernel's convention touches exactly the ties
    corr = vf.limit_tie_correction(c)
    assert np.array_equal(corr != 0, (kinds == 0) | (kinds == 1))
    assert np.allclose(corr[0][kinds[0] == 0], 0.5 * 100.0 / (102 * 2)) and np.allclose(corr[2][kinds[2] == 1], -0.5 * 100.0 / (102 * 1))
    # and the oracle's own gradient of the limit term alone is that half slope there
    only = dict(c, name="limits/only", weights=np.array([0, 0, 0, 0, 100.0, 0]), w_temp=0.0)
    _, g = vf.oracle_eval(only)
    assert np.abs(g["joint_rotations"][(kinds == 0) | (kinds == 1)]).max() == 0.0
    assert np.allclose(g["joint_rotations"][0][kinds[0] == 3], 100.0 / (102 * 2))


def test_float32_oracle_alone_stays_inside_the_fixed_bars(cases, capsys):
    """the fixed bars (terms 1e-4, tensor gradients 5e-4) must leave room for float32 arithmetic at every fused case: a case the
    reference's own formula cannot pass in float32 would only ever pass through the yardstick"""
    lines, bad = [], []
    for name, c in cases.items():
        t64, g64 = vf.oracle_eval(c)
        t32, g32 = vf.oracle_eval(c, torch.float32)
        for q, (err, kind) in vf.fused_deviations(t32, g32, t64, g64).items():
            if "[" in q:
                continue
            lines.append("%-18s %-24s f32 oracle %.2e" % (name, q, err))
            if err > vf.BAR[kind]:
                bad.append(lines[-1])
    with capsys.disabled():
        print("\n[value forms: float32 oracle vs float64 oracle]\n" + "\n".join(lines))
    assert not bad, "\n".join(bad)


def test_weight_and_frame_cases_have_exact_zeros_in_the_oracle(cases):
    for col, slots in vf.WEIGHT_SLOTS.items():
        t, _ = vf.oracle_eval(cases["weights_off/" + col])
        for s in slots:
            assert t[vf.LOSS_NAMES.index(s)] == 0.0
        assert sum(t != 0) == 7 - len(slots)
    t, g = vf.oracle_eval(cases["weights_off/all"])
    assert not t.any() and not any(v.any() for v in g.values())
    t, _ = vf.oracle_eval(cases["one_frame"])
    assert not t[5:8].any() and t[0] > 0


# ---- the host build of smalfit_math.h under the device's bounds -------------------------------------------------------
def _hm_rodrigues(shim, th, G):  # noqa: F811
    n = len(th)
    R, dth = np.zeros((n, 9), np.float32), np.zeros((n, 3), np.float32)
    shim.hm_rodrigues(n, _p(np.ascontiguousarray(th)), _p(np.ascontiguousarray(G.reshape(n, 9))), _p(R), _p(dth))
    return R, dth


def test_rodrigues_host_per_magnitude(shim, capsys):  # noqa: F811
    lines, bad = [], []
    for m, kind, th, G in vf.rodrigues_sweep():
        R, dth = _hm_rodrigues(shim, th, G)
        assert np.isfinite(R).all() and np.isfinite(dth).all(), (m, kind)
        (fwd, bwd, skew), (yf, yb, ys), d64 = vf.rodrigues_deviations(R, dth, th, G)
        lines.append("|theta| %-8s %-6s fwd max-abs %.2e (f32 oracle %.2e)  sin(a) r rel-L2 %.2e (f32 oracle %.2e)  adjoint rel-L2 %.2e (f32 oracle %.2e)"
                     % (vf.magnitude_label(m), kind, fwd, yf, skew, ys, bwd, yb))
        if fwd > vf.bound("rodrigues_fwd", yf) or bwd > vf.bound("rodrigues_bwd", yb) or skew > vf.bound("rodrigues_skew", ys):
            bad.append(lines[-1])
        if m == 0.0:
            assert np.abs(dth - d64).max() < 1e-5                    # theta = 0: the generators, finite
    for count in vf.RODRIGUES_COUNTS:
        th, G = vf.rodrigues_count_case(count)
        R, dth = _hm_rodrigues(shim, th, G)
        (fwd, bwd, skew), (yf, yb, ys), _ = vf.rodrigues_deviations(R, dth, th, G)
        assert fwd <= vf.bound("rodrigues_fwd", yf) and bwd <= vf.bound("rodrigues_bwd", yb) and skew <= vf.bound("rodrigues_skew", ys), (count, fwd, bwd, skew)
    with capsys.disabled():
        print("\n[value forms: host build of rodrigues_fwd / _bwd vs float64 oracle]\n" + "\n".join(lines))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("scale", vf.CHAIN_SCALES)
def test_global_rigid_host_at_value_edges(shim, synth_model, scale):  # noqa: F811
    parents = np.ascontiguousarray(synth_model.parents, np.int32)
    for count in (1, 65):
        c = vf.chain_case(count, scale)
        newJ, A = np.zeros((count, 35, 3), np.float32), np.zeros((count, 35, 4, 4), np.float32)
        ls = None if c["ls"] is None else _p(c["ls"])
        shim.hm_global_rigid(count, _p(c["Rs"]), _p(c["Js"]), _p(parents), ls, _p(newJ), _p(A))
        dRs, dJs, dls = np.zeros_like(c["Rs"]), np.zeros_like(c["Js"]), np.zeros((count, 6), np.float32)
        shim.hm_global_rigid_bwd(count, _p(c["Rs"]), _p(c["Js"]), _p(parents), ls, _p(c["dnewJ"]), _p(c["dA"]), _p(dRs), _p(dJs), _p(dls))
        r64, r32 = vf.chain_oracle(c, parents), vf.chain_oracle(c, parents, torch.float32)
        got = {"newJ": newJ, "A": A, "dRs": dRs, "dJs": dJs, "dls": dls}
        for k in r64:
            err, y = vf.rel(got[k], r64[k]), vf.rel(r32[k], r64[k])
            assert err <= vf.bound("chain", y), (count, scale, k, err, y)
        assert (A[:, :, 3, :] == np.array([0, 0, 0, 1.0], np.float32)).all()


def test_camera_host_at_every_depth(shim):  # noqa: F811
    pts, g, which = vf.project_case(3, 300)
    n = pts.shape[0] * pts.shape[1]
    half = 0.5 * (vf.S - 1)
    # proj = half (1 - ndc), (row, col) = (y, x): the upstream gradient of (x_ndc, y_ndc) is -half (g_col, g_row)
    g2 = np.ascontiguousarray(-half * g.reshape(n, 2)[:, ::-1], np.float32)
    ndc, g3 = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    shim.hm_camera(n, _p(pts.reshape(n, 3)), _p(g2), _p(ndc), _p(g3))
    proj = np.stack([half * (1.0 - ndc[:, 1].astype(np.float64)), half * (1.0 - ndc[:, 0].astype(np.float64))], 1)
    p64, d64 = vf.project_oracle(pts, g)
    p32, d32 = vf.project_oracle(pts, g, torch.float32)
    for k, zv in enumerate(vf.PROJECT_DEPTHS):
        sel = which == k
        assert np.allclose(ndc[sel, 2], zv, atol=1e-6)
        for got, r64, r32 in ((proj, p64.reshape(n, 2), p32.reshape(n, 2)), (g3, d64.reshape(n, 3), d32.reshape(n, 3))):
            err, y = vf.rel(got[sel], r64[sel]), vf.rel(r32[sel], r64[sel])
            assert err <= vf.bound("camera", y), (zv, err, y)


@pytest.mark.parametrize("t", vf.ADAM_STEPS)
def test_adam_host_at_value_edges(shim, t):  # noqa: F811
    f = C.c_float
    shim.hm_adam.argtypes = [C.c_int] + [C.c_void_p] * 4 + [f] * 4 + [C.c_int, C.c_int, C.c_void_p]
    lr, b1, b2, eps = (float(np.float32(x)) for x in vf.ADAM_HYPER)
    bias = np.zeros(2, np.float32)
    for count in vf.ADAM_COUNTS:
        p, g, m, v, zero = vf.adam_case(count, t)
        assert (g == 0).any() == (count > 6) and (count < 7 or ((np.abs(g) == np.float32(1e-20)).any() and (np.abs(g) == np.float32(1e15)).any()))
        p0 = p.copy()
        want = vf.adam_reference(p, g, m, v, t)
        shim.hm_adam(count, _p(p), _p(g), _p(m), _p(v), lr, b1, b2, eps, t, 0, _p(bias))
        for got, ref in zip((p, m, v), want):
            assert np.isfinite(got).all() and vf.rel(got, ref) < vf.BAR["adam"], (count, t)
        assert np.array_equal(p[zero].view(np.uint32), p0[zero].view(np.uint32))      # g = 0 on zero moments: the parameter stays
