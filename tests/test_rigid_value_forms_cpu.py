"""CPU: the rigid pre-alignment's shared arithmetic (the host shims tests/host_rigid_align.py and tests/host_rigid_trim.py, which
compile rigid_align_math.h) and the host fold of fitter_3d.trainer away from the blob at the origin: the cases of
tests/rigid_value_forms.py.  What is proved here without a GPU: the scale window and what lies beyond it, the rank test's new
right-hand side, the admission of every place and template case the GPU file runs, the promise on non-finite coordinates, and
exp / log of a rotation at every branch.  The worst fold figure is recorded in tests/golden/hip_rigid_value_forms_measured.json
(cpu/*) with SMALFIT_WRITE_RIGID_VALUE_FORMS_MEASURED=<path>."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from smalify_amd.fitter_3d import trainer
from tests import host_rigid_align as hr
from tests import host_rigid_trim as ht
from tests import rigid_align_cases as rc
from tests import rigid_trim_cases as tc
from tests import rigid_value_forms as vf

HERE = os.path.dirname(os.path.abspath(__file__))
MEASURED = os.path.join(HERE, "golden", "hip_rigid_value_forms_measured.json")
WRITE_ENV = "SMALFIT_WRITE_RIGID_VALUE_FORMS_MEASURED"
RECOVERY_ANGLE_CAP = 1e-3       # rad: tests/test_gpu_rigid_align.py
I = vf.SCALE_ITERATIONS_CPU


def _scaled(a, k):
    return vf.ldexp32(a, k)


# ---- A: scale ---------------------------------------------------------------------------------------------------------------------
_UNIT = {}


def _unit(n, wp, wv):
    if (n, wp, wv) not in _UNIT:
        x, p = vf.batch()
        _UNIT[n, wp, wv] = vf.shim_align(x[n], p[n], I, wp, wv)
    return _UNIT[n, wp, wv]


def test_the_window_holds_every_scale_of_the_gpu_test_and_the_old_right_hand_side_did_not_reach_its_edge():
    x, p = vf.batch()
    xt, pt, kp, kv = vf.partial()
    for wp, wv in vf.WEIGHTS:
        for lo, hi in [vf.scale_window(x[n], p[n], wp, wv) for n in range(3)] + [vf.scale_window(xt, pt, wp, wv, (kp, kv))]:
            print(wp, wv, lo, hi)
            assert lo <= min(vf.SCALES) and max(vf.SCALES) <= hi
            assert vf.OUTSIDE[0] < lo and hi < vf.OUTSIDE[1]
    lo, hi = vf.scale_window(x[0], p[0])
    olo, ohi = vf.old_rank_window(x[0], p[0])
    print("window", lo, hi, "the product under the old root", olo, ohi)
    # the product of degree 4 left the normal range about half way to the edge of everything else
    assert ohi < vf.RANK_RHS_OVERFLOWED_AT <= hi and ohi < hi // 2 + 4


@pytest.mark.parametrize("k", vf.SCALES)
@pytest.mark.parametrize("wp,wv", vf.WEIGHTS)
def test_untrimmed_batch_scales_bit_for_bit(wp, wv, k):
    x, p = vf.batch()
    for n in range(3):
        s = vf.shim_align(_scaled(x[n], k), _scaled(p[n], k), I, wp, wv)
        assert vf.scaled_equal(_unit(n, wp, wv), s, k) == [], (n, k)


@pytest.mark.parametrize("k", vf.SCALES)
@pytest.mark.parametrize("wp,wv", vf.WEIGHTS)
def test_trimmed_partial_case_scales_bit_for_bit(wp, wv, k):
    x, p, kp, kv = vf.partial()
    u = vf.shim_align(x, p, I, wp, wv, (kp, kv))
    s = vf.shim_align(_scaled(x, k), _scaled(p, k), I, wp, wv, (kp, kv))
    assert vf.scaled_equal(u, s, k) == []
    assert int(u["vert_kept"].sum()) == (vf.K * kv if wv > 0 else vf.K * len(x) * vf.BYTE_SENTINEL)


def test_both_edges_of_the_window_scale_bit_for_bit_and_one_step_outside_does_not():
    x, p = vf.batch()
    lo, hi = vf.scale_window(x[0], p[0])
    u = _unit(0, 1.0, 1.0)
    for k in (lo, hi):
        assert vf.scaled_equal(u, vf.shim_align(_scaled(x[0], k), _scaled(p[0], k), I), k) == [], k
    V = x.shape[1]
    # far below: every d^2 underflows to 0 -- every score 0, every match index 0 (the first of equal d^2), H = 0: no rotation is
    # determined, every solve keeps its start's
    below = vf.shim_align(_scaled(x[0], vf.OUTSIDE[0]), _scaled(p[0], vf.OUTSIDE[0]), I)
    assert np.all(below["scores"] == 0) and np.all(below["vert_nn"] == 0) and np.all(below["kept_rotation"] == I)
    # far above: d^2 beyond a 2^-6 of the extent is +inf, `<` never holds there: no match (-1), and every cost is +inf
    above = vf.shim_align(_scaled(x[0], vf.OUTSIDE[1]), _scaled(p[0], vf.OUTSIDE[1]), I)
    assert np.all(np.isposinf(above["scores"])) and np.any(above["vert_nn"] == -1) and np.any(above["point_nn"] == -1)
    assert np.all(above["kept_rotation"] == I) and above["best"] == 0
    for o in (below, above):
        assert np.array_equal(o["transforms"].reshape(-1, 3, 4)[:, :, :3], hr.cube_rotations()), "the starts' rotations, bit for bit"
        assert vf.promise_violations(o, V, V, vf.K, I, False) == []


def test_the_rank_test_at_the_scales_where_the_old_product_left_the_range():
    """k = 33: sum w |x|^2 sum w |p|^2 is +inf, and under one root nothing was ever `determined` and no start rotated.  With a root
    of each sum start 5 rotates as it does at scale 1.  k = -40: the product is 0 and collinear points passed; they are refused"""
    c = rc.RECOVERY_CASES["cube5_skew15"]
    x, p = c["x"], c["p"]
    u = vf.shim_align(x, p, 30, starts=hr.cube_rotations()[5:6])
    assert u["kept_rotation"][0] == 0 and rc.rotation_angle(vf.split(u["transforms"][0])[0], c["R"]) < RECOVERY_ANGLE_CAP
    k = vf.RANK_RHS_OVERFLOWED_AT
    s = vf.shim_align(_scaled(x, k), _scaled(p, k), 30, starts=hr.cube_rotations()[5:6])
    assert s["kept_rotation"][0] == 0 and vf.scaled_equal(u, s, k) == []
    # the two sides of the test, straight from the solve: the right-hand side is finite and the scaled bits of scale 1
    M = hr.moments_of_pairs(x[:40], p[:40], np.full(40, 1.0 / 40), hr.means(x), hr.means(p))
    deg = np.array([0] + [1] * 6 + [2] * 12)
    prev = hr.start_transform(np.eye(3), np.zeros(3), np.zeros(3))
    _, kept1, gap1, scale1 = hr.solve(M, hr.means(x), hr.means(p), prev)
    for kk in (k + 1, 45, 60, -40, -60):
        Mk = np.array([vf.ldexp32(M[i], int(deg[i]) * kk) for i in range(19)], np.float32)
        _, kept, gap, scale = hr.solve(Mk, _scaled(hr.means(x), kk), _scaled(hr.means(p), kk), prev)
        assert kept == kept1 == 0, kk
        assert np.float32(scale) == vf.ldexp32(scale1, 2 * kk) and np.float32(gap) == vf.ldexp32(gap1, 2 * kk), kk
        assert float(M[16]) * float(M[17]) * 2.0 ** (4 * kk) > vf.FLT_MAX or float(M[16]) * float(M[17]) * 2.0 ** (4 * kk) < vf.FLT_MIN
    xb, line = rc.lopsided_blob(), rc.collinear_points()
    for kk in (0, vf.RANK_RHS_UNDERFLOWED_AT, k):
        o = vf.shim_align(_scaled(xb, kk), _scaled(line, kk), 4, starts=hr.cube_rotations()[5:7])
        assert np.all(o["kept_rotation"] == 4), (kk, o["kept_rotation"])
        assert np.array_equal(o["transforms"].reshape(-1, 3, 4)[:, :, :3], hr.cube_rotations()[5:7])


def test_no_existing_case_changes_its_determined_decision():
    """sqrt(a) sqrt(b) against sqrt(a b) in float32 differ by an ulp or two of a right-hand side that is 1e-5 of the left where a
    rotation is determined, and face a left-hand side of rounding alone where it is not: over every start and iteration of every
    recovery and rank-deficient case the two sides are never within a factor of 8 of each other"""
    sets = [(c["x"], c["p"], c["w_point"], c["w_vert"]) for c in rc.RECOVERY_CASES.values()]
    sets += [(rc.lopsided_blob(), rc.coincident_points(), 1.0, 1.0), (rc.lopsided_blob(), rc.collinear_points(), 1.0, 1.0)]
    closest = np.inf
    for x, p, wp, wv in sets:
        cX, cP = hr.means(x), hr.means(p)
        for k in range(0, 24, 5):
            T = hr.start_transform(hr.cube_rotation(k), cX, cP)
            for _ in range(4):
                r = hr.iterate(x, p, T, wp, wv)
                iv, ip = r["idx_v"], r["idx_p"]
                xs = np.concatenate(([x] if wv > 0 else []) + ([x[ip]] if wp > 0 else []))
                ps = np.concatenate(([p[iv]] if wv > 0 else []) + ([p] if wp > 0 else []))
                w = np.concatenate(([np.full(len(x), wv / len(x))] if wv > 0 else []) + ([np.full(len(p), wp / len(p))] if wp > 0 else []))
                _, kept, gap, scale = hr.solve(hr.moments_of_pairs(xs, ps, w, cX, cP), cX, cP, T)
                rhs = 1e-5 * scale
                assert kept == r["kept"]
                if rhs > 0:
                    closest = min(closest, max(gap / rhs, rhs / max(gap, 1e-300)) if gap > 0 else np.inf)
                T = r["T"]
    print("closest ratio of the two sides", closest)
    assert closest > 8.0


# ---- B: place ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("o,trimmed", vf.PLACE_CASES, ids=vf.PLACE_IDS)
def test_place_cases_are_admitted_and_the_shim_stays_under_the_caps(o, trimmed):
    c, ref = vf.place_case(o, trimmed), vf.place_reference(o, trimmed)
    b = ref["best"]
    admission = rc.rotation_angle(ref["R"][b], c["R"])
    gap, blur = vf.winner_margin(c, ref)
    print("restatement: best", b, "off R* by", admission, "gap", gap, "blur", blur)
    assert admission < vf.PLACE_ADMISSION and gap > blur and ref["kept"][b] == 0
    sh = vf.shim_align(c["x"], c["p"], vf.PLACE_ITERATIONS, keep=c["keep"])
    angle, pos = vf.place_figures(c, ref, sh["best"], sh["best_transform"])
    print("shim: best", sh["best"], "angle", angle, "position", pos, "ulp(L)", "score", sh["scores"][sh["best"]], "float64", ref["scores"][b])
    assert angle < RECOVERY_ANGLE_CAP and pos < vf.POSITION_CAP_ULPS
    # `best`: the restatement's, or a start that ended at the same rotation and the same score up to the blur (two starts that reach
    # one fixed point: in float64 the lower score is rounding, in float32 the bits are equal and the lower index wins)
    assert rc.rotation_angle(ref["R"][sh["best"]], ref["R"][b]) < 1e-6 and abs(ref["scores"][sh["best"]] - ref["scores"][b]) < blur


@pytest.mark.parametrize("o,trimmed", vf.PLACE_NOT_ADMITTED)
def test_the_place_cases_left_out_are_undecided_in_float32(o, trimmed):
    c, ref = vf.place_case(o, trimmed), vf.place_reference(o, trimmed)
    gap, blur = vf.winner_margin(c, ref)
    print(o, "gap", gap, "blur", blur)
    assert 0 < gap < blur
    # start by start the shim still follows the restatement where float32 resolves the lattice (o = 1024)
    if o == 1024:
        sh = vf.shim_align(c["x"], c["p"], vf.PLACE_ITERATIONS, keep=c["keep"], starts=hr.cube_rotations()[[5, 22]])
        for j, k in enumerate((5, 22)):
            assert rc.rotation_angle(vf.split(sh["transforms"][j])[0], ref["R"][k]) < 1e-5


# ---- C: non-finite coordinates ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trimmed", (False, True), ids=("untrimmed", "trimmed"))
@pytest.mark.parametrize("where,value", vf.NONFINITE, ids=vf.NONFINITE_IDS)
def test_a_non_finite_coordinate_stays_in_bounds_on_the_shims(where, value, trimmed):
    x, p = vf.batch()
    xb, pb = vf.poisoned(x, p, where, value)
    V, S = x.shape[1], p.shape[1]
    keep = (tc.KEEP_POINT, tc.KEEP_VERT) if trimmed else None
    o = vf.shim_align(xb[1], pb[1], vf.NONFINITE_ITERATIONS, keep=keep)
    assert vf.promise_violations(o, V, S, vf.K, vf.NONFINITE_ITERATIONS, trimmed) == []
    # on the shim (the header leaves the values open; the device is held to the promise alone): the means are poisoned, no
    # transform is finite, no query has a match, the cost is +inf; trimmed, no query has a key, nothing is kept and the cost is 0,
    # as the header says of a mesh without keys
    assert not np.isfinite(o["transforms"].reshape(-1, 3, 4)[:, :, 3]).all(-1).any()
    assert np.all(o["vert_nn"] == -1) and np.all(o["point_nn"] == -1)
    assert np.all(o["scores"] == 0) if trimmed else np.all(np.isposinf(o["scores"]))
    if trimmed:
        assert not o["vert_kept"].any() and not o["point_kept"].any() and np.all(o["trim_d2"] == 0)


def test_one_shim_iteration_on_a_poisoned_mesh_leaves_its_guard_rows_alone():
    x, p = vf.batch()
    lib = hr.load()
    ht.load()
    for where, value in vf.NONFINITE:
        xb, pb = vf.poisoned(x, p, where, value)
        xs, ps = np.ascontiguousarray(xb[1]), np.ascontiguousarray(pb[1])
        V, S, G = len(xs), len(ps), vf.GUARD
        T = hr.start_transform(np.eye(3), hr.means(xs), hr.means(ps))
        iv, ip = np.full(V + 2 * G, vf.SENTINEL, np.int32), np.full(S + 2 * G, vf.SENTINEL, np.int32)
        kv, kp = np.full(V + 2 * G, vf.BYTE_SENTINEL, np.uint8), np.full(S + 2 * G, vf.BYTE_SENTINEL, np.uint8)
        out, cost, d2 = np.full(12 + 2 * G, vf.SENTINEL, np.float32), C.c_float(), np.full(2 + 2 * G, vf.SENTINEL, np.float32)
        lib.hra_iterate(V, xs.ctypes.data, S, ps.ctypes.data, T.ctypes.data, 1.0, 1.0, out[G:].ctypes.data, C.addressof(cost),
                        iv[G:].ctypes.data, ip[G:].ctypes.data)
        ht.load().hrt_iterate(V, xs.ctypes.data, S, ps.ctypes.data, T.ctypes.data, 1.0, 1.0, tc.KEEP_POINT, tc.KEEP_VERT, out[G:].ctypes.data,
                              C.addressof(cost), iv[G:].ctypes.data, ip[G:].ctypes.data, kv[G:].ctypes.data, kp[G:].ctypes.data,
                              d2[G:].ctypes.data)
        for buf, sentinel in ((iv, vf.SENTINEL), (ip, vf.SENTINEL), (kv, vf.BYTE_SENTINEL), (kp, vf.BYTE_SENTINEL), (out, vf.SENTINEL),
                              (d2, vf.SENTINEL)):
            assert np.all(buf[:G] == sentinel) and np.all(buf[-G:] == sentinel)
        assert np.all(iv[G:-G] == -1) and np.all(ip[G:-G] == -1) and not kv[G:-G].any() and not kp[G:-G].any()


# ---- D: the template --------------------------------------------------------------------------------------------------------------
def test_the_template_case_is_admitted():
    c = vf.template_case()
    assert c["x"].shape == (3889, 3) and c["p"].shape == (3889, 3) and len(c["x"]) > 3 * 1024      # four staged chunks
    ref = vf.template_reference()
    b = ref["best"]
    print("best", b, "score", ref["scores"][b], "off R* by", rc.rotation_angle(ref["R"][b], c["R"]))
    # the mirror image of the rest pose is not a rotation of it: a start that ends at R* wins, at a score of float64 rounding
    assert rc.rotation_angle(ref["R"][b], c["R"]) < rc.RECOVERY_ADMISSION and ref["scores"][b] < 1e-12 and ref["kept"][b] == 0
    assert np.abs(ref["t"][b] - c["t"]).max() < 1e-6 * c["extent"]
    # every start that ends within the cap of R* ends at the same place, the true start among them; the rest are far worse
    near = np.array([rc.rotation_angle(R, c["R"]) < RECOVERY_ANGLE_CAP for R in ref["R"]])
    assert near[vf.TEMPLATE_TRUE_START] and ref["scores"][near].max() < 1e-12 and ref["scores"][~near].min() > 1e-4


def test_the_trimmed_template_case_is_admitted():
    """the points are drawn on the faces of the partial target: the restatement ends a sampling error from R*, inside
    TEMPLATE_TRIM_ADMISSION, and its winner is decided: the best start that ends elsewhere lies above it by far more than float32
    at this place can blur"""
    c, ref = vf.template_partial(), vf.template_reference(trimmed=True)
    b = ref["best"]
    off = rc.rotation_angle(ref["R"][b], c["R"])
    gap, blur = vf.template_margin(ref, c["ulp"])
    order = np.argsort(ref["scores"])
    print("best", b, "score", ref["scores"][b], "off R* by", off, "gap", gap, "blur", blur, "next", order[1], ref["scores"][order[1]])
    assert b == vf.TEMPLATE_TRIM_TRUE_START and off < vf.TEMPLATE_TRIM_ADMISSION and ref["kept"][b] == 0
    assert gap > 10 * blur
    assert np.abs(ref["t"][b] - c["t"]).max() < vf.TEMPLATE_TRIM_ADMISSION * c["extent"]


def test_the_template_scans_of_the_shim_are_the_definition():
    """3889 records are four staged chunks on the device; on the shim one plain loop: its matches are the exhaustive float64 ones
    wherever float64 has one nearest record by a margin float32 resolves"""
    c = vf.template_case()
    x, p = c["x"], c["p"]
    T = hr.start_transform(hr.cube_rotation(13), hr.means(x), hr.means(p))
    idx, d2 = hr.nearest(0, T, x, p)
    R, t = vf.split(T)
    z = x.astype(np.float64) @ R.T + t
    ti, td2 = tc.nearest_tree(z, p.astype(np.float64))
    clear = np.abs(d2 - td2) <= 64 * vf.EPS32 * (td2 + np.abs(z).max() ** 2)
    assert clear.all()
    assert (idx == ti).mean() > 0.99 and np.all((idx >= 0) & (idx < len(p)))
    pc = vf.template_partial()
    assert pc["p"].shape == (3889, 3) and 1 < pc["keep_point"] < 3889 and 1 < pc["keep_vert"] < 3889


# ---- E: the host fold -------------------------------------------------------------------------------------------------------------
def _record_cpu(key, value):
    path = os.environ.get(WRITE_ENV)
    if path:
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc["cpu/" + key] = max(float(value), doc.get("cpu/" + key, 0.0))
        with open(path, "w") as fh:
            json.dump(doc, fh, indent=1, sort_keys=True)


def test_exp_is_the_rotation_about_the_axis():
    worst = 0.0
    for an, a in vf.FOLD_AXES.items():
        for th in vf.FOLD_ANGLES:
            R = trainer._rotation_exp(a * th)
            worst = max(worst, rc.rotation_angle(R, vf.rodrigues(a, th)), np.abs(R @ R.T - np.eye(3)).max())
            assert abs(np.linalg.det(R) - 1.0) < vf.FOLD_BOUND
    print("exp against the closed form", worst)
    assert worst < vf.FOLD_BOUND


def test_log_then_exp_gives_the_rotation_back():
    """judged: the angle between exp(log(R)) and R, held to 64 float64 roundings for both kinds of input.  The angle sees the
    rotation between the two alone: what a float32-rounded matrix lacks of being orthonormal is a symmetric stretch (R = Q S, log
    projects onto Q first), which no angle measures.  So a second figure sees it: |exp(log(R)) - R| in the Frobenius norm against
    the yardstick |Q - R|, zero to rounding for a float64 rotation and the float32 rounding (1e-7) for a float32 one.  Before the
    quaternion branch the worst angle was 1.4e-6 rad, about +-(1,1,1) at pi - 2e-6"""
    worst = dict(f64=0.0, f32=0.0, f32_yard=0.0)
    for name, R in vf.fold_matrices():
        r = trainer._rotation_log(R)
        th = float(np.linalg.norm(r))
        assert np.all(np.isfinite(r)) and 0.0 <= th <= vf.PI + vf.FOLD_BOUND, name
        back = trainer._rotation_exp(r)
        figure = rc.rotation_angle(back, R)
        yard = float(np.linalg.norm(vf.projection(R) - R))
        kind = name.rsplit("/", 1)[1]
        worst[kind] = max(worst[kind], figure)
        if kind == "f32":
            worst["f32_yard"] = max(worst["f32_yard"], yard)
        else:
            assert yard < vf.FOLD_BOUND, name
        assert figure <= vf.FOLD_BOUND, (name, figure)
        # (a rotation by a small angle a is sqrt(2) a away in the Frobenius norm)
        assert float(np.linalg.norm(back - R)) <= yard + 2.0 * vf.FOLD_BOUND, (name, yard)
    print(worst)
    assert 1e-8 < worst["f32_yard"] < 3 * np.sqrt(9.0) * vf.EPS32      # nine entries, each rounded by half an ulp of at most 1
    _record_cpu("fold_angle/f64", worst["f64"])
    _record_cpu("fold_angle/f32", worst["f32"])
    _record_cpu("fold_yardstick_frobenius/f32", worst["f32_yard"])
    rec = json.load(open(MEASURED)) if os.path.exists(MEASURED) else {}
    if not os.environ.get(WRITE_ENV):
        assert "cpu/fold_angle/f64" in rec, "tests/golden/hip_rigid_value_forms_measured.json has no cpu/ section"


def test_log_of_a_composition_as_the_fold_forms_it():
    """global_rot <- log(R exp(global_rot)) with R a float32 transform's rotation: the fold's own expression, at a half turn about a
    diagonal (back to front about a tilted axis) composed with small and large poses"""
    rs = np.random.RandomState(2)
    for an in ("diag", "-diag", "y", "skew"):
        for th in (vf.PI, vf.PI - 2e-6, 3.0):
            R32 = vf.rodrigues(vf.FOLD_AXES[an], th).astype(np.float32).astype(np.float64)
            for scale in (0.0, 1e-7, 0.3):
                g = scale * rs.randn(3)
                want = vf.projection(R32 @ trainer._rotation_exp(g))
                got = trainer._rotation_exp(trainer._rotation_log(R32 @ trainer._rotation_exp(g)))
                assert rc.rotation_angle(got, want) < vf.FOLD_BOUND, (an, th, scale)
