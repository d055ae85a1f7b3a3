"""GPU: the trimmed rigid pre-alignment (smalfit_trimmed_rigid_align; include/smalfit.h) through every layer: one iteration against
the float32 host shim (the matches, the kept bytes and the bits of the threshold, exactly) and float64 Kabsch on the device's own
kept pairs; trimming off is smalfit_rigid_align bit for bit; chaining and repeatability; ties; recovery of a known rotation from a
side scan with a floor (the cases the untrimmed call misses by more than 1 rad: tests/test_rigid_trim_cpu.py); the shapes where the
selection can go wrong; a direction of weight 0; entry order; refusals; and the Python layer (engine.RigidAligner.align,
fitter_3d.trainer.rigid_prealign, optimise.py --prealign_trim_*) on the stand-in model.

Tolerances (agreement with float64 Kabsch, orthonormality, recovery, composition): none was fixed in advance.  Each is the deviation
from the float64 restatement measured when tests/golden/hip_rigid_trim_measured.json was written (device/*; the float32 host shim's
own deviation beside it as the yardstick, shim/*), asserted at 3 x the recorded value, one float32 eps where the record is zero.
Hard caps, as the untrimmed call's: a recovered rotation within 1e-3 rad of R*, t within 1e-3 of the extent, the composition error
under 1e-4 of the extent.  SMALFIT_WRITE_RIGID_TRIM_MEASURED=<path> records instead of ratcheting.  Every figure is printed before
it is judged.

The stand-in model's case draws its points ON the target's faces: no rigid motion brings those pairs to distance 0, and the float64
restatement itself ends a sampling error from R* (tests/rigid_trim_cases.py, MODEL_ADMISSION).  There the device is held, under the
same caps, to the restatement's answer on the device's own vertices and points, and the restatement to R* under MODEL_ADMISSION."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from smalify_amd import _lib  # noqa: E402
from smalify_amd import engine as eng  # noqa: E402
from tests import host_rigid_align as hr  # noqa: E402
from tests import host_rigid_trim as ht  # noqa: E402
from tests import mesh3d_cases as mc  # noqa: E402
from tests import rigid_align_cases as rc  # noqa: E402
from tests import rigid_trim_cases as tc  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
MEASURED = os.path.join(HERE, "golden", "hip_rigid_trim_measured.json")
WRITE_ENV = "SMALFIT_WRITE_RIGID_TRIM_MEASURED"
RATCHET = 3.0
EPS32 = float(np.finfo(np.float32).eps)
ZERO_RECORD = 1e-12
ZERO_FLOOR = EPS32
RECOVERY_ANGLE_CAP = 1e-3       # rad
RECOVERY_T_CAP = 1e-3           # of the extent
COMPOSITION_CAP = 1e-4          # of the extent
SENTINEL = -7
BYTE_SENTINEL = 0xAB


def dev(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).cuda()


def _judge(key, value, cap=None, shim=None):
    """print, record and judge one deviation: under its hard cap, and within RATCHET x what was recorded"""
    rec = json.load(open(MEASURED)) if os.path.exists(MEASURED) else {}
    print("%-44s %.3e   cap %s   recorded %s   shim %s" % (key, value, cap, rec.get("device/" + key), shim))
    path = os.environ.get(WRITE_ENV)
    if path:
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc["device/" + key] = max(float(value), doc.get("device/" + key, 0.0))
        if shim is not None:
            doc["shim/" + key] = max(float(shim), doc.get("shim/" + key, 0.0))
        with open(path, "w") as fh:
            json.dump(doc, fh, indent=1, sort_keys=True)
    assert np.isfinite(value)
    if cap is not None:
        assert value < cap, (key, value, cap)
    if path:
        return                                   # a recording run: the ratchet is judged by the next run, against the file
    assert "device/" + key in rec, "tests/golden/hip_rigid_trim_measured.json has no device/%s: run this file with %s=<path> on a " \
        "GPU and commit the result" % (key, WRITE_ENV)
    assert rec["device/" + key] < (cap if cap is not None else np.inf)      # a recorded value above the cap is a bug
    recorded = rec["device/" + key]
    bound = RATCHET * recorded if recorded > ZERO_RECORD else ZERO_FLOOR
    assert value <= bound, (key, value, recorded, bound)


def _split(T):
    T = np.asarray(T, np.float64).reshape(T.shape[:-1] + (3, 4))
    return T[..., :3], T[..., 3]


def _aligner(N, V, S, K=64):
    return eng.RigidAligner(N, V, S, K)


def _host(o):
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in o.items()}


def _frac(keep, count):
    """a fraction that keep_count turns back into `keep`: the midpoint of ((keep - 1) / count, keep / count]"""
    f = (keep - 0.5) / count
    assert eng.keep_count(f, count) == keep
    return f


OUTPUTS = ("transforms", "scores", "best", "best_transform", "kept_rotation", "history", "vert_nn", "point_nn")
TRIM_OUTPUTS = ("vert_kept", "point_kept", "trim_d2")


def _align(al, x, p, keep_point, keep_vert, **kw):
    """engine.RigidAligner.align with the keeps as counts, every optional output on"""
    V, S = int(x.shape[1]), int(p.shape[1])
    return al.align(x, p, trim_point=_frac(keep_point, S), trim_vert=_frac(keep_vert, V), kept=True, history=True, correspondences=True, **kw)


def _raw(al, x, p, trim, iterations=1, w_point=1.0, w_vert=1.0, K=24, fill=SENTINEL, mutate=None):
    """smalfit_trimmed_rigid_align itself, the built-in starts, every output preallocated with a sentinel; trim: None (NULL), or
    (keep_vert, keep_point).  mutate(block, trim block) may break either.  -> (return code, outputs, trim outputs)"""
    N, V, S = int(x.shape[0]), int(x.shape[1]), int(p.shape[1])
    a = _lib.RigidAlignArgs()
    a.num_meshes, a.num_verts, a.num_points, a.num_starts, a.iterations = N, V, S, K, iterations
    a.verts, a.points, a.w_point, a.w_vert = x.data_ptr(), p.data_ptr(), w_point, w_vert
    shapes = dict(transforms=((N, K, 12), torch.float32), scores=((N, K), torch.float32), best=((N,), torch.int32),
                  best_transform=((N, 12), torch.float32), kept_rotation=((N, K), torch.int32), history=((N, K, iterations + 1), torch.float32),
                  vert_nn=((N, K, V), torch.int32), point_nn=((N, K, S), torch.int32))
    o = {k: torch.full(s, fill, dtype=d, device="cuda") for k, (s, d) in shapes.items()}
    for k, v in o.items():
        setattr(a, k, C.c_void_p(v.data_ptr()))
    t, to = None, {}
    if trim is not None:
        t = _lib.RigidTrimArgs()
        t.keep_vert, t.keep_point = trim
        to = dict(vert_kept=torch.full((N, K, V), BYTE_SENTINEL, dtype=torch.uint8, device="cuda"),
                  point_kept=torch.full((N, K, S), BYTE_SENTINEL, dtype=torch.uint8, device="cuda"),
                  trim_d2=torch.full((N, K, 2), float(fill), device="cuda"))
        for k, v in to.items():
            setattr(t, k, C.c_void_p(v.data_ptr()))
    if mutate is not None:
        mutate(a, t)
    fn = _lib.resolve(al.lib, "smalfit_trimmed_rigid_align")
    code = fn(al.handle, None, C.byref(a), C.byref(t) if t is not None else None)
    torch.cuda.synchronize()
    return code, o, to


def _check_round(x, p, o, n, K, keep_point, keep_vert, wp=1.0, wv=1.0):
    """the score's round under the final transforms: matches, kept bytes and threshold bits are the shim's exactly; the score is
    the float64 cost of the kept pairs.  Every direction that is on at its full count: trimming is off and trim_d2 reads 0"""
    V, S = len(x), len(p)
    off = (wv == 0 or keep_vert == V) and (wp == 0 or keep_point == S)
    x64, p64 = x.astype(np.float64), p.astype(np.float64)
    for k in range(K):
        T = o["transforms"][n, k]
        assert np.isfinite(T).all()
        sh = ht.iterate(x, p, T, keep_point, keep_vert, wp, wv)
        R, t = _split(T)
        z = x64 @ R.T + t
        cost = 0.0
        if wv > 0:
            assert np.array_equal(o["vert_nn"][n, k], sh["idx_v"]), (n, k)
            assert np.array_equal(o["vert_kept"][n, k], sh["kept_v"]), (n, k)
            assert int(o["vert_kept"][n, k].sum()) == keep_vert
            m = o["vert_kept"][n, k] == 1
            cost += wv / V * ((z[m] - p64[o["vert_nn"][n, k][m]]) ** 2).sum()
        if wp > 0:
            assert np.array_equal(o["point_nn"][n, k], sh["idx_p"]), (n, k)
            assert np.array_equal(o["point_kept"][n, k], sh["kept_p"]), (n, k)
            assert int(o["point_kept"][n, k].sum()) == keep_point
            m = o["point_kept"][n, k] == 1
            cost += wp / S * ((z[o["point_nn"][n, k][m]] - p64[m]) ** 2).sum()
        want_d2 = np.zeros(2, np.float32) if off else sh["trim_d2"]
        assert np.array_equal(o["trim_d2"][n, k].view(np.uint32), want_d2.view(np.uint32)), (n, k, o["trim_d2"][n, k], want_d2)
        L2 = max(np.abs(z).max(), np.abs(p64).max(), 1e-30) ** 2
        assert abs(o["scores"][n, k] - cost) <= 64 * EPS32 * (cost + L2), (n, k, o["scores"][n, k], cost)
        assert abs(np.linalg.det(R) - 1.0) <= 1e-4


def _kept_pairs(x, p, o, n, k, wp, wv):
    xs, ps, ws = [], [], []
    if wv > 0:
        m = o["vert_kept"][n, k] == 1
        xs.append(x[m]); ps.append(p[o["vert_nn"][n, k][m]]); ws.append(np.full(int(m.sum()), wv / len(x)))
    if wp > 0:
        m = o["point_kept"][n, k] == 1
        xs.append(x[o["point_nn"][n, k][m]]); ps.append(p[m]); ws.append(np.full(int(m.sum()), wp / len(p)))
    return np.concatenate(xs).astype(np.float64), np.concatenate(ps).astype(np.float64), np.concatenate(ws)


# ---- one iteration is the definition --------------------------------------------------------------------------------------------
def test_one_iteration_is_the_definition():
    name = "cube5_skew15"
    c = tc.PARTIAL_CASES[name]
    x, p, kp, kv = c["x"], c["p"], c["keep_point"], c["keep_vert"]
    V, S, K = len(x), len(p), 24
    al = _aligner(1, V, S)
    xd, pd = dev(x[None]), dev(p[None])
    o0 = _host(_align(al, xd, pd, kp, kv, iterations=0))
    assert o0["keep_point"] == kp and o0["keep_vert"] == kv
    T0 = o0["transforms"][0]
    cX, cP = hr.means(x), hr.means(p)
    cube = hr.cube_rotations()
    assert np.array_equal(T0, np.stack([hr.start_transform(cube[k], cX, cP) for k in range(K)]))
    assert np.array_equal(o0["history"][0, :, 0], o0["scores"][0]) and np.all(o0["kept_rotation"] == 0)
    _check_round(x, p, o0, 0, K, kp, kv)           # matches, kept bytes, threshold bits: the shim's, exactly
    o1 = _host(_align(al, xd, pd, kp, kv, start_transforms=dev(T0[None]), iterations=1))
    assert np.array_equal(o1["history"][0, :, 0], o0["scores"][0]) and np.array_equal(o1["history"][0, :, 1], o1["scores"][0])
    R1, t1 = _split(o1["transforms"][0])
    worst = dict(angle=0.0, t=0.0, ortho=0.0, shim_angle=0.0, shim_t=0.0, shim_ortho=0.0)
    x64, p64 = x.astype(np.float64), p.astype(np.float64)
    for k in range(K):
        xs, ps, w = _kept_pairs(x, p, o0, 0, k, 1.0, 1.0)
        Rk, tk, determined = rc.kabsch(xs, ps, w, x64.mean(0), p64.mean(0))
        assert determined and o1["kept_rotation"][0, k] == 0
        Rs, ts = _split(ht.iterate(x, p, T0[k], kp, kv)["T"])
        worst["angle"] = max(worst["angle"], rc.rotation_angle(R1[k], Rk))
        worst["t"] = max(worst["t"], np.abs(t1[k] - tk).max() / c["extent"])
        worst["ortho"] = max(worst["ortho"], np.abs(R1[k] @ R1[k].T - np.eye(3)).max())
        worst["shim_angle"] = max(worst["shim_angle"], rc.rotation_angle(Rs, Rk))
        worst["shim_t"] = max(worst["shim_t"], np.abs(ts - tk).max() / c["extent"])
        worst["shim_ortho"] = max(worst["shim_ortho"], np.abs(Rs @ Rs.T - np.eye(3)).max())
        assert np.linalg.det(R1[k]) > 0.999
    _judge("kabsch_angle/" + name, worst["angle"], shim=worst["shim_angle"])
    _judge("kabsch_t/" + name, worst["t"], shim=worst["shim_t"])
    _judge("orthonormality/" + name, worst["ortho"], shim=worst["shim_ortho"])


# ---- off ------------------------------------------------------------------------------------------------------------------------
def test_trimming_off_is_the_untrimmed_call_bit_for_bit():
    cs = [rc.RECOVERY_CASES[n] for n in rc.BATCH_CASE]
    x, p = dev(np.stack([c["x"] for c in cs])), dev(np.stack([c["p"] for c in cs]))
    N, V, S, K, I = 3, int(x.shape[1]), int(p.shape[1]), 24, 4
    al = _aligner(N, V, S)
    plain = _host(al.align(x, p, iterations=I, history=True, correspondences=True))
    code, null, _ = _raw(al, x, p, None, iterations=I)
    assert code == 0
    code, full, to = _raw(al, x, p, (V, S), iterations=I)
    assert code == 0
    for k in OUTPUTS:
        assert np.array_equal(null[k].cpu().numpy(), plain[k]), k
        assert np.array_equal(full[k].cpu().numpy(), plain[k]), k
    # nothing is computed for the trim outputs: every query kept, no threshold
    assert bool((to["vert_kept"] == 1).all()) and bool((to["point_kept"] == 1).all()) and bool((to["trim_d2"] == 0).all())
    # Python: fractions of 1 with kept=True read (V, S)
    o = _host(al.align(x, p, iterations=I, history=True, correspondences=True, kept=True))
    assert (o["keep_vert"], o["keep_point"]) == (V, S) and o["vert_kept"].all() and o["point_kept"].all()
    for k in OUTPUTS:
        assert np.array_equal(o[k], plain[k]), k
    # a full keep of the one direction that is on, whatever the other's says: off as well
    want = _host(al.align(x, p, iterations=I, w_vert=0.0, history=True, correspondences=True))
    code, got, to = _raw(al, x, p, (1, S), iterations=I, w_vert=0.0)
    assert code == 0 and bool((to["vert_kept"] == BYTE_SENTINEL).all()) and bool((to["point_kept"] == 1).all())
    for k in OUTPUTS:
        if k != "vert_nn":                          # (left alone: the sentinel there, zeros here)
            assert np.array_equal(got[k].cpu().numpy(), want[k]), k


# ---- chaining, repeatability ----------------------------------------------------------------------------------------------------
def _partial_batch():
    cs = [tc.PARTIAL_CASES[n] for n in tc.POSES]
    return cs, np.stack([c["x"] for c in cs]), np.stack([c["p"] for c in cs])


def test_chained_calls_and_repeated_calls_give_the_same_bits():
    cs, x, p = _partial_batch()
    N, V, S = x.shape[0], x.shape[1], p.shape[1]
    kp, kv = tc.KEEP_POINT, tc.KEEP_VERT
    al = _aligner(N, V, S)
    xd, pd = dev(x), dev(p)
    whole = _host(_align(al, xd, pd, kp, kv, iterations=5))
    again = _host(_align(al, xd, pd, kp, kv, iterations=5))
    for k in whole:
        assert np.array_equal(whole[k], again[k]), k
    T = dev(_host(_align(al, xd, pd, kp, kv, iterations=0))["transforms"])
    hist, kept = [], 0
    for it in range(5):
        o = _host(_align(al, xd, pd, kp, kv, start_transforms=T, iterations=1))
        hist.append(o["history"][:, :, 0])
        kept = kept + o["kept_rotation"]
        T = dev(o["transforms"])
    hist.append(o["history"][:, :, 1])
    for k in ("transforms", "scores", "best", "best_transform", "vert_nn", "point_nn") + TRIM_OUTPUTS:
        assert np.array_equal(o[k], whole[k]), k
    assert np.array_equal(np.stack(hist, -1), whole["history"])
    assert np.array_equal(kept, whole["kept_rotation"])


# ---- ties -----------------------------------------------------------------------------------------------------------------------
IDENTITY_T = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)


def test_ties_keep_the_lowest_indices():
    c = tc.PARTIAL_CASES["identity"]
    x, p, seen = c["x"], c["p"], c["seen"]            # the 96 seen vertices copied exactly, then 40 floor points
    V, S = len(x), len(p)
    al = _aligner(1, V, S)
    T = dev(IDENTITY_T[None, None])
    kp, kv = 50, 40                                    # below the 96 inliers of either direction: every kept d^2 is exactly 0
    o = _host(_align(al, dev(x[None]), dev(p[None]), kp, kv, start_transforms=T, iterations=0))
    assert np.array_equal(np.flatnonzero(o["point_kept"][0, 0]), np.arange(kp))
    assert np.array_equal(np.flatnonzero(o["vert_kept"][0, 0]), np.flatnonzero(seen)[:kv])
    assert np.array_equal(o["trim_d2"][0, 0].view(np.uint32), np.zeros(2, np.uint32)) and o["scores"][0, 0] == 0.0
    _check_round(x, p, o, 0, 1, kp, kv)
    # every d^2 equal: vertices 4 apart on a line, every point 0.5 beside its vertex
    n = 70
    xl = np.zeros((n, 3), np.float32)
    xl[:, 0] = 4.0 * np.arange(n)
    pl = xl + np.array([0.0, 0.5, 0.0], np.float32)
    o = _host(_align(_aligner(1, n, n), dev(xl[None]), dev(pl[None]), 33, 65, start_transforms=T, iterations=0))
    assert np.array_equal(np.flatnonzero(o["point_kept"][0, 0]), np.arange(33))
    assert np.array_equal(np.flatnonzero(o["vert_kept"][0, 0]), np.arange(65))
    assert np.array_equal(o["trim_d2"][0, 0], np.full(2, 0.25, np.float32))
    _check_round(xl, pl, o, 0, 1, 33, 65)


# ---- recovery -------------------------------------------------------------------------------------------------------------------
def _shim_recovery(c, start):
    T = hr.start_transform(hr.cube_rotation(start), hr.means(c["x"]), hr.means(c["p"]))
    for _ in range(tc.TRIM_ITERATIONS):
        T = ht.iterate(c["x"], c["p"], T, c["keep_point"], c["keep_vert"])["T"]
    R, t = _split(T)
    return rc.rotation_angle(R, c["R"]), np.abs(t - c["t"]).max() / c["extent"]


def test_recovery_from_a_side_scan_with_a_floor():
    """the four admitted poses as one N = 4 call, 24 starts, 30 iterations"""
    cs, x, p = _partial_batch()
    al = _aligner(4, x.shape[1], p.shape[1])
    o = _host(_align(al, dev(x), dev(p), tc.KEEP_POINT, tc.KEEP_VERT, iterations=tc.TRIM_ITERATIONS))
    for k in ("transforms", "scores", "history", "trim_d2"):
        assert np.isfinite(o[k]).all(), k
    for n, c in enumerate(cs):
        b = int(o["best"][n])
        assert b == int(np.argmin(o["scores"][n])) and np.array_equal(o["best_transform"][n], o["transforms"][n, b])
        R, t = _split(o["best_transform"][n])
        ref = tc.reference(c["name"])
        shim_angle, shim_t = _shim_recovery(c, ref["best"])
        _judge("recovery_angle/" + c["name"], rc.rotation_angle(R, c["R"]), cap=RECOVERY_ANGLE_CAP, shim=shim_angle)
        _judge("recovery_t/" + c["name"], np.abs(t - c["t"]).max() / c["extent"], cap=RECOVERY_T_CAP, shim=shim_t)
        assert o["kept_rotation"][n, b] == 0
        assert o["scores"][n, b] <= 1e-6            # the kept pairs are exact correspondences: the optimum's cost is rounding
        # the floor is dropped: no kept point of the winner lies on it, and the winner's thresholds are rounding
        assert not o["point_kept"][n, b][96:].any() and o["trim_d2"][n, b].max() <= 1e-6


# ---- shapes where it can go wrong -----------------------------------------------------------------------------------------------
def _cloud(V, S, seed):
    rs = np.random.RandomState(seed)
    x = (rs.randn(V, 3) * [1.0, 0.5, 0.25]).astype(np.float32)
    p = rc.moved(x[rs.randint(0, V, S)] + (0.02 * rs.randn(S, 3)).astype(np.float32), rc.axis_angle([1, 1, 0], 10.0), [0.1, 0.0, -0.1])
    return x, p


def _random_rotations(K, seed):
    rs = np.random.RandomState(seed)
    return np.stack([rc.axis_angle(rs.randn(3), rs.uniform(0, 180)) for _ in range(K)]).astype(np.float32)


@pytest.mark.parametrize("V,S,kv,kp", [(1, 1, 1, 1), (65, 2500, 33, 1700), (255, 256, 254, 1), (256, 257, 129, 256), (257, 255, 1, 128)])
def test_sizes_at_the_edges_of_a_block_a_chunk_and_the_selection_stride(V, S, kv, kp):
    x, p = _cloud(V, S, V * 7 + S)
    K, I = 3, 2
    starts = _random_rotations(K, V + S)
    starts[0] = np.eye(3)
    o = _host(_align(_aligner(1, V, S, K), dev(x[None]), dev(p[None]), kp, kv, starts=starts, iterations=I))
    _check_round(x, p, o, 0, K, kp, kv)
    assert o["best"][0] == int(np.argmin(o["scores"][0]))
    if V == 1:
        assert np.all(o["kept_rotation"] == I)


def test_one_start_through_start_transforms_and_three_meshes():
    N, V, S, kv, kp = 3, 130, 97, 70, 60
    clouds = [_cloud(V, S, 40 + n) for n in range(N)]
    x, p = np.stack([c[0] for c in clouds]), np.stack([c[1] for c in clouds])
    T0 = np.stack([np.concatenate([rc.axis_angle([n + 1, 1, 0], 8.0 * n), [[0.1], [0.0], [-0.1]]], 1).reshape(1, 12) for n in range(N)]).astype(np.float32)
    al = _aligner(N, V, S, 1)
    o = _host(_align(al, dev(x), dev(p), kp, kv, start_transforms=dev(T0), iterations=2))
    assert o["transforms"].shape == (N, 1, 12) and np.all(o["best"] == 0)
    one = _aligner(1, V, S, 1)
    for n in range(N):
        _check_round(x[n], p[n], o, n, 1, kp, kv)
        single = _host(_align(one, dev(x[n:n + 1]), dev(p[n:n + 1]), kp, kv, start_transforms=dev(T0[n:n + 1]), iterations=2))
        for k in OUTPUTS + TRIM_OUTPUTS:
            assert np.array_equal(o[k][n], single[k][0]), (n, k)


@pytest.mark.parametrize("wp,wv", [(1.0, 0.0), (0.0, 1.0)])
def test_a_direction_of_weight_zero_is_skipped(wp, wv):
    c = tc.PARTIAL_CASES["cube5_skew15"]
    x, p = c["x"], c["p"]
    V, S, K = len(x), len(p), 24
    al = _aligner(1, V, S)
    out = dict(vert_nn=torch.full((1, K, V), SENTINEL, dtype=torch.int32, device="cuda"),
               point_nn=torch.full((1, K, S), SENTINEL, dtype=torch.int32, device="cuda"),
               vert_kept=torch.full((1, K, V), BYTE_SENTINEL, dtype=torch.uint8, device="cuda"),
               point_kept=torch.full((1, K, S), BYTE_SENTINEL, dtype=torch.uint8, device="cuda"),
               trim_d2=torch.full((1, K, 2), float(SENTINEL), device="cuda"))
    o = _host(_align(al, dev(x[None]), dev(p[None]), c["keep_point"], c["keep_vert"], iterations=2, w_point=wp, w_vert=wv, out=out))
    assert np.all(o["vert_nn"] == SENTINEL) == (wv == 0.0) and np.all(o["point_nn"] == SENTINEL) == (wp == 0.0)
    assert np.all(o["vert_kept"] == BYTE_SENTINEL) == (wv == 0.0) and np.all(o["point_kept"] == BYTE_SENTINEL) == (wp == 0.0)
    assert np.all(o["trim_d2"][0, :, 0 if wv == 0.0 else 1] == 0.0)           # a skipped direction's threshold reads 0
    _check_round(x, p, o, 0, K, c["keep_point"], c["keep_vert"], wp, wv)
    # a keep out of range for the direction of weight 0 is accepted and ignored
    code, raw, to = _raw(al, dev(x[None]), dev(p[None]), (c["keep_vert"] if wv > 0 else 10 ** 6, c["keep_point"] if wp > 0 else -5),
                         iterations=2, w_point=wp, w_vert=wv)
    assert code == 0
    for k in ("transforms", "scores", "best"):
        assert np.array_equal(raw[k].cpu().numpy(), o[k]), k


# ---- entry order ------------------------------------------------------------------------------------------------------------------
def test_entry_order_and_a_larger_handle():
    cs, x, p = _partial_batch()
    x, p = dev(x[:2]), dev(p[:2])
    V, S, kp, kv = int(x.shape[1]), int(p.shape[1]), tc.KEEP_POINT, tc.KEEP_VERT
    fresh_trim = _host(_align(_aligner(2, V, S, 24), x, p, kp, kv, iterations=3))
    fresh_plain = _host(_aligner(2, V, S, 24).align(x, p, iterations=3, history=True, correspondences=True))
    al = _aligner(2, V, S, 24)
    first = _host(_align(al, x, p, kp, kv, iterations=3))
    plain = _host(al.align(x, p, iterations=3, history=True, correspondences=True))
    second = _host(_align(al, x, p, kp, kv, iterations=3))
    for k in fresh_trim:
        assert np.array_equal(first[k], fresh_trim[k]) and np.array_equal(second[k], fresh_trim[k]), k
    for k in fresh_plain:
        assert np.array_equal(plain[k], fresh_plain[k]), k
    roomy = _aligner(5, V + 300, S + 1000, 64)
    big = _host(_align(roomy, x, p, kp, kv, iterations=3))
    for k in fresh_trim:
        assert np.array_equal(big[k], fresh_trim[k]), k
    # an untrimmed call first, on a handle that has not trimmed yet
    late = _aligner(2, V, S, 24)
    late.align(x, p, iterations=1)
    got = _host(_align(late, x, p, kp, kv, iterations=3))
    for k in fresh_trim:
        assert np.array_equal(got[k], fresh_trim[k]), k


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_a_refused_block_leaves_every_output_alone():
    c = tc.PARTIAL_CASES["identity"]
    x, p = dev(c["x"][None]), dev(c["p"][None])
    V, S = int(x.shape[1]), int(p.shape[1])
    al = _aligner(1, V, S, 24)
    lib = _lib.load()

    def bad_size(a, t):
        t.struct_size += 8

    def bad_args(a, t):
        a.iterations = 1001

    refused = [
        ((77, 87), bad_size, "smalfit_rigid_trim_args.struct_size does not match"),
        ((0, 87), None, "keep_vert must be 1 .. num_verts"),
        ((V + 1, 87), None, "keep_vert must be 1 .. num_verts"),
        ((77, 0), None, "keep_point must be 1 .. num_points"),
        ((77, S + 1), None, "keep_point must be 1 .. num_points"),
        ((0, S + 1), None, "keep_vert must be 1 .. num_verts"),              # the vertices' keep is judged first
        ((0, 0), bad_size, "struct_size does not match"),                   # ... and the size before either
        ((77, 87), bad_args, "iterations must be 0..1000"),                 # the call's own block before the trim block
        (None, bad_args, "iterations must be 0..1000"),
    ]
    for trim, mutate, text in refused:
        code, o, to = _raw(al, x, p, trim, mutate=mutate)
        assert code != 0 and text in lib.smalfit_last_error().decode(), (trim, text, lib.smalfit_last_error())
        assert lib.smalfit_last_error().decode().startswith("smalfit_trimmed_rigid_align: ")
        for k, v in o.items():
            assert bool((v == SENTINEL).all()), (text, k)
        for k, v in to.items():
            assert bool((v == (BYTE_SENTINEL if v.dtype == torch.uint8 else SENTINEL)).all()), (text, k)
    # the same blocks, mended, are accepted on the same handle
    code, o, to = _raw(al, x, p, (77, 87))
    assert code == 0 and not bool((o["scores"] == SENTINEL).any()) and not bool((to["trim_d2"] == SENTINEL).any())
    # Python: a fraction outside (0, 1] raises before anything is allocated or enqueued
    for kw in (dict(trim_point=0.0), dict(trim_vert=1.5), dict(trim_point=float("nan"))):
        with pytest.raises(eng.SmalfitError, match="must be in \\(0, 1\\]"):
            al.align(x, p, iterations=1, **kw)


# ---- the Python layer on the stand-in model -------------------------------------------------------------------------------------
def test_rigid_prealign_trimmed_folds_the_transform_into_the_parameters():
    from smalify_amd.fitter_3d import TargetMeshes, trainer
    md, fit, _ = mc.fitter_problem(1, seed=3)
    g, j, b = tc.model_parameters()
    with torch.no_grad():
        fit.global_rot.copy_(dev(g))
        fit.joint_rot.copy_(dev(j.reshape(fit.joint_rot.shape)))
        fit.betas.copy_(dev(b.reshape(fit.betas.shape)))
    frozen = {k: getattr(fit, k).detach().clone() for k in ("betas", "joint_rot", "log_beta_scales", "deform_verts")}
    before32 = fit().cpu().numpy()
    before = before32.astype(np.float64)
    tv, tf, seen = tc.partial_target(before[0], md.faces)
    targets = TargetMeshes([tv], [tf])
    S, V = tc.MODEL_POINTS, before.shape[1]
    # the admission, on the fitter's own vertices and the points rigid_prealign draws: the float64 restatement lands at R*
    key = (5 + trainer.PREALIGN_SEED_OFFSET) & (2 ** 64 - 1)
    points = targets.sample(S, key, trainer.PREALIGN_ITERATION).cpu().numpy()
    kp, kv = eng.keep_count(tc.MODEL_TRIM_POINT, S), eng.keep_count(tc.MODEL_TRIM_VERT, V)
    ref = tc.align(before32[0], points[0], kp, kv, nearest=tc.nearest_tree)
    rb = ref["best"]
    admitted = rc.rotation_angle(ref["R"][rb], tc.MODEL_TURN)
    print("restatement: best", rb, "angle off R*", admitted, "score", ref["scores"][rb])
    assert admitted <= tc.MODEL_ADMISSION, "the cut is not admitted on the device's vertices and points: choose another"
    report = trainer.rigid_prealign(fit, targets, num_points=S, seed=5, trim_point=tc.MODEL_TRIM_POINT, trim_vert=tc.MODEL_TRIM_VERT)
    after = fit().cpu().numpy().astype(np.float64)
    row = report[0]
    R, t = _split(np.asarray(row["transform"]))
    extent = (before[0].max(0) - before[0].min(0)).max()
    print("device: best", row["best"], "off R*", rc.rotation_angle(R, tc.MODEL_TURN), "score", row["score"], "thresholds",
          row["trim_dist_point"], row["trim_dist_vert"])
    assert row["best"] == rb and row["kept_rotation"] == 0
    assert (row["trim_point"], row["trim_vert"], row["kept_points"], row["kept_verts"]) == (tc.MODEL_TRIM_POINT, tc.MODEL_TRIM_VERT, kp, kv)
    assert 0 < row["trim_dist_point"] < 0.2 * extent and 0 < row["trim_dist_vert"] < 0.2 * extent
    assert abs(row["trim_dist_point"] - np.sqrt(ref["trim_d2"][rb, 1])) <= 1e-2 * extent
    _judge("model_angle", rc.rotation_angle(R, ref["R"][rb]), cap=RECOVERY_ANGLE_CAP)
    _judge("model_t", np.abs(t - ref["t"][rb]).max() / extent, cap=RECOVERY_T_CAP)
    assert rc.rotation_angle(R, tc.MODEL_TURN) <= tc.MODEL_ADMISSION + RECOVERY_ANGLE_CAP
    _judge("composition", np.abs(after[0] - (before[0] @ R.T + t)).max() / extent, cap=COMPOSITION_CAP)
    for k, v in frozen.items():
        assert torch.equal(getattr(fit, k).detach(), v), k
    # untrimmed, the report is what it was: none of the new keys
    plain = trainer.rigid_prealign(fit, targets, num_points=S, seed=5, iterations=1)
    assert set(plain[0]) == {"best", "score", "angle", "angle_degrees", "kept_rotation", "identity_score", "transform"}


def _write_meshes(tmp_path, meshes):
    mesh_dir = tmp_path / "meshes"
    mesh_dir.mkdir()
    for name, (v, f) in meshes.items():
        with open(mesh_dir / (name + ".obj"), "w") as fh:
            for q in v:
                fh.write("v %.7f %.7f %.7f\n" % tuple(q))
            for tri in f:
                fh.write("f %d %d %d\n" % tuple(tri + 1))
    return mesh_dir


def test_optimise_main_with_the_trim_flags(tmp_path):
    from smalify_amd.fitter_3d import optimise
    md = mc.synthetic.synthetic_model(seed=0, shape_family_id=-1)
    tv, tf = mc.target_meshes_from_smal(md, 1, seed=9)
    mesh_dir = _write_meshes(tmp_path, dict(m0=(tv[0], tf)))

    def run(out, *flags):
        args = optimise.build_parser().parse_args(["--mesh_dir", str(mesh_dir), "--results_dir", str(tmp_path / out), "--scheme", "init",
                                                   "--nits", "2", "--lr", "0.05", "--seed", "4", "--no_plots", *flags])
        optimise.main(args, model_data=md, smal_data=mc.synthetic_smal_data())
        return np.load(tmp_path / out / "optimise.npz", allow_pickle=True)

    parsed = optimise.build_parser().parse_args([])
    assert parsed.prealign_trim_point is None and parsed.prealign_trim_vert is None
    plain = run("plain", "--prealign", "--prealign_iterations", "4")
    trimmed = run("trimmed", "--prealign", "--prealign_iterations", "4", "--prealign_trim_point", "0.8", "--prealign_trim_vert", "0.6")
    doc_plain = json.load(open(tmp_path / "plain" / "prealign.json"))
    doc = json.load(open(tmp_path / "trimmed" / "prealign.json"))
    new = {"trim_point", "trim_vert", "kept_points", "kept_verts", "trim_dist_point", "trim_dist_vert"}
    old = {"name", "best", "score", "angle", "angle_degrees", "kept_rotation", "identity_score", "transform"}
    assert set(doc_plain) == set(doc) == {"iterations", "starts", "meshes"}
    for row in doc_plain["meshes"]:
        assert set(row) == old
    for row in doc["meshes"]:
        assert set(row) == old | new
        assert (row["trim_point"], row["trim_vert"]) == (0.8, 0.6) and row["kept_verts"] == eng.keep_count(0.6, md.num_verts)
        assert row["trim_dist_point"] >= 0 and row["trim_dist_vert"] >= 0
    assert sorted(plain.files) == sorted(trimmed.files)                  # the .npz arrays are those of a plain --prealign run
    # the flags without --prealign are refused, before anything is loaded or written
    for flags in (("--prealign_trim_point", "0.8"), ("--prealign_trim_vert", "0.6")):
        with pytest.raises(ValueError, match="give --prealign"):
            run("refused", *flags)
        assert not os.path.exists(tmp_path / "refused")
    # YAML: the same keys under args
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("stages:\n  Stage0:\n    scheme: 'init'\n    nits: 2\n    lr: 0.05\nargs:\n  results_dir: %s\n  prealign: true\n"
                   "  prealign_iterations: 3\n  prealign_trim_point: 0.7\n  prealign_trim_vert: 0.5\n" % (tmp_path / "yaml"))
    args = optimise.build_parser().parse_args(["--mesh_dir", str(mesh_dir), "--yaml_src", str(cfg), "--no_plots"])
    optimise.main(args, model_data=md, smal_data=mc.synthetic_smal_data())
    ydoc = json.load(open(tmp_path / "yaml" / "prealign.json"))
    assert ydoc["iterations"] == 3 and ydoc["meshes"][0]["trim_point"] == 0.7 and ydoc["meshes"][0]["trim_vert"] == 0.5
