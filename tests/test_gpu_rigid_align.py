"""GPU: the rigid pre-alignment (smalfit_rigid_align; include/smalfit.h) through every layer: one iteration against the float32
host shim (the matches, exactly) and float64 Kabsch on those same pairs; chaining and repeatability bit for bit; recovery of a
known rotation on every admitted case of tests/rigid_align_cases.py; the shapes where the kernels can go wrong; refusals; and the
Python layer (engine.RigidAligner, fitter_3d.trainer.rigid_prealign, optimise.py --prealign) on the stand-in model.

Tolerances (agreement with float64 Kabsch, orthonormality, recovery, composition): none was fixed in advance.  Each is the deviation
from the float64 restatement measured when tests/golden/hip_rigid_align_measured.json was written (device/*; the float32 host shim's
own deviation stands beside it as the yardstick, shim/*), asserted at 3 x the recorded value; only where the recorded value is zero
(the identity, the half turn: cube rotations the start already holds exactly) one float32 eps stands in for it.  Hard caps the ratchet cannot hide a wrong answer behind: a recovered rotation within 1e-3 rad of R*, t within 1e-3 of the
extent, the composition error under 1e-4 of the extent.  SMALFIT_WRITE_RIGID_ALIGN_MEASURED=<path> records instead of ratcheting.
Every figure is printed before it is judged."""
import json
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from smalify_amd import engine as eng  # noqa: E402
from tests import host_rigid_align as hr  # noqa: E402
from tests import mesh3d_cases as mc  # noqa: E402
from tests import rigid_align_cases as rc  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
MEASURED = os.path.join(HERE, "golden", "hip_rigid_align_measured.json")
RATCHET = 3.0
EPS32 = float(np.finfo(np.float32).eps)
ZERO_RECORD = 1e-12             # a recorded deviation below this is zero up to float64 rounding: 3 x it bounds nothing ...
ZERO_FLOOR = EPS32              # ... and one float32 eps, a last bit of a rotation's entry, stands in for it
RECOVERY_ANGLE_CAP = 1e-3       # rad
RECOVERY_T_CAP = 1e-3           # of the extent
COMPOSITION_CAP = 1e-4          # of the extent
SENTINEL = -7


def _chunk():
    src = open(os.path.join(HERE, "..", "smalify_amd", "csrc", "kernels_rigid_align.inc")).read()
    return int(re.search(r"constexpr int kRigidChunk = (\d+);", src).group(1))


CHUNK = _chunk()


def dev(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).cuda()


def _judge(key, value, cap=None, shim=None):
    """print, record and judge one deviation: under its hard cap, and within RATCHET x what was recorded"""
    rec = json.load(open(MEASURED)) if os.path.exists(MEASURED) else {}
    print("%-44s %.3e   cap %s   recorded %s   shim %s" % (key, value, cap, rec.get("device/" + key), shim))
    path = os.environ.get("SMALFIT_WRITE_RIGID_ALIGN_MEASURED")
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
    assert "device/" + key in rec, "tests/golden/hip_rigid_align_measured.json has no device/%s: run this file with " \
        "SMALFIT_WRITE_RIGID_ALIGN_MEASURED=<path> on a GPU and commit the result" % key
    assert rec["device/" + key] < (cap if cap is not None else np.inf)      # a recorded value above the cap is a bug
    recorded = rec["device/" + key]
    bound = RATCHET * recorded if recorded > ZERO_RECORD else ZERO_FLOOR
    assert value <= bound, (key, value, recorded, bound)


def _split(T):
    T = np.asarray(T, np.float64).reshape(T.shape[:-1] + (3, 4))
    return T[..., :3], T[..., 3]


def _gpu_pairs(x, p, vert_nn, point_nn, w_point, w_vert):
    """the weighted pair set of the matches the device found"""
    xs, ps, ws = [], [], []
    if w_vert > 0:
        xs.append(x); ps.append(p[vert_nn]); ws.append(np.full(len(x), w_vert / len(x)))
    if w_point > 0:
        xs.append(x[point_nn]); ps.append(p); ws.append(np.full(len(p), w_point / len(p)))
    return np.concatenate(xs).astype(np.float64), np.concatenate(ps).astype(np.float64), np.concatenate(ws)


def _aligner(N, V, S, K=64):
    return eng.RigidAligner(N, V, S, K)


def _host(o):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


# ---- one iteration is the definition --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("cube5_skew15", "cube9_skew18_subset"))
def test_one_iteration_is_the_definition(name):
    c = rc.RECOVERY_CASES[name]
    x, p, wp, wv = c["x"], c["p"], c["w_point"], c["w_vert"]
    V, S, K = len(x), len(p), 24
    al = _aligner(1, V, S)
    xd, pd = dev(x[None]), dev(p[None])
    o0 = _host(al.align(xd, pd, iterations=0, w_point=wp, w_vert=wv, history=True, correspondences=True))
    T0 = o0["transforms"][0]
    # the starts: z = R_k (x - c_X) + c_P with the means summed as the header says -- the shim's bits
    cX, cP = hr.means(x), hr.means(p)
    cube = hr.cube_rotations()
    want_T0 = np.stack([hr.start_transform(cube[k], cX, cP) for k in range(K)])
    assert np.array_equal(T0, want_T0)
    assert np.array_equal(o0["history"][0, :, 0], o0["scores"][0]) and np.all(o0["kept_rotation"] == 0)
    o1 = _host(al.align(xd, pd, start_transforms=dev(T0[None]), iterations=1, w_point=wp, w_vert=wv, history=True))
    # history[0] is the cost under the start: the scores of the I = 0 call, bit for bit
    assert np.array_equal(o1["history"][0, :, 0], o0["scores"][0])
    assert np.array_equal(o1["history"][0, :, 1], o1["scores"][0])
    R1, t1 = _split(o1["transforms"][0])
    worst = dict(angle=0.0, t=0.0, ortho=0.0, shim_angle=0.0, shim_t=0.0, shim_ortho=0.0)
    x64, p64 = x.astype(np.float64), p.astype(np.float64)
    for k in range(K):
        # the matches are the float32 host shim's, exactly
        if wv > 0:
            assert np.array_equal(o0["vert_nn"][0, k], hr.nearest(0, T0[k], x, p)[0]), k
        if wp > 0:
            assert np.array_equal(o0["point_nn"][0, k], hr.nearest(1, T0[k], x, p)[0]), k
        xs, ps, w = _gpu_pairs(x, p, o0["vert_nn"][0, k], o0["point_nn"][0, k], wp, wv)
        Rk, tk, determined = rc.kabsch(xs, ps, w, x64.mean(0), p64.mean(0))
        assert determined and o1["kept_rotation"][0, k] == 0
        sh = hr.iterate(x, p, T0[k], wp, wv)
        Rs, ts = _split(sh["T"])
        worst["angle"] = max(worst["angle"], rc.rotation_angle(R1[k], Rk))
        worst["t"] = max(worst["t"], np.abs(t1[k] - tk).max() / c["extent"])
        worst["ortho"] = max(worst["ortho"], np.abs(R1[k] @ R1[k].T - np.eye(3)).max())
        worst["shim_angle"] = max(worst["shim_angle"], rc.rotation_angle(Rs, Rk))
        worst["shim_t"] = max(worst["shim_t"], np.abs(ts - tk).max() / c["extent"])
        worst["shim_ortho"] = max(worst["shim_ortho"], np.abs(Rs @ Rs.T - np.eye(3)).max())
        assert np.linalg.det(R1[k]) > 0.999
        # the cost is the definition's: w_point / S sum d^2 + w_vert / V sum d^2 over those matches
        z = x64 @ _split(T0[k])[0].T + _split(T0[k])[1]
        cost = (wv / V * ((z - p64[o0["vert_nn"][0, k]]) ** 2).sum() if wv > 0 else 0.0) + \
               (wp / S * ((z[o0["point_nn"][0, k]] - p64) ** 2).sum() if wp > 0 else 0.0)
        assert abs(o0["scores"][0, k] - cost) <= 64 * EPS32 * cost + 1e-12
    _judge("kabsch_angle/" + name, worst["angle"], shim=worst["shim_angle"])
    _judge("kabsch_t/" + name, worst["t"], shim=worst["shim_t"])
    _judge("orthonormality/" + name, worst["ortho"], shim=worst["shim_ortho"])


# ---- chaining, repeatability ----------------------------------------------------------------------------------------------------
def _batch():
    cs = [rc.RECOVERY_CASES[n] for n in rc.BATCH_CASE]
    return cs, np.stack([c["x"] for c in cs]), np.stack([c["p"] for c in cs])


def test_chained_calls_and_repeated_calls_give_the_same_bits():
    cs, x, p = _batch()
    N, V, S = x.shape[0], x.shape[1], p.shape[1]
    al = _aligner(N, V, S)
    xd, pd = dev(x), dev(p)
    whole = _host(al.align(xd, pd, iterations=5, history=True))
    again = _host(al.align(xd, pd, iterations=5, history=True))
    for k in whole:
        assert np.array_equal(whole[k], again[k]), k
    T = dev(_host(al.align(xd, pd, iterations=0))["transforms"])
    hist, kept = [], 0
    for it in range(5):
        o = _host(al.align(xd, pd, start_transforms=T, iterations=1, history=True))
        hist.append(o["history"][:, :, 0])
        kept = kept + o["kept_rotation"]
        T = dev(o["transforms"])
    hist.append(o["history"][:, :, 1])
    assert np.array_equal(o["transforms"], whole["transforms"])
    assert np.array_equal(o["scores"], whole["scores"])
    assert np.array_equal(np.stack(hist, -1), whole["history"])
    assert np.array_equal(kept, whole["kept_rotation"])
    assert np.array_equal(o["best"], whole["best"]) and np.array_equal(o["best_transform"], whole["best_transform"])


# ---- recovery -------------------------------------------------------------------------------------------------------------------
_SINGLE = {}


def _single(name):
    """the default call (24 built-in starts, 30 iterations) on one recovery case, computed once"""
    if name not in _SINGLE:
        c = rc.RECOVERY_CASES[name]
        al = _aligner(1, len(c["x"]), len(c["p"]))
        _SINGLE[name] = _host(al.align(dev(c["x"][None]), dev(c["p"][None]), iterations=rc.RECOVERY_ITERATIONS, w_point=c["w_point"],
                                       w_vert=c["w_vert"], history=True))
    return _SINGLE[name]


def _shim_recovery(name):
    """the float32 host shim iterated from the start the float64 restatement's winner began at: the yardstick"""
    c = rc.RECOVERY_CASES[name]
    k = rc.reference(name)["best"]
    T = hr.start_transform(hr.cube_rotation(k), hr.means(c["x"]), hr.means(c["p"]))
    for _ in range(rc.RECOVERY_ITERATIONS):
        T = hr.iterate(c["x"], c["p"], T, c["w_point"], c["w_vert"])["T"]
    R, t = _split(T)
    return rc.rotation_angle(R, c["R"]), np.abs(t - c["t"]).max() / c["extent"]


@pytest.mark.parametrize("name", sorted(rc.RECOVERY_CASES))
def test_recovery_of_a_known_rotation(name):
    c = rc.RECOVERY_CASES[name]
    o = _single(name)
    scores = o["scores"][0]
    b = int(o["best"][0])
    assert np.isfinite(o["transforms"]).all() and np.isfinite(scores).all() and np.isfinite(o["history"]).all()
    assert b == int(np.argmin(scores))                     # (argmin: the lowest index among equal values)
    assert np.array_equal(o["best_transform"][0], o["transforms"][0, b])
    assert np.array_equal(o["history"][0, :, -1], scores)
    R, t = _split(o["best_transform"][0])
    shim_angle, shim_t = _shim_recovery(name)
    _judge("recovery_angle/" + name, rc.rotation_angle(R, c["R"]), cap=RECOVERY_ANGLE_CAP, shim=shim_angle)
    _judge("recovery_t/" + name, np.abs(t - c["t"]).max() / c["extent"], cap=RECOVERY_T_CAP, shim=shim_t)
    assert o["kept_rotation"][0, b] == 0
    ref = rc.reference(name)
    assert scores[b] <= 1e-6 and ref["scores"][ref["best"]] <= 1e-12      # exact correspondences exist: the optimum's cost is rounding
    if name == "back_to_front":
        assert scores[0] > scores[b] and scores[0] > 1e-3     # the identity start settles back to front: strictly worse


def test_batch_of_three_meshes_each_with_its_own_rotation():
    """N = 3 with a different R* per mesh: every mesh's outputs are the bits of its own N = 1 call (catches mesh indexing)"""
    cs, x, p = _batch()
    al = _aligner(3, x.shape[1], p.shape[1])
    o = _host(al.align(dev(x), dev(p), iterations=rc.RECOVERY_ITERATIONS, history=True))
    for n, c in enumerate(cs):
        one = _single(c["name"])
        for k in ("transforms", "scores", "best", "best_transform", "kept_rotation", "history"):
            assert np.array_equal(o[k][n], one[k][0]), (n, k)
        R, t = _split(o["best_transform"][n])
        assert rc.rotation_angle(R, c["R"]) < RECOVERY_ANGLE_CAP


# ---- shapes where it can go wrong -----------------------------------------------------------------------------------------------
def _random_rotations(K, seed):
    rs = np.random.RandomState(seed)
    return np.stack([rc.axis_angle(rs.randn(3), rs.uniform(0, 180)) for _ in range(K)]).astype(np.float32)


def _check_against_the_definition(x, p, o, n, K, iterations, wp=1.0, wv=1.0):
    """under the final transforms: the matches are the shim's exactly, the scores the float64 cost of those matches; outputs finite"""
    V, S = len(x), len(p)
    x64, p64 = x.astype(np.float64), p.astype(np.float64)
    for k in range(K):
        T = o["transforms"][n, k]
        assert np.isfinite(T).all()
        R, t = _split(T)
        z = x64 @ R.T + t
        cost = 0.0
        if wv > 0:
            assert np.array_equal(o["vert_nn"][n, k], hr.nearest(0, T, x, p)[0]), (n, k)
            cost += wv / V * ((z - p64[o["vert_nn"][n, k]]) ** 2).sum()
        if wp > 0:
            assert np.array_equal(o["point_nn"][n, k], hr.nearest(1, T, x, p)[0]), (n, k)
            cost += wp / S * ((z[o["point_nn"][n, k]] - p64) ** 2).sum()
        # float32 d^2 of a transformed point: a few eps of the squared coordinates, not of the (possibly tiny) cost
        L2 = max(np.abs(z).max(), np.abs(p64).max(), 1e-30) ** 2
        assert abs(o["scores"][n, k] - cost) <= 64 * EPS32 * (cost + L2), (n, k, o["scores"][n, k], cost)
        assert 0 <= o["kept_rotation"][n, k] <= iterations
        assert abs(np.linalg.det(R) - 1.0) <= 1e-4


@pytest.mark.parametrize("V,S", [(v, s) for v in (1, 63, 64, 65) for s in (1, 63, 64, 65)] + [(CHUNK + 1, 70), (70, CHUNK + 1)])
def test_sizes_at_the_edges_of_a_block_and_of_the_staged_chunk(V, S):
    rs = np.random.RandomState(V * 7 + S)
    x = (rs.randn(V, 3) * [1.0, 0.5, 0.25]).astype(np.float32)
    p = rc.moved(x[rs.randint(0, V, S)] + (0.02 * rs.randn(S, 3)).astype(np.float32), rc.axis_angle([1, 1, 0], 10.0), [0.1, 0.0, -0.1])
    K, I = 3, 2
    starts = _random_rotations(K, V + S)
    starts[0] = np.eye(3)
    al = _aligner(1, V, S, K)
    o = _host(al.align(dev(x[None]), dev(p[None]), starts=starts, iterations=I, history=True, correspondences=True))
    _check_against_the_definition(x, p, o, 0, K, I)
    assert o["best"][0] == int(np.argmin(o["scores"][0]))
    if V == 1 or S == 1:
        # one vertex or one point: every pair set is coincident on one side, the rotation is undetermined and kept
        assert np.all(o["kept_rotation"] == I)
        for k in range(K):
            assert np.array_equal(o["transforms"][0, k].reshape(3, 4)[:, :3], starts[k])


@pytest.mark.parametrize("K", (1, 24, 64))
def test_start_counts(K):
    c = rc.RECOVERY_CASES["cube13_skew25"]
    x, p = c["x"], c["p"]
    starts = None if K == 24 else _random_rotations(K, K)
    al = _aligner(1, len(x), len(p), K)
    o = _host(al.align(dev(x[None]), dev(p[None]), starts=starts, iterations=1, history=True, correspondences=True))
    assert o["transforms"].shape == (1, K, 12) and o["scores"].shape == (1, K) and o["history"].shape == (1, K, 2)
    _check_against_the_definition(x, p, o, 0, K, 1)
    assert o["best"][0] == int(np.argmin(o["scores"][0]))
    if K == 1:
        assert o["best"][0] == 0 and np.array_equal(o["best_transform"][0], o["transforms"][0, 0])


@pytest.mark.parametrize("wp,wv", [(1.0, 0.0), (0.0, 1.0), (0.5, 2.0)])
def test_a_direction_of_weight_zero_is_skipped(wp, wv):
    c = rc.RECOVERY_CASES["cube5_skew15"]
    x, p = c["x"], c["p"][:100]
    V, S, K = len(x), len(p), 24
    al = _aligner(1, V, S)
    out = dict(vert_nn=torch.full((1, K, V), SENTINEL, dtype=torch.int32, device="cuda"),
               point_nn=torch.full((1, K, S), SENTINEL, dtype=torch.int32, device="cuda"))
    o = _host(al.align(dev(x[None]), dev(p[None]), iterations=2, w_point=wp, w_vert=wv, history=True, correspondences=True, out=out))
    # the skipped direction's output keeps what it held; the other one is written
    assert np.all(o["vert_nn"] == SENTINEL) == (wv == 0.0) and np.all(o["point_nn"] == SENTINEL) == (wp == 0.0)
    _check_against_the_definition(x, p, o, 0, K, 2, wp, wv)


@pytest.mark.parametrize("kind", ("coincident", "collinear"))
def test_rank_deficient_points_keep_the_rotation(kind):
    x = rc.lopsided_blob()
    p = rc.coincident_points() if kind == "coincident" else rc.collinear_points()
    I, K = 4, 24
    al = _aligner(1, len(x), len(p))
    o = _host(al.align(dev(x[None]), dev(p[None]), iterations=I, history=True))
    for k in ("transforms", "scores", "best_transform", "history"):
        assert np.isfinite(o[k]).all(), k
    assert np.all(o["kept_rotation"] == I)
    cube = hr.cube_rotations()
    for k in range(K):
        assert np.array_equal(o["transforms"][0, k].reshape(3, 4)[:, :3], cube[k])       # the start's rotation, bit for bit
    assert o["best"][0] == int(np.argmin(o["scores"][0]))


def test_a_handle_larger_than_the_call_gives_the_same_bits():
    cs, x, p = _batch()
    x, p = x[:2], p[:2, :97]
    tight = _aligner(2, x.shape[1], p.shape[1], 24)
    roomy = _aligner(5, x.shape[1] + 300, p.shape[1] + 1000, 64)
    a = _host(tight.align(dev(x), dev(p), iterations=3, history=True, correspondences=True))
    b = _host(roomy.align(dev(x), dev(p), iterations=3, history=True, correspondences=True))
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_a_refused_block_leaves_every_output_alone():
    c = rc.RECOVERY_CASES["identity"]
    x, p = dev(c["x"][None]), dev(c["p"][None])
    V, S, K = x.shape[1], p.shape[1], 24
    al = _aligner(1, V, S, 24)

    def sentinels(K=K, I=1):
        return dict(transforms=torch.full((1, K, 12), float(SENTINEL), device="cuda"), scores=torch.full((1, K), float(SENTINEL), device="cuda"),
                    best=torch.full((1,), SENTINEL, dtype=torch.int32, device="cuda"), best_transform=torch.full((1, 12), float(SENTINEL), device="cuda"),
                    kept_rotation=torch.full((1, K), SENTINEL, dtype=torch.int32, device="cuda"),
                    history=torch.full((1, K, I + 1), float(SENTINEL), device="cuda"))

    bad_start = np.eye(3, dtype=np.float32)[None].repeat(K, 0).copy()
    bad_start[5, 0, 0] = -1.0                                 # a reflection
    refused = [
        (dict(iterations=1001), "iterations must be 0..1000", 1001),
        (dict(iterations=1, w_point=0.0, w_vert=0.0), "w_point and w_vert are both 0", 1),
        (dict(iterations=1, w_vert=float("nan")), "w_point and w_vert must be finite and >= 0", 1),
        (dict(iterations=1, starts=bad_start), "every start must have determinant +1", 1),
        (dict(iterations=1, starts=np.eye(3, dtype=np.float32)[None].repeat(23, 0)), None, 1),       # K = 23 is fine with starts ...
        (dict(iterations=1, starts=bad_start, start_transforms=torch.zeros(1, K, 12, device="cuda")), "starts and start_transforms are both given", 1),
    ]
    for kw, text, I in refused:
        Kc = len(kw["starts"]) if kw.get("starts") is not None and "start_transforms" not in kw else K
        out = sentinels(Kc, I)
        if text is None:
            al.align(x, p, history=True, out=out, **kw)
            torch.cuda.synchronize()
            assert not bool((out["scores"] == SENTINEL).any())
            continue
        with pytest.raises(eng.SmalfitError, match=re.escape(text)):
            al.align(x, p, history=True, out=out, **kw)
        torch.cuda.synchronize()
        for k, v in out.items():
            assert bool((v == SENTINEL).all()), (text, k)
    # beyond the handle: more vertices, more meshes, more starts than it was created for
    small = _aligner(1, V - 1, S, 8)
    for kw, text in ((dict(), "num_verts must be 1 .. the aligner's max_verts"),):
        with pytest.raises(eng.SmalfitError, match=re.escape(text)):
            small.align(x, p, iterations=1)
    with pytest.raises(eng.SmalfitError, match="num_starts"):
        _aligner(1, V, S, 8).align(x, p, iterations=1)
    with pytest.raises(eng.SmalfitError, match="num_meshes"):
        al.align(torch.cat([x, x]), torch.cat([p, p]), iterations=1)
    # the Python layer's own shape and device checks
    with pytest.raises(eng.SmalfitError, match="points must be"):
        al.align(x, p[0], iterations=1)
    with pytest.raises(eng.SmalfitError, match="on the device of verts"):
        al.align(x, p.cpu(), iterations=1)
    with pytest.raises(eng.SmalfitError):
        eng.RigidAligner(1, 10, 10, 65)
    # a preallocated output of the right shape in the wrong place, or strided, is refused before its pointer is taken
    with pytest.raises(eng.SmalfitError, match="out\\['scores'\\] must be a contiguous tensor on the device"):
        al.align(x, p, iterations=1, out=dict(scores=torch.zeros(1, K)))
    with pytest.raises(eng.SmalfitError, match="out\\['transforms'\\] must be a contiguous tensor on the device"):
        al.align(x, p, iterations=1, out=dict(transforms=torch.zeros(1, 12, K, device="cuda").transpose(1, 2)))


# ---- the Python layer on the stand-in model -------------------------------------------------------------------------------------
def _turned_targets(md, N, seed):
    """the stand-in's posed meshes, each turned by a rotation of its own: back to front, and a cube rotation with a skew turn"""
    from smalify_amd.fitter_3d import TargetMeshes
    tv, tf = mc.target_meshes_from_smal(md, N, seed=seed)
    turns = [rc.axis_angle([0, 1, 0], 180.0), rc.cube_rotations()[9] @ rc.axis_angle([1, 2, -1], 12.0)]
    out = []
    for n, v in enumerate(tv):
        v = v.astype(np.float64) @ turns[n % 2].T
        v = v - v.mean(0)
        out.append((v / np.abs(v).max()).astype(np.float32))
    return out, tf, TargetMeshes(out, [tf] * N)


TURNS = (rc.axis_angle([0, 1, 0], 180.0), rc.cube_rotations()[9] @ rc.axis_angle([1, 2, -1], 12.0))


def test_rigid_prealign_folds_the_transform_into_the_parameters():
    from smalify_amd.fitter_3d import TargetMeshes, trainer
    md, fit, _ = mc.fitter_problem(2, seed=3)
    rs = np.random.RandomState(0)
    with torch.no_grad():
        fit.joint_rot.copy_(dev(0.1 * rs.randn(*fit.joint_rot.shape)))
        fit.global_rot.copy_(dev(0.3 * rs.randn(2, 3)))
        fit.trans.copy_(dev(0.2 * rs.randn(2, 3)))
        fit.betas.add_(dev(0.3 * rs.randn(*fit.betas.shape)))
    frozen = {k: getattr(fit, k).detach().clone() for k in ("betas", "joint_rot", "log_beta_scales", "deform_verts")}
    before = fit().cpu().numpy().astype(np.float64)
    # the targets: the fitter's own meshes, each turned by a rotation of its own (back to front; a cube rotation with a skew turn)
    # and moved -- the surfaces agree exactly under that motion and under no other
    moved = [(before[n] @ TURNS[n].T + [0.3, -0.2, 0.1]).astype(np.float32) for n in range(2)]
    targets = TargetMeshes(moved, [np.asarray(md.faces, np.int64)] * 2)
    report = trainer.rigid_prealign(fit, targets, num_points=600, seed=5)
    after = fit().cpu().numpy().astype(np.float64)
    assert len(report) == 2
    worst = 0.0
    for n, row in enumerate(report):
        R, t = _split(np.asarray(row["transform"]))
        extent = (before[n].max(0) - before[n].min(0)).max()
        worst = max(worst, np.abs(after[n] - (before[n] @ R.T + t)).max() / extent)
        assert 0 <= row["best"] < 24 and row["kept_rotation"] == 0 and np.isfinite(row["score"])
        assert row["score"] < row["identity_score"]
        assert abs(row["angle"] - rc.rotation_angle(R, np.eye(3))) <= 1e-5 and abs(np.degrees(row["angle"]) - row["angle_degrees"]) <= 1e-9
        # the mesh was turned to its target's orientation, not to one of the other 23 (each a quarter turn or more away)
        print("mesh", n, "best", row["best"], "score", row["score"], "identity", row["identity_score"], "off", rc.rotation_angle(R, TURNS[n]))
        assert rc.rotation_angle(R, TURNS[n]) < 0.3
    _judge("composition", worst, cap=COMPOSITION_CAP)
    for k, v in frozen.items():
        assert torch.equal(getattr(fit, k).detach(), v), k
    # deform_verts is added after the pose and would not turn with it
    with torch.no_grad():
        fit.deform_verts[1, 7, 2] = 1e-3
    with pytest.raises(ValueError, match="deform_verts"):
        trainer.rigid_prealign(fit, targets, iterations=1, num_points=64)
    with torch.no_grad():
        fit.deform_verts.zero_()
    with pytest.raises(ValueError, match="target meshes"):
        trainer.rigid_prealign(fit, TargetMeshes(moved[:1], [np.asarray(md.faces, np.int64)]), iterations=1, num_points=64)


def _write_meshes(tmp_path, tv, tf):
    mesh_dir = tmp_path / "meshes"
    mesh_dir.mkdir()
    for name, v in zip(("m0", "m1"), tv):
        with open(mesh_dir / (name + ".obj"), "w") as fh:
            for q in v * 3.0 + 0.5:                           # the loader re-centres and re-scales
                fh.write("v %.7f %.7f %.7f\n" % tuple(q))
            for f in tf:
                fh.write("f %d %d %d\n" % tuple(f + 1))
    return mesh_dir


def test_optimise_main_with_and_without_prealign(tmp_path, monkeypatch):
    from smalify_amd.fitter_3d import optimise, trainer
    md = mc.synthetic.synthetic_model(seed=0, shape_family_id=-1)
    tv, tf, _ = _turned_targets(md, 2, seed=9)
    mesh_dir = _write_meshes(tmp_path, tv, tf)

    def run(out, *flags):
        args = optimise.build_parser().parse_args(["--mesh_dir", str(mesh_dir), "--results_dir", str(tmp_path / out), "--scheme", "init",
                                                   "--nits", "3", "--lr", "0.05", "--seed", "4", "--no_plots", *flags])
        optimise.main(args, model_data=md, smal_data=mc.synthetic_smal_data())
        return np.load(tmp_path / out / "optimise.npz", allow_pickle=True)

    assert optimise.build_parser().parse_args([]).prealign is False
    # without the flag nothing of the aligner is constructed or called: this run would raise if it were
    with monkeypatch.context() as m:
        def never(*a, **k):
            raise AssertionError("the aligner was touched without --prealign")
        m.setattr(eng, "RigidAligner", never)
        m.setattr(trainer, "rigid_prealign", never)
        plain = run("plain")
    assert not os.path.exists(tmp_path / "plain" / "prealign.json")
    pre = run("pre", "--prealign", "--prealign_iterations", "8")
    doc = json.load(open(tmp_path / "pre" / "prealign.json"))
    assert doc["iterations"] == 8 and sorted(m["name"] for m in doc["meshes"]) == ["m0", "m1"]
    for row in doc["meshes"]:
        assert set(row) >= {"name", "best", "score", "angle", "angle_degrees", "kept_rotation", "identity_score", "transform"}
        assert row["score"] <= row["identity_score"]
    assert not np.array_equal(pre["global_rot"], plain["global_rot"])
    # ... and after the aligner has run in this process, a run without the flag still writes the bits of the first
    plain2 = run("plain2")
    for k in ("global_rot", "joint_rot", "betas", "log_beta_scales", "trans", "deform_verts", "verts", "faces"):
        assert np.array_equal(plain[k], plain2[k]), k
    # YAML: args: {prealign: true}
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("stages:\n  Stage0:\n    scheme: 'init'\n    nits: 2\n    lr: 0.05\nargs:\n  results_dir: %s\n  prealign: true\n"
                   "  prealign_iterations: 3\n" % (tmp_path / "yaml"))
    args = optimise.build_parser().parse_args(["--mesh_dir", str(mesh_dir), "--yaml_src", str(cfg), "--no_plots"])
    optimise.main(args, model_data=md, smal_data=mc.synthetic_smal_data())
    assert json.load(open(tmp_path / "yaml" / "prealign.json"))["iterations"] == 3
