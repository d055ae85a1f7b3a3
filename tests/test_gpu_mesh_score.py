"""smalfit_mesh_score on the device (mesh3d_surface_dist_kernel<0|1> and mesh3d_score_reduce_kernel of kernels_mesh3d.inc behind
MeshObjective.score; the definitions are this project's, include/smalfit.h) (-m gpu):

  branches      every branch of the query split (V in 3, 63, 64, 65, 130 -- a topology needs three vertices, so 3 stands for
                the issue's 1 -- and S in 1, 63, 64, 65, 130) and of the scan (1, 2, 3, 5 triangles: waves with an empty quarter;
                chunk - 1, chunk, chunk + 1, 2 chunk + 3, the chunk read from the plan through tests/host_mesh_score.py), in both
                roles, against the float64 brute force of tests/mesh_score_cases.py
  ragged        N = 3 targets of 1, chunk + 1 and 7 faces: row n is the one-mesh call on target n, bit for bit
  zeros         a mesh against itself, points that are its vertices: identically 0
  closed form   a cube against translated copies
  counts, sums  within == numpy's count on the returned distances, the maximum exactly, the sums within V 2^-24 relative, two
                calls the same bits, nothing of an earlier larger call survives
  one direction points = None: zero rows, the same vert_dist bits
  whole mesh    the stand-in SMAL mesh against a posed target, 3000 sampled points
  surface       refusals leave the outputs alone; Stage.metrics, StageManager.run(metrics=True), off by default

The bar on a distance: L = the largest coordinate magnitude of the queries and the scanned mesh (every pair's L is at most
that), deviation from float64 on the same float32 inputs in ulp(L) = 2^-23 L; at most 4 x the host shim's recorded worst
(tests/golden/hip_mesh_score_measured.json: shim/near_surface_ulp; the margin is for the device's own fma contraction) and at
most 3 x what these kernels measured when the file was written (device/*; SMALFIT_WRITE_MESH_SCORE_MEASURED=<path> writes it).
Every figure is printed before it is judged.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from smalify_amd import _lib, synthetic             # noqa: E402
from smalify_amd import engine as eng               # noqa: E402
from tests import host_mesh_score as hms            # noqa: E402
from tests import mesh3d_cases as m3                # noqa: E402
from tests import mesh_score_cases as mc            # noqa: E402

MEASURED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hip_mesh_score_measured.json")
CHUNK = hms.surface_chunk()
DEV = "cuda"


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """a device error ends the session: nothing more is started on a GPU that has just faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:
        pytest.exit("device error, stopping: %s" % exc, returncode=3)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def _judge(key, got32, want64, L_ulp):
    """print, record and judge one deviation in ulp(L)"""
    rec = json.load(open(MEASURED)) if os.path.exists(MEASURED) else {}
    dev = mc.deviation_ulp(got32, want64, L_ulp)
    bar = mc.DEVICE_FACTOR_OVER_SHIM * rec["shim/near_surface_ulp"]
    print("%-40s %8.3f ulp(L)   bar %.1f   recorded %s" % (key, dev, bar, rec.get("device/" + key)))
    path = os.environ.get("SMALFIT_WRITE_MESH_SCORE_MEASURED")
    if path:
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc["device/" + key] = dev
        json.dump(doc, open(path, "w"), indent=1, sort_keys=True)
    assert np.isfinite(np.asarray(got32)).all(), key
    assert dev <= bar, (key, dev, bar)
    if path:
        return                                     # a recording run: the ratchet is judged by the next run, against the file
    assert "device/" + key in rec, "tests/golden/hip_mesh_score_measured.json has no device/%s: run this file with " \
        "SMALFIT_WRITE_MESH_SCORE_MEASURED=<path> on a GPU box and commit the result" % key
    # (floor of 1 ulp(L): a recorded 0.3 must not turn a last-bit difference into a failure)
    assert dev <= max(mc.DEVICE_RATCHET * rec["device/" + key], 1.0), (key, dev, rec["device/" + key])


def _score(fit_verts, fit_faces, target_verts, target_faces, points=None, thresholds=(), max_points=130, objective=None):
    """fit_verts (N,V,3); targets: lists of N (verts, faces); points (N,S,3) or None -> (result dict on the host, objective)"""
    N, V = fit_verts.shape[:2]
    obj = objective or eng.MeshObjective(V, fit_faces, N, max_points)
    tg = eng.MeshTargets(target_verts, target_faces)
    o = obj.score(_t(fit_verts), tg, None if points is None else _t(points), thresholds)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}, obj


# ---- every branch of the query split and the scan -------------------------------------------------------------------------
# (V fitted vertices, S points, F faces of the target soup): the ribbon of V vertices has V - 2 faces, the scanned set of role 1
BRANCH_CASES = ((3, 1, 1), (4, 63, 2), (5, 64, 3), (7, 65, 5), (63, 130, CHUNK - 1), (64, 1, CHUNK), (65, 63, CHUNK + 1),
                (130, 64, 2 * CHUNK + 3), (CHUNK + 1, 65, 7), (CHUNK + 2, 130, 7), (CHUNK + 3, 5, 7), (2 * CHUNK + 5, 70, 9))


def test_the_cases_reach_every_branch():
    assert {c[0] for c in BRANCH_CASES} >= {3, 63, 64, 65, 130} and {c[1] for c in BRANCH_CASES} >= set(mc.QUERY_COUNTS)
    assert {c[2] for c in BRANCH_CASES} >= set(mc.scanned_counts(CHUNK))                 # role 0 scans the target
    assert {c[0] - 2 for c in BRANCH_CASES} >= set(mc.scanned_counts(CHUNK))             # role 1 scans the fitted mesh


@pytest.mark.parametrize("V,S,F", BRANCH_CASES)
def test_branches_against_float64(V, S, F):
    N = 2
    fit, faces, tv, tf, pts = [], None, [], [], []
    for n in range(N):
        v, faces = mc.ribbon(V, seed=100 * V + n)
        fit.append(v)
        sv, sf = mc.soup(F, seed=7 * F + S + n)
        tv.append(sv)
        tf.append(sf)
        pts.append(mc.points_near(sv, sf, S, seed=S + 3 * n))
    fit, pts = np.stack(fit), np.stack(pts)
    o, _ = _score(fit, faces, tv, tf, pts, thresholds=(0.05,))
    for n in range(N):
        want0 = mc.surface_dist(fit[n], tv[n], tf[n])
        want1 = mc.surface_dist(pts[n], fit[n], faces)
        _judge("branches/V%d_S%d_F%d/mesh%d/verts" % (V, S, F, n), o["vert_dist"][n], want0, mc.ulp_l(fit[n], tv[n]))
        _judge("branches/V%d_S%d_F%d/mesh%d/points" % (V, S, F, n), o["point_dist"][n], want1, mc.ulp_l(pts[n], fit[n]))


# ---- ragged targets ---------------------------------------------------------------------------------------------------------
def test_ragged_targets_read_their_own_slice():
    V = 130
    faces_of = (1, CHUNK + 1, 7)
    fit = np.stack([mc.ribbon(V, seed=40 + n)[0] for n in range(3)])
    faces = mc.ribbon(V, seed=0)[1]
    tv, tf = zip(*(mc.soup(F, seed=50 + n) for n, F in enumerate(faces_of)))
    assert len({len(v) for v in tv}) == 3                                             # different vertex counts too
    pts = np.stack([mc.points_near(tv[n], tf[n], 70, seed=60 + n) for n in range(3)])
    o, _ = _score(fit, faces, list(tv), list(tf), pts, thresholds=(0.02, 0.1))
    for n in range(3):
        one, _ = _score(fit[n:n + 1], faces, [tv[n]], [tf[n]], pts[n:n + 1], thresholds=(0.02, 0.1))
        for k in ("vert_dist", "point_dist", "sums", "within"):
            assert np.array_equal(o[k][n].view(np.int32), one[k][0].view(np.int32)), (n, k)
        _judge("ragged/mesh%d/verts" % n, o["vert_dist"][n], mc.surface_dist(fit[n], tv[n], tf[n]), mc.ulp_l(fit[n], tv[n]))


# ---- exact zeros ------------------------------------------------------------------------------------------------------------
def test_a_mesh_against_itself_is_identically_zero():
    rv, rf = mc.ribbon(130, seed=8)
    cv = np.concatenate([mc.CUBE_VERTS * np.float32(0.37) + np.float32(0.11), rv[:122]])          # 130 vertices, cube + strip
    cf = np.concatenate([mc.CUBE_FACES, mc.ribbon(122, seed=8)[1] + 8]).astype(np.int32)
    for v, f in ((rv, rf), (cv, cf)):
        o, _ = _score(v[None], f, [v], [f], v[None])
        assert (o["vert_dist"] == 0.0).all() and (o["point_dist"] == 0.0).all()
        assert (o["sums"] == 0.0).all()


# ---- closed-form batch ------------------------------------------------------------------------------------------------------
def test_cube_against_translated_copies():
    N = len(mc.CUBE_SHIFTS)
    fit = np.repeat(mc.CUBE_VERTS[None], N, 0)
    tv = [mc.CUBE_VERTS + s for s in mc.CUBE_SHIFTS]
    pts = np.stack(tv)                                                                # the targets' corners lie on the targets
    o, _ = _score(fit, mc.CUBE_FACES, tv, [mc.CUBE_FACES] * N, pts, max_points=8)
    for n, s in enumerate(mc.CUBE_SHIFTS):
        want0 = mc.box_surface_dist(mc.CUBE_VERTS, s, s + 1.0)
        want1 = mc.box_surface_dist(tv[n], np.zeros(3), np.ones(3))
        _judge("cube/shift%d/verts" % n, o["vert_dist"][n], want0, mc.ulp_l(fit[n], tv[n]))
        _judge("cube/shift%d/points" % n, o["point_dist"][n], want1, mc.ulp_l(fit[n], tv[n]))
    # corner (1,1,0) lies inside the first copy, an eighth above its bottom face: a dyadic plane distance, exact in float32
    assert o["vert_dist"][0][6] == np.float32(0.125)


# ---- counts and sums --------------------------------------------------------------------------------------------------------
def _counts_problem():
    V, N = 130, 2
    fit = np.stack([mc.ribbon(V, seed=20 + n)[0] for n in range(N)])
    faces = mc.ribbon(V, seed=0)[1]
    tv, tf = zip(*(mc.soup(40 + n, seed=30 + n) for n in range(N)))
    return fit, faces, list(tv), list(tf)


@pytest.mark.parametrize("T", (1, 3, 8))
def test_counts_and_sums(T):
    fit, faces, tv, tf = _counts_problem()
    N, V = fit.shape[:2]
    S = 130
    pts = np.stack([mc.points_near(tv[n], tf[n], S, seed=70 + n, sigma=0.05) for n in range(N)])
    first, obj = _score(fit, faces, tv, tf, pts)
    # thresholds from the distances themselves: some exactly ON a returned distance (d <= t counts it), one below all, one above
    d_all = np.sort(np.concatenate([first["vert_dist"].ravel(), first["point_dist"].ravel()]))
    picks = [d_all[len(d_all) // 2], d_all[0] * np.float32(0.5) + np.float32(1e-9), d_all[-1] * np.float32(2), d_all[len(d_all) // 4],
             d_all[3 * len(d_all) // 4], np.float32(0.01), np.float32(0.03), d_all[len(d_all) // 8]]
    thr = tuple(float(np.float32(t)) for t in picks[:T])
    o, _ = _score(fit, faces, tv, tf, pts, thresholds=thr, objective=obj)
    again, _ = _score(fit, faces, tv, tf, pts, thresholds=thr, objective=obj)
    for k in o:
        assert np.array_equal(o[k].view(np.int32), again[k].view(np.int32)), k                    # two calls, the same bits
        if k in first:
            assert np.array_equal(o[k].view(np.int32), first[k].view(np.int32)), k                # thresholds change nothing else
    assert o["within"].shape == (N, 2, T) and o["within"].dtype == np.int32
    for n in range(N):
        for d, dist in enumerate((o["vert_dist"][n], o["point_dist"][n])):
            for t in range(T):
                assert o["within"][n, d, t] == int((dist <= np.float32(thr[t])).sum()), (n, d, t)
            assert o["sums"][n, d, 2] == dist.max()
            s1, s2 = dist.astype(np.float64).sum(), (dist.astype(np.float64) ** 2).sum()
            rel = len(dist) * 2.0 ** -24                     # the worst case of ANY order of float32 sums of non-negative terms
            print("sums mesh %d dir %d: rel err %.2e %.2e (bar %.2e)" % (n, d, abs(o["sums"][n, d, 0] - s1) / s1,
                                                                         abs(o["sums"][n, d, 1] - s2) / s2, rel))
            assert abs(o["sums"][n, d, 0] - s1) <= rel * s1 and abs(o["sums"][n, d, 1] - s2) <= rel * s2
    if T == 3:
        assert 0 < o["within"][..., 0].sum() < N * (V + S)                                        # the median splits the queries
        assert (o["within"][..., 1] == 0).all() and (o["within"][:, 0, 2] == V).all() and (o["within"][:, 1, 2] == S).all()


def test_nothing_of_an_earlier_call_survives():
    fit, faces, tv, tf = _counts_problem()
    N = len(fit)
    big = np.stack([mc.points_near(tv[n], tf[n], 130, seed=80 + n) for n in range(N)])
    small = np.stack([mc.points_near(tv[n], tf[n], 70, seed=90 + n) for n in range(N)])
    thr = (0.01, 0.04)
    _, used = _score(fit, faces, tv, tf, big, thresholds=thr)
    after, _ = _score(fit, faces, tv, tf, small, thresholds=thr, objective=used)
    fresh, _ = _score(fit, faces, tv, tf, small, thresholds=thr)
    for k in fresh:
        assert after[k].shape == fresh[k].shape and np.array_equal(after[k].view(np.int32), fresh[k].view(np.int32)), k
    # ... nor of a call with points in a call without: the rows of direction 1 are zero, not the earlier call's
    none, _ = _score(fit, faces, tv, tf, None, thresholds=thr, objective=used)
    assert (none["sums"][:, 1] == 0).all() and (none["within"][:, 1] == 0).all()


def test_one_direction_only():
    fit, faces, tv, tf = _counts_problem()
    N = len(fit)
    pts = np.stack([mc.points_near(tv[n], tf[n], 65, seed=95 + n) for n in range(N)])
    both, obj = _score(fit, faces, tv, tf, pts, thresholds=(0.02,))
    one, _ = _score(fit, faces, tv, tf, None, thresholds=(0.02,), objective=obj)
    assert "point_dist" not in one
    assert np.array_equal(one["vert_dist"].view(np.int32), both["vert_dist"].view(np.int32))
    assert np.array_equal(one["sums"][:, 0].view(np.int32), both["sums"][:, 0].view(np.int32))
    assert np.array_equal(one["within"][:, 0], both["within"][:, 0])
    assert (one["sums"][:, 1].view(np.int32) == 0).all() and (one["within"][:, 1] == 0).all()
    assert (both["sums"][:, 1, 0] > 0).all()


# ---- whole mesh, once -------------------------------------------------------------------------------------------------------
def test_whole_mesh_against_float64():
    md = synthetic.synthetic_model(seed=0, shape_family_id=-1)
    fit = np.asarray(md.v_template, np.float32)
    fit = ((fit - fit.mean(0)) / np.abs(fit - fit.mean(0)).max()).astype(np.float32)[None]        # normalised like the targets
    faces = np.asarray(md.faces, np.int32)
    tv, tf = m3.target_meshes_from_smal(md, 1, seed=4)
    assert fit.shape[1] == 3889 and len(tf) == 7774
    obj = eng.MeshObjective(3889, faces, 1, 3000)
    tg = eng.MeshTargets(tv, [tf])
    pts = tg.sample(3000, 17, 0)
    o = obj.score(_t(fit), tg, pts, (0.01, 0.05))
    torch.cuda.synchronize()
    p = pts.cpu().numpy()
    want0 = mc.surface_dist_culled(fit[0], tv[0], tf)
    want1 = mc.surface_dist_culled(p[0], fit[0], faces)
    _judge("whole/verts", o["vert_dist"].cpu().numpy()[0], want0, mc.ulp_l(fit, tv[0]))
    _judge("whole/points", o["point_dist"].cpu().numpy()[0], want1, mc.ulp_l(p, fit))
    s = o["sums"].cpu().numpy()[0]
    assert want0.mean() > 1e-3 and want1.mean() > 1e-3                                    # a posed target: not a fit at all
    for d, k in enumerate(("vert_dist", "point_dist")):
        got = o[k].cpu().numpy()[0].astype(np.float64)
        assert abs(s[d, 0] - got.sum()) <= len(got) * 2.0 ** -24 * got.sum() and s[d, 2] == got.max()
    w = o["within"].cpu().numpy()[0]
    assert (w[:, 0] <= w[:, 1]).all() and w[0, 1] <= 3889 and w[1, 1] <= 3000


# ---- the surface ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone():
    fit, faces, tv, tf = _counts_problem()
    N, V = fit.shape[:2]
    obj = eng.MeshObjective(V, faces, N, 70)
    tg = eng.MeshTargets(tv, tf)
    verts, pts = _t(fit), _t(np.stack([mc.points_near(tv[n], tf[n], 70, seed=n) for n in range(N)]))
    # through the wrapper: an error is raised
    with pytest.raises(eng.SmalfitError, match="1 <= num_points <= max_points"):
        obj.score(verts, tg, _t(np.zeros((N, 71, 3))))
    with pytest.raises(eng.SmalfitError, match="number of target meshes differs"):
        obj.score(verts, eng.MeshTargets(tv[:1], tf[:1]), pts)
    with pytest.raises(eng.SmalfitError, match="num_meshes exceeds"):
        obj.score(_t(np.zeros((N + 1, V, 3))), tg)
    with pytest.raises(eng.SmalfitError, match="finite and > 0"):
        obj.score(verts, tg, pts, thresholds=(0.1, 0.0))
    with pytest.raises(eng.SmalfitError, match="at most 8 thresholds"):
        obj.score(verts, tg, pts, thresholds=(0.1,) * 9)
    with pytest.raises(eng.SmalfitError):
        obj.score(verts[:, :-1].contiguous(), tg, pts)
    # through the C-ABI: every rule's text reaches smalfit_last_error and no output is written
    lib = _lib.load()
    fn = _lib.resolve(lib, "smalfit_mesh_score")
    out = dict(vert_dist=torch.full((N, V), -7.0, device=DEV), point_dist=torch.full((N, 70), -7.0, device=DEV),
               sums=torch.full((N, 2, 3), -7.0, device=DEV), within=torch.full((N, 2, 3), -7, dtype=torch.int32, device=DEV))

    def block():
        a = mc.valid_args(N=N, S=70, T=3)
        a.verts, a.points = verts.data_ptr(), pts.data_ptr()
        for k, v in out.items():
            setattr(a, k, v.data_ptr())
        return a
    for name, change, targets, text in mc.REFUSALS:
        a = block()
        change(a)
        if a.num_meshes > N:                       # (the capacity of THIS objective)
            a.num_meshes = N + 1
        t = tg if targets is None or a.num_meshes > N else eng.MeshTargets(tv[:targets], tf[:targets])
        assert fn(obj.handle, t.handle, eng._stream(), C.byref(a)) != 0, name
        assert lib.smalfit_last_error().decode() == "smalfit_mesh_score: " + text, name
    assert fn(None, tg.handle, eng._stream(), C.byref(block())) != 0 and b"null argument" in lib.smalfit_last_error()
    assert fn(obj.handle, None, eng._stream(), C.byref(block())) != 0 and b"null argument" in lib.smalfit_last_error()
    assert fn(obj.handle, tg.handle, eng._stream(), None) != 0 and b"null argument" in lib.smalfit_last_error()
    torch.cuda.synchronize()
    for k, v in out.items():
        assert (v == -7).all(), k
    # and the accepted block writes all four
    assert fn(obj.handle, tg.handle, eng._stream(), C.byref(block())) == 0
    torch.cuda.synchronize()
    assert (out["vert_dist"] >= 0).all() and (out["point_dist"] >= 0).all() and (out["sums"] >= 0).all() and (out["within"] >= 0).all()


def test_stage_metrics_changes_no_later_step():
    from smalify_amd.fitter_3d import Stage
    results = []
    for scored in (True, False):
        md, fit, targets = m3.fitter_problem(2, seed=6)
        stage = Stage(8, "default", fit, targets, lr=0.02, custom_lrs=m3.DEFAULT_CUSTOM_LRS, seed=11)
        for it in range(6):
            stage.step(it)
        if scored:
            s = stage.metrics(thresholds=(0.02, 0.1))
            for k in ("vert_mean", "vert_rms", "vert_max", "point_mean", "point_rms", "point_max", "hausdorff", "chamfer_l2"):
                assert s[k].shape == (2,) and np.isfinite(s[k]).all() and (s[k] > 0).all(), k
            for k in ("precision", "recall", "fscore"):
                assert s[k].shape == (2, 2) and np.isfinite(s[k]).all() and (s[k] >= 0).all() and (s[k] <= 1).all(), k
            assert (s["vert_mean"] <= s["vert_rms"]).all() and (s["vert_rms"] <= s["vert_max"]).all()
            assert (s["hausdorff"] == np.maximum(s["vert_max"], s["point_max"])).all()
            # a score is a function of the fit alone: the same figures again, and with a seed of the caller's other points
            s2 = stage.metrics(thresholds=(0.02, 0.1))
            assert all(np.array_equal(s[k], s2[k]) for k in ("vert_mean", "point_mean", "fscore"))
            s3 = stage.metrics(thresholds=(0.02, 0.1), seed=5)
            assert np.array_equal(s3["vert_mean"], s["vert_mean"]) and not np.array_equal(s3["point_mean"], s["point_mean"])
            s4 = stage.metrics(thresholds=(), num_points=0)
            assert np.array_equal(s4["vert_mean"], s["vert_mean"]) and np.isnan(s4["point_mean"]).all()
        loss = stage.step(6).clone()
        torch.cuda.synchronize()
        results.append((loss.cpu().numpy(), {k: getattr(fit, k).detach().cpu().numpy().copy() for k in
                                             ("betas", "global_rot", "joint_rot", "trans", "deform_verts")},
                        stage.last_points.cpu().numpy().copy()))
    (la, pa, qa), (lb, pb, qb) = results
    assert np.array_equal(la.view(np.int32), lb.view(np.int32))
    assert np.array_equal(qa.view(np.int32), qb.view(np.int32))
    for k in pa:
        assert np.array_equal(pa[k].view(np.int32), pb[k].view(np.int32)), k


def test_stage_manager_writes_metrics_json_when_asked(tmp_path):
    from smalify_amd.fitter_3d import Stage, StageManager
    for asked in (False, True):
        out_dir = tmp_path / ("with" if asked else "without")
        md, fit, targets = m3.fitter_problem(2, seed=3)
        mgr = StageManager(out_dir=str(out_dir), labels=["a", "b"])
        mgr.add_stage(Stage(4, "init", fit, targets, name="Stage0", lr=0.05, out_dir=str(out_dir), mesh_names=["a", "b"]))
        if asked:
            mgr.run(plot=False, progress=False, metrics=True, metric_thresholds=(0.02, 0.1))
        else:
            mgr.run(plot=False, progress=False)
        assert os.path.exists(out_dir / "Stage0.npz")
        assert os.path.exists(out_dir / "metrics.json") == asked
        if asked:
            doc = json.load(open(out_dir / "metrics.json"))
            rows = doc["stages"]["Stage0"]["meshes"]
            assert list(rows) == ["a", "b"] and doc["stages"]["Stage0"]["thresholds"] == [0.02, 0.1]
            for row in rows.values():
                assert row["hausdorff"] > 0 and len(row["fscore"]) == 2
            assert doc["stages"]["Stage0"]["batch"]["meshes"] == 2
            assert sorted(np.load(out_dir / "Stage0.npz", allow_pickle=True).files) == sorted(
                ["global_rot", "joint_rot", "betas", "log_beta_scales", "trans", "deform_verts", "verts", "faces", "labels"])
