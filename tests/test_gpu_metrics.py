"""The fit metrics on the device (smalfit_fit_metrics: cover_kernel, sil_counts_kernel, pck_kernel of kernels_color.inc behind
Engine.fit_metrics; the definitions are this project's, include/smalfit.h) (-m gpu):

  closed forms   the scenes of tests/metrics_cases.py: the four counts and the mask exactly
  binarisation   float targets at 0.5 and the next float above, byte targets at 127 and 128: the counts exactly
  whole mesh     strict <= mask <= relaxed pixel for pixel (oracle.smal_oracle.hard_phong_winners; tests/test_metrics_cpu.py caps
                 what lies between at 3 %), mask == (render_color != white), counts == numpy's on the returned mask
  frames, state  frame n of a 3- and a 9-frame call is the one-frame call, bit for bit; nothing of an earlier call survives
  PCK            counts exactly; distances against float64 on the same float32 inputs within 1e-6 relative (two subtractions,
                 hypot, the count's conversion, sqrt, the quotient: seven float32 roundings of at most 2 ulp ~ 8e-7).
                 Measured on MI355X: 2.0e-7 at most (T = 8; 1.2e-7 at T = 1 and 3; printed past the capture)
  refusals       every rule reaches smalfit_last_error(); the outputs are left alone
  fitters        FusedFitter.metrics, ImageBatchFitter.image_metrics, SMALFitter.metrics, fit_sequence(metrics=True)
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from smalify_amd import config as cfg                 # noqa: E402
from smalify_amd import engine as eng                 # noqa: E402
from smalify_amd import metrics as met                # noqa: E402
from smalify_amd import model_io, synthetic           # noqa: E402
from tests import color_cases as cc                   # noqa: E402
from tests import metrics_cases as mc                 # noqa: E402

FRAMES = 9
V_PAD = 3100           # smalfit_model_create wants the SMAL landmark vertex ids (up to 3055) to exist
DIST_BAR = 1e-6


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """a device error ends the session: nothing more is started on a GPU that has just faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:
        pytest.exit("device error, stopping: %s" % exc, returncode=3)


def _tiny_engine(faces, S, _cache={}):
    """tests/test_gpu_color.py::_anchor_engine with room for FRAMES frames: `faces` over V_PAD free vertices, no blend shapes,
    rigid skinning"""
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


def _call(e, verts, target, *kp, **kw):
    out = e.fit_metrics(verts, target, *kp, **kw)
    assert e.status() == 0
    return {k: v.cpu().numpy() for k, v in out.items()}


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ---- 1. closed forms ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", mc.SIZES)
@pytest.mark.parametrize("name", mc.SCENES)
def test_closed_form_coverage(name, S):
    sc = mc.scene(name, S)
    e = _tiny_engine(sc["faces"], S)
    verts = _pad(sc["verts"][None])
    for target in (sc["target"].astype(np.float32), sc["target"].astype(np.uint8) * 255):
        got = _call(e, verts, _dev(target[None]), want_mask=True)
        assert got["mask"].dtype == np.uint8 and set(np.unique(got["mask"])) <= {0, 1}
        assert np.array_equal(got["mask"][0].astype(bool), sc["mask"]), (name, S, int((got["mask"][0].astype(bool) ^ sc["mask"]).sum()))
        assert got["sil_counts"][0].tolist() == mc.counts(sc["mask"], sc["target"]).tolist()
    if name == "nothing":
        assert got["sil_counts"][0].tolist() == [0, int(sc["target"].sum()), 0, int(sc["target"].sum())]
        empty = _call(e, verts, _dev(np.zeros((1, S, S), np.float32)))
        assert empty["sil_counts"][0].tolist() == [0, 0, 0, 0]


# ---- 2. target binarisation --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", (16, 51))
def test_target_binarisation(S):
    """three frames of the same triangle (at 51^2 a frame's pixels start at no multiple of 16 bytes), another arrangement of the
    four values in each"""
    sc = mc.scene("single", S)
    e = _tiny_engine(sc["faces"], S)
    M = 3
    verts = _pad(np.repeat(sc["verts"][None], M, 0))
    p = mc.pattern(M, S)
    for values, on in ((mc.FLOAT_VALUES, mc.FLOAT_VALUES > 0.5), (mc.BYTE_VALUES, mc.BYTE_VALUES >= 128)):
        assert on.tolist() == [False, True, False, True]
        got = _call(e, verts, _dev(values[p]))
        want = mc.counts(np.broadcast_to(sc["mask"], (M, S, S)), on[p])
        assert got["sil_counts"].tolist() == want.tolist()
        assert len({tuple(r) for r in want.tolist()}) == M                    # the frames differ


# ---- 3. the whole mesh --------------------------------------------------------------------------------------------------
def _mesh_engine(S, _cache={}):
    if "dm" not in _cache:
        _cache["dm"] = eng.DeviceModel(cc.model("standin"))
    if S not in _cache:
        _cache[S] = eng.Engine(_cache["dm"], FRAMES, S)
    return _cache[S]


@pytest.mark.parametrize("view,S", [(v, S) for v in ("front", "shifted", "far") for S in cc.SIZES], ids=lambda x: str(x))
def test_whole_mesh(view, S):
    md, v = cc.view(view)
    sc = cc.scoring(view, S)
    strict, relaxed = sc["strict"], sc["relaxed"]
    target = np.roll(sc["exact"], 3, axis=-1)
    e = _mesh_engine(S)
    verts = _dev(v.astype(np.float32))
    got = _call(e, verts, _dev(target.astype(np.float32)), want_mask=True)
    mask = got["mask"].astype(bool)
    assert not (strict & ~mask).any() and not (mask & ~relaxed).any(), (int((strict & ~mask).sum()), int((mask & ~relaxed).sum()))
    img = e.render_color(verts, cc.COLOUR).cpu().numpy()
    assert np.array_equal(mask, ~(img == np.float32(1.0)).all(1))              # the metric scores what the collage shows
    want = mc.counts(mask, target)
    assert got["sil_counts"].tolist() == want.tolist()
    as_bytes = _call(e, verts, _dev(target.astype(np.uint8) * 255), want_mask=True)
    assert np.array_equal(as_bytes["mask"], got["mask"]) and as_bytes["sil_counts"].tolist() == want.tolist()
    # the target is the exact coverage moved by three columns: intersection < rendered, target < union (rendered and target
    # themselves are both the mesh's area, so they may agree)
    assert (want[:, 0] < want[:, 2:].min(1)).all() and (want[:, 2:].max(1) < want[:, 1]).all(), want
    lo, hi = mc.counts(strict, target), mc.counts(relaxed, target)
    assert (lo[:, :3] <= want[:, :3]).all() and (want[:, :3] <= hi[:, :3]).all() and (want[:, 3] == lo[:, 3]).all()


# ---- 4. frames and state ------------------------------------------------------------------------------------------------
def _nine_frames(S):
    """nine frames of the stand-in: the views of tests/color_cases.py one after the other; a target and keypoints per frame"""
    v = np.concatenate([cc.view(n)[1] for n in ("front", "far", "shifted", "turned")] + [cc.view("front")[1][:1]]).astype(np.float32)
    assert len(v) == 9
    rs = np.random.RandomState(3)
    target = np.zeros((9, S, S), np.float32)
    for n in range(9):
        r0, c0 = rs.randint(0, S // 2, 2)
        target[n, r0:r0 + S // 3 + n, c0:c0 + S // 4 + 2 * n] = 1.0
    proj = (S * rs.rand(9, 25, 2)).astype(np.float32)
    tj = (proj + 6.0 * rs.randn(9, 25, 2)).astype(np.float32)
    vis = mc.visibility(9, "mixed")
    return v, target, proj, tj, vis


def _same(a, b, rows=slice(None)):
    return all(a[k][rows].tobytes() == b[k].tobytes() for k in ("sil_counts", "mask", "keypoint_dist", "pck_counts")) and set(a) == set(b)


@pytest.mark.parametrize("S", (50, 128))
def test_frames_are_independent_and_nothing_survives_a_call(S):
    """50^2 = 2500 pixels: frames 1.. start at no multiple of 16 bytes, and the one-frame calls get slices of the tensors, whose
    addresses are not those of the many-frame call"""
    e = _mesh_engine(S)
    v, target, proj, tj, vis = _nine_frames(S)
    thr = mc.THRESHOLDS[3]
    for tgt in (target, (target * 255).astype(np.uint8)):
        full = [_dev(x) for x in (v, tgt, proj, tj, vis)]
        nine = _call(e, *full, thresholds=thr, want_mask=True)
        assert _same(nine, _call(e, *full, thresholds=thr, want_mask=True))                     # twice the same bits
        assert len({tuple(r) for r in nine["sil_counts"].tolist()}) >= 7
        three = _call(e, *[x[2:5].contiguous() for x in full], thresholds=thr, want_mask=True)
        assert _same(nine, three, slice(2, 5))
        for n in reversed(range(9)):
            one = _call(e, *[x[n:n + 1] for x in full], thresholds=thr, want_mask=True)          # slices: other alignments
            assert _same(nine, one, slice(n, n + 1)), n
    # `far` right after `front` on this engine against a fresh engine's: a stale mask or stale counters would show
    full = [_dev(x) for x in (v, target, proj, tj, vis)]
    _call(e, *[x[0:2].contiguous() for x in full], thresholds=thr, want_mask=True)
    after = _call(e, *[x[3:5].contiguous() for x in full], thresholds=thr, want_mask=True)
    fresh = _call(eng.Engine(e.model, 2, S), *[x[3:5].contiguous() for x in full], thresholds=thr, want_mask=True)
    assert _same(after, fresh) and after["sil_counts"][:, 2].min() > 0
    assert after["sil_counts"][:, 2].max() < nine["sil_counts"][0, 2]           # the far mesh covers less than the front one left behind


# ---- 5. PCK --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", sorted(mc.THRESHOLDS))
def test_pck(T, capsys):
    S, M = 50, 4
    sc = mc.scene("single", S)
    e = _tiny_engine(sc["faces"], S)
    verts = _pad(np.repeat(sc["verts"][None], M, 0))
    target = np.zeros((M, S, S), np.float32)
    target[0, 5:33, 10:35], target[2, 20:21, 3:44], target[3, 1:49, 2:27] = 1.0, 1.0, 1.0     # frame 1: an empty target
    areas = target.reshape(M, -1).sum(1).astype(np.int64)
    assert areas.tolist() == [700, 0, 41, 1200]
    thr = mc.THRESHOLDS[T]
    proj, tj = mc.pck_inputs(M, S, areas, thr)
    sil_only = _call(e, verts, _dev(target))
    assert set(sil_only) == {"sil_counts"} and sil_only["sil_counts"][:, 3].tolist() == areas.tolist()
    worst = 0.0
    for kind in ("all", "none", "mixed"):
        vis = mc.visibility(M, kind)
        dist, rows, clearance = mc.pck_expected(proj, tj, vis, areas, thr)
        assert clearance >= mc.PCK_CLEARANCE
        got = _call(e, verts, _dev(target), _dev(proj), _dev(tj), _dev(vis), thresholds=thr)
        assert got["pck_counts"].shape == (M, 1 + T) and got["pck_counts"].tolist() == rows.tolist(), kind
        assert got["sil_counts"].tolist() == sil_only["sil_counts"].tolist()      # the keypoints change nothing about the silhouette
        assert np.isposinf(got["keypoint_dist"][1]).all() and got["pck_counts"][1, 1:].tolist() == [0] * T
        if kind == "none":
            assert not got["pck_counts"].any()
        if kind == "all":
            assert got["pck_counts"][:, 0].tolist() == [25] * M
        have = areas > 0
        d, want = got["keypoint_dist"][have].astype(np.float64), dist[have]
        assert np.array_equal(d == 0.0, want == 0.0)                             # ratio 0: the projection itself
        nz = want > 0
        worst = max(worst, float((np.abs(d[nz] - want[nz]) / want[nz]).max()))
        # every distance is written, visible or not
        assert got["keypoint_dist"].tobytes() == _call(e, verts, _dev(target), _dev(proj), _dev(tj), _dev(mc.visibility(M, "all")),
                                                       thresholds=thr)["keypoint_dist"].tobytes()
    with capsys.disabled():
        print("\n[pck T=%d: keypoint_dist vs float64 on the same float32 inputs, largest relative deviation %.3e, bar %.0e]" % (T, worst, DIST_BAR))
    assert worst <= DIST_BAR, worst


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------
_CTX = {}


def _refusal_ctx():
    """an engine of mc.MAX frames at 16^2; every output a buffer of sevens"""
    if not _CTX:
        sc = mc.scene("single", 16)
        _CTX["e"] = eng.Engine(_tiny_engine(sc["faces"], 16).model, mc.MAX, 16)
        _CTX["verts"] = _pad(np.repeat(sc["verts"][None], mc.MAX + 1, 0))
        _CTX["buf"] = {k: torch.full(((mc.MAX + 1) * 16 * 16,), 7.0, device="cuda") for k in mc.POINTERS if k != "verts"}
    return _CTX


@pytest.mark.parametrize("name", [n for n, (_, text) in mc.REFUSALS.items() if text is not None])
def test_refusal_reaches_last_error(name):
    fields, text = mc.REFUSALS[name]
    c = _refusal_ctx()
    e = c["e"]
    pointers = dict({k: b.data_ptr() for k, b in c["buf"].items()}, verts=c["verts"].data_ptr())
    rc = e.lib.smalfit_fit_metrics(e.handle, eng._stream(), C.byref(mc.block(fields, pointers)))
    assert rc != 0
    assert e.lib.smalfit_last_error().decode() == "smalfit_fit_metrics: " + text
    torch.cuda.synchronize()
    assert all(bool((b == 7.0).all()) for b in c["buf"].values()) and e.status() == 0          # nothing was launched


def test_null_block_is_refused():
    e = _refusal_ctx()["e"]
    assert e.lib.smalfit_fit_metrics(e.handle, eng._stream(), None) != 0
    assert e.lib.smalfit_last_error().decode() == "smalfit_fit_metrics: null argument"


def test_python_layer_refuses_what_the_library_cannot_see():
    sc = mc.scene("single", 16)
    e = _tiny_engine(sc["faces"], 16)
    verts = _pad(sc["verts"][None])
    for bad in (torch.zeros(1, 8, 8, device="cuda"), torch.zeros(256, device="cuda"), torch.zeros(16, 1, 16, device="cuda"),
                torch.zeros(1, 16, 16, device="cuda", dtype=torch.float64), torch.zeros(1, 16, 16, device="cuda", dtype=torch.bool)):
        with pytest.raises(eng.SmalfitError, match="target_sil must be a"):
            e.fit_metrics(verts, bad)
    with pytest.raises(eng.SmalfitError, match="must be on the device of verts"):
        e.fit_metrics(verts, torch.zeros(1, 16, 16))
    with pytest.raises(eng.SmalfitError, match="keypoint tensors must be"):
        z = torch.zeros(1, 25, 2, device="cuda")
        e.fit_metrics(verts, torch.zeros(1, 16, 16, device="cuda"), z, z, torch.ones(25, device="cuda"))
    with pytest.raises(eng.SmalfitError, match="at most 8 thresholds"):
        e.fit_metrics(verts, torch.zeros(1, 16, 16, device="cuda"), thresholds=[0.1] * 9)
    with pytest.raises(eng.SmalfitError, match="every threshold must be finite and > 0"):
        z = torch.zeros(1, 25, 2, device="cuda")
        e.fit_metrics(verts, torch.zeros(1, 16, 16, device="cuda"), z, z, torch.ones(1, 25, device="cuda"), thresholds=[0.0])


# ---- 7. fitters ----------------------------------------------------------------------------------------------------------
def _bits(a, b):
    return set(a) == set(b) and all(a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes() for k in a)


def test_fused_fitter_metrics_is_fit_metrics_on_its_own_outputs():
    from smalify_amd import fitter as fit
    from tests import image_batch_cases as ic
    from tests import parity_cases as pc
    M, S = 2, 64
    e, _, _, tg = pc.make_problem(M, S, 2, seed=21)
    sp = synthetic.synthetic_shape_prior()
    f = fit.FusedFitter(e, tg["tj"], tg["vis"], tg["tsil"], 2, mean_betas=sp[1][:20], mean_log_scales=sp[1][20:26])
    for stage, iters in ((0, 3), (1, 2)):
        weights, _, lr = ic.stage_weights(stage)
        f.begin_stage(stage)
        f.run_iterations(weights, float(np.array(cfg.OPT_WEIGHTS).T[stage][6]), lr, stage, iters)
    losses = f.losses.clone()
    thr = (0.1, 0.15)
    got = f.metrics(thr, want_mask=True)
    assert torch.equal(f.losses, losses)                                       # the fit's loss vector is left alone
    verts, proj = torch.empty(M, e.model.num_verts, 3, device="cuda"), torch.empty(M, 25, 2, device="cuda")
    e.fit_eval(betas=f.p["betas"], log_beta_scales=f.p["log_beta_scales"], global_rotation=f.p["global_rotation"],
               joint_rotations=f.p["joint_rotations"], trans=f.p["trans"], target_joints=None, target_visibility=None, target_sil=None,
               weights=(0, 0, 0, 0, 0, 0), w_temp=0.0, window=2, temporal=False, grads={}, want=(), proj_out=proj, verts_out=verts)
    want = e.fit_metrics(verts, f.target_sil, proj, f.target_joints, f.visibility_full, thresholds=thr, want_mask=True)
    assert e.status() == 0 and _bits(got, want)
    snap_verts, _, snap_proj = f.snapshot()                                    # the collage's snapshot is of the same mesh
    assert torch.equal(snap_verts, verts) and float((snap_proj - proj).abs().max()) < 1e-3
    assert f.target_sil.dtype == torch.uint8                                   # a binary mask is stored as bytes: the byte path
    c = got["sil_counts"].cpu().numpy()
    assert (c[:, 3] == tg["tsil"].reshape(M, -1).sum(1)).all() and (c[:, 2] > 0).all() and (c[:, 0] > 0).all()
    assert got["pck_counts"][:, 0].tolist() == (tg["vis"] > 0).sum(1).tolist()
    s = met.summarise(got["sil_counts"], got["keypoint_dist"], f.visibility_full, thr)
    assert s["correct"].tolist() == got["pck_counts"][:, 1:].tolist()          # the host's float64 comparison agrees with the ballot
    assert ((s["iou"] > 0) & (s["iou"] <= 1)).all()


def test_image_metrics_row_is_the_row_of_a_batch_of_one():
    from smalify_amd import image_batch
    from tests import image_batch_cases as ic
    from tests import parity_cases as pc
    N, S = 3, 64
    e, _, sp = pc.get_engine(8, S)
    tg = ic.targets(ic.make_images(N, S))
    weights, _, lr = ic.stage_weights(1)

    def fitter(rows):
        return image_batch.ImageBatchFitter(e, tg["tj"][rows], tg["vis"][rows], tg["tsil"][rows], mean_betas=sp[1][:20], mean_log_scales=sp[1][20:26])

    f = fitter(slice(0, N))
    f.begin_stage(1)
    f.run_iterations(weights, 0.0, lr, 1, 3)
    batch = f.image_metrics((0.15, 0.3), want_mask=True)
    assert e.status() == 0 and tuple(batch["sil_counts"].shape) == (N, 4) and tuple(batch["pck_counts"].shape) == (N, 3)
    for n in range(N):
        g = fitter(slice(n, n + 1))                     # image n alone, at the parameters the batch's fit left it with
        for k in g.p:
            g.p[k].copy_(f.p[k][n:n + 1])
        alone = g.image_metrics((0.15, 0.3), want_mask=True)
        for k in batch:
            assert batch[k][n:n + 1].cpu().numpy().tobytes() == alone[k].cpu().numpy().tobytes(), (n, k)
    assert len({tuple(r) for r in batch["sil_counts"].tolist()}) == N and (batch["sil_counts"][:, 0] > 0).all()


def test_smal_fitter_metrics():
    """the drop-in's: the frames of a batch_range in its order, windows of batch_size per library call"""
    from tests import parity_cases as pc
    from smalify_amd.smal_fitter.smal_fitter import SMALFitter
    N, S = 3, 64
    _, cur, tg = pc.make_problem_cpu(N, S, 2, seed=21)
    data = (torch.zeros(N, 3, S, S), torch.from_numpy(tg["tsil"])[:, None], torch.from_numpy(tg["tj"]), torch.from_numpy(tg["vis"]))
    f = SMALFitter("cuda", data, 2, 1, True, model_data=synthetic.synthetic_model(seed=0, shape_family_id=1),
                   pose_prior_data=synthetic.synthetic_pose_prior(), shape_prior_data=synthetic.synthetic_shape_prior())
    with torch.no_grad():
        f.global_rotation.copy_(torch.from_numpy(cur["global_rotation"]))
        f.joint_rotations.copy_(torch.from_numpy(cur["joint_rotations"]))
        f.trans.copy_(torch.from_numpy(cur["trans"]))
    every = f.metrics(thresholds=(0.15,), want_mask=True)
    assert tuple(every["sil_counts"].shape) == (N, 4) and tuple(every["mask"].shape) == (N, S, S)
    c = every["sil_counts"].cpu().numpy()
    assert (c[:, 3] == tg["tsil"].reshape(N, -1).sum(1)).all() and (c[:, 0] > 0).all()
    picked = f.metrics([2, 0], thresholds=(0.15,), want_mask=True)
    assert all(picked[k].cpu().numpy().tobytes() == every[k][[2, 0]].cpu().numpy().tobytes() for k in every)
    # the mask is the collage's colour render of the same frames
    with torch.no_grad():
        theta = torch.cat([(f.global_rotation * f.global_mask).unsqueeze(1), f.joint_rotations * f.rotation_mask], dim=1)
        verts, _, _, _ = f.smal_model(f.betas.expand(N, 20).contiguous(), theta.contiguous(), betas_logscale=f.log_beta_scales.expand(N, 6).contiguous())
        img = f._engine(N).render_color((verts + f.trans.unsqueeze(1)).contiguous().float(), cc.COLOUR).cpu().numpy()
    assert np.array_equal(every["mask"].cpu().numpy().astype(bool), ~(img == np.float32(1.0)).all(1))


def test_fit_sequence_writes_metrics_json_only_when_asked(tmp_path, capsys):
    from smalify_amd.smal_fitter.optimize_to_joints import fit_sequence
    from tests import parity_cases as pc
    N, S = 2, 64
    _, _, tg = pc.make_problem_cpu(N, S, 2, seed=21)
    md = synthetic.synthetic_model(seed=0, shape_family_id=1)
    data = (np.zeros((N, 3, S, S), np.float32), tg["tsil"][:, None], tg["tj"], tg["vis"])
    names = ["frame_%02d.png" % i for i in range(N)]
    thr = (0.15, 0.3)
    runs = {}
    for on in (False, True):
        out = tmp_path / ("on" if on else "off")
        f = fit_sequence(data, names, md, synthetic.synthetic_pose_prior(), synthetic.synthetic_shape_prior(), output_dir=str(out),
                         window_size=2, iters_scale=0.01, **(dict(metrics=True, thresholds=thr) if on else {}))
        assert f.e.status() == 0
        runs[on] = (f, out, capsys.readouterr().out)
    f, out, text = runs[False]
    assert not os.path.exists(out / "metrics.json") and "IoU" not in text
    assert np.array_equal(runs[True][0].flat.cpu().numpy(), f.flat.cpu().numpy())              # asking changes nothing about the fit
    f, out, text = runs[True]
    assert [ln.split(":")[0] for ln in text.splitlines() if "IoU" in ln] == ["stage %d" % s for s in range(4)]
    doc = json.load(open(out / "metrics.json"))
    got = f.metrics(thr)
    want = met.report(met.summarise(got["sil_counts"], got["keypoint_dist"], f.visibility_full, thr), thr, names)
    assert json.dumps(doc, sort_keys=True) == json.dumps(want, sort_keys=True)
    assert list(doc["frames"]) == names and doc["thresholds"] == [0.15, 0.3]
    c = got["sil_counts"].cpu().numpy()
    assert [doc["frames"][n]["iou"] for n in names] == (c[:, 0] / c[:, 1]).tolist()
    assert doc["sequence"]["pck"] == (got["pck_counts"][:, 1:].sum(0).cpu().numpy() / got["pck_counts"][:, 0].sum().item()).tolist()


def test_fit_images_metrics_rows_follow_the_loader_across_batches(tmp_path, capsys):
    """three images in batches of two: metrics.json has one row per image under its file name, in the loader's order, and
    row n is the row of fitting image n's batch alone; without metrics=True no file and no line"""
    from smalify_amd.smal_fitter.optimize_to_joints import fit_images
    from tests import image_batch_cases as ic
    N, S = 3, 64
    tg = ic.targets(ic.make_images(N, S))
    md = synthetic.synthetic_model(seed=0, shape_family_id=1)
    names = ["img_%d.png" % i for i in (7, 3, 5)]
    thr = (0.15, 0.3)
    pp, sp = synthetic.synthetic_pose_prior(), synthetic.synthetic_shape_prior()

    def run(rows, out, **kw):
        data = (np.zeros((len(range(N)[rows]), 3, S, S), np.float32), tg["tsil"][rows][:, None], tg["tj"][rows], tg["vis"][rows])
        fit_images(data, names[rows], md, pp, sp, output_dir=str(out), iters_scale=0.01, max_batch=2, **kw)
        return capsys.readouterr().out

    text = run(slice(0, N), tmp_path / "off")
    assert not os.path.exists(tmp_path / "off" / "metrics.json") and "IoU" not in text
    text = run(slice(0, N), tmp_path / "on", metrics=True, thresholds=thr)
    lines = [ln.split(":")[0] for ln in text.splitlines() if "IoU" in ln]
    assert lines == ["images 0..1 stage %d" % s for s in range(4)] + ["images 2..2 stage %d" % s for s in range(4)]
    doc = json.load(open(tmp_path / "on" / "metrics.json"))
    assert list(doc["frames"]) == names and doc["thresholds"] == [0.15, 0.3]
    rows = {}
    for part, rows_of in (("a", slice(0, 2)), ("b", slice(2, 3))):                 # the two batches, each fitted on its own
        run(rows_of, tmp_path / part, metrics=True, thresholds=thr)
        rows.update(json.load(open(tmp_path / part / "metrics.json"))["frames"])
    assert json.dumps(doc["frames"], sort_keys=True) == json.dumps({n: rows[n] for n in names}, sort_keys=True)
    vis = sum(doc["frames"][n]["visible"] for n in names)
    assert vis == int((tg["vis"] > 0).sum()) and doc["sequence"]["visible"] == vis
    assert doc["sequence"]["pck"] == [sum(doc["frames"][n]["correct"][t] for n in names) / vis for t in range(2)]
    assert len({doc["frames"][n]["target"] for n in names}) == N
