"""GPU: SMALFitter(..., epoch_evaluation=True) -- the reference's per-window loop served from ONE evaluation of the whole sequence
per epoch (smalfit_fit_eval_windows): the reference's recorded trajectory (golden G8), values and gradients against the float64
oracle with a silhouette and under non-uniform upstream weights, every event that must turn the cached evaluation over, and the
calls that must not use it."""
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import smal_oracle as so  # noqa: E402
from smalify_amd import config as cfg  # noqa: E402
from smalify_amd import synthetic  # noqa: E402
from tests import parity_cases as pc  # noqa: E402
from tests.parity_cases import rel  # noqa: E402

PARAMS = ("global_rotation", "joint_rotations", "trans", "betas", "log_beta_scales")
W_TABLE = np.array(cfg.OPT_WEIGHTS).T


@pytest.fixture(scope="module")
def md():
    return synthetic.synthetic_model(seed=0, shape_family_id=1)


def _golden_fitter(golden, md, window, epoch, frames=None):
    from smalify_amd.smal_fitter.smal_fitter import SMALFitter
    tj, vis = golden["g6_target_joints"], golden["g6_visibility"]
    if frames is not None:
        reps = (frames + tj.shape[0] - 1) // tj.shape[0]
        tj, vis = np.concatenate([tj] * reps)[:frames], np.concatenate([vis] * reps)[:frames]
    N, S = tj.shape[0], int(golden["g6_image_size"])
    data = (torch.zeros(N, 3, S, S), torch.zeros(N, 1, S, S), torch.from_numpy(tj), torch.from_numpy(vis))
    f = SMALFitter("cuda", data, window, 1, True, model_data=md,
                   pose_prior_data=(golden["pose_prec"], golden["pose_mean"], golden["pose_mask"]),
                   shape_prior_data=(golden["unity_prec"], golden["unity_mean"]), epoch_evaluation=epoch)
    rs = np.random.RandomState(9)                      # away from the symmetric start: every gradient is alive
    with torch.no_grad():
        f.joint_rotations.add_(torch.from_numpy((0.1 * rs.randn(N, 34, 3)).astype(np.float32)).cuda())
        f.trans.add_(torch.from_numpy((0.02 * rs.randn(N, 3)).astype(np.float32)).cuda())
    return f


def _windows(f):
    N, B = f.num_images, f.batch_size
    return [list(range(j, min(N, j + B))) for j in range(0, N, B)]


def _grads(f):
    return {k: None if getattr(f, k).grad is None else getattr(f, k).grad.detach().cpu().numpy().copy() for k in PARAMS}


def _epoch(f, weights, stage_id=1, w_temp=None, upstream=None):
    """one epoch of the reference's loop without the optimiser: -> (window losses as floats, objs of the last window, grads)"""
    for k in PARAMS:
        getattr(f, k).grad = None
    acc, vals, objs = 0, [], None
    for i, br in enumerate(_windows(f)):
        loss, objs = f(br, weights, stage_id)
        vals.append(loss)
        acc = acc + (1.0 if upstream is None else upstream[i]) * loss.mean()
    if w_temp is not None:
        jl, gl, tl = f.get_temporal(w_temp)
        acc = acc + jl + gl + tl
    acc.backward()
    return [float(v.detach()) for v in vals], objs, _grads(f)


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            assert np.array_equal(a[k], b[k]), k


def _reference_style_loop(f, golden, vis_full, window=2):
    """tests/test_gpu_dropin.py's restatement of the reference's driver (optimize_to_joints.py:90-137), restated"""
    hist, snaps, N, epochs = [], {}, f.num_images, 0
    for stage_id, its in golden["g8_schedule"]:
        weights = (golden["g6_w0"] if stage_id == 0 else golden["g6_w1"])
        w_temp, lr = W_TABLE[stage_id][6], W_TABLE[stage_id][8]
        opt = torch.optim.Adam(f.parameters(), lr=lr, betas=(0.5, 0.999))
        if stage_id == 0:
            f.joint_rotations.requires_grad = False
            f.betas.requires_grad = False
            f.log_beta_scales.requires_grad = False
            tv = f.target_visibility.clone()
            f.target_visibility *= 0
            f.target_visibility[:, cfg.TORSO_JOINTS] = tv[:, cfg.TORSO_JOINTS]
        else:
            f.joint_rotations.requires_grad = True
            f.betas.requires_grad = True
            f.log_beta_scales.requires_grad = True
            f.target_visibility = vis_full.clone()          # CPU float tensor, like data[-1].clone()
        for _ in range(int(its)):
            acc = 0
            opt.zero_grad()
            for j in range(0, N, window):
                loss, _ = f(list(range(j, min(N, j + window))), weights, stage_id)
                acc = acc + loss.mean()
            jl, gl, tl = f.get_temporal(w_temp)
            acc = acc + jl + gl + tl
            acc.backward()
            opt.step()
            hist.append(acc.item())
            epochs += 1
            if stage_id == 0:
                assert f.betas.grad is None and f.joint_rotations.grad is None and f.log_beta_scales.grad is None
        snaps[int(stage_id)] = {k: getattr(f, k).detach().cpu().numpy().copy() for k in PARAMS}
    return hist, snaps, epochs


def test_reference_loop_reproduces_the_reference_trajectory_with_one_evaluation_per_epoch(golden, md):
    from smalify_amd.smal_fitter.smal_fitter import SMALFitter
    N, S = golden["g6_target_joints"].shape[0], int(golden["g6_image_size"])

    def make(epoch):
        data = (torch.zeros(N, 3, S, S), torch.zeros(N, 1, S, S), torch.from_numpy(golden["g6_target_joints"]), torch.from_numpy(golden["g6_visibility"]))
        return SMALFitter("cuda", data, 2, 1, True, model_data=md, pose_prior_data=(golden["pose_prec"], golden["pose_mean"], golden["pose_mask"]),
                          shape_prior_data=(golden["unity_prec"], golden["unity_mean"]), epoch_evaluation=epoch)

    f = make(True)
    hist, snaps, epochs = _reference_style_loop(f, golden, torch.from_numpy(golden["g6_visibility"]))
    assert np.allclose(hist, golden["g8_loss_history"], rtol=5e-4), (hist, golden["g8_loss_history"])
    for stage in (0, 1):
        for k, v in snaps[stage].items():
            r = rel(v, golden["g8_after_stage%d_%s" % (stage, k)])
            assert r < 5e-4, (stage, k, r)
    assert f.engine_evaluations == epochs
    twin = make(False)
    _reference_style_loop(twin, golden, torch.from_numpy(golden["g6_visibility"]))
    assert twin.engine_evaluations == epochs * ((N + 1) // 2)
    # the switch can also sit in the config module a four-import user already has
    assert make(None).epoch_evaluation is False
    cfg.EPOCH_EVALUATION = True
    try:
        assert make(None).epoch_evaluation is True and make(False).epoch_evaluation is False
    finally:
        cfg.EPOCH_EVALUATION = False


# ---- against the oracle, with a silhouette ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sil_case(md):
    """M = 4, S = 64, windows of 2, stage-2 weights: a flag-on fitter at the perturbed state of tests/parity_cases.py"""
    from smalify_amd.smal_fitter.smal_fitter import SMALFitter
    M, S, window = 4, 64, 2
    prob, cur, tg = pc.make_problem_cpu(M, S, window, seed=21, with_sil=True)
    pp, sp = synthetic.synthetic_pose_prior(), synthetic.synthetic_shape_prior()
    data = (torch.zeros(M, 3, S, S), torch.from_numpy(tg["tsil"]).reshape(M, 1, S, S), torch.from_numpy(tg["tj"]), torch.from_numpy(tg["vis"]))

    def make(epoch=True):
        f = SMALFitter("cuda", data, window, 1, True, model_data=md, pose_prior_data=pp, shape_prior_data=sp, epoch_evaluation=epoch)
        with torch.no_grad():
            for k, v in cur.items():
                getattr(f, k).copy_(torch.from_numpy(v))
        return f

    return dict(prob=prob, cur=cur, make=make, weights=W_TABLE[2][:6].copy(), w_temp=float(W_TABLE[2][6]), window=window, M=M)


def _oracle_expression(c, upstream, w_temp):
    """autograd of sum_w upstream[w] * window_loss_w (+ temporal) in float64 -> (window totals, grads)"""
    leaf = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in c["cur"].items()}
    acc, totals = 0.0, []
    for (br, full, owned), u in zip(c["prob"].window_groups(), upstream):
        tot, _ = so.window_loss(c["prob"], leaf, br, c["weights"], None, None, full, owned)
        totals.append(float(tot.detach()))
        if u:
            acc = acc + u * tot
    if w_temp is not None:
        acc = acc + sum(so.temporal_terms(leaf, w_temp))
    acc.backward()
    return totals, {k: None if v.grad is None else v.grad.numpy() for k, v in leaf.items()}


def test_window_losses_and_epoch_gradients_with_a_silhouette(sil_case):
    c = sil_case
    f = c["make"]()
    vals, objs, grads = _epoch(f, c["weights"], 2, w_temp=c["w_temp"])
    totals_o, grads_o = _oracle_expression(c, (1.0, 1.0), c["w_temp"])
    assert f.engine_evaluations == 1
    for w, (v, o) in enumerate(zip(vals, totals_o)):
        print("window", w, "loss rel", abs(v - o) / abs(o))
        assert abs(v - o) / abs(o) < 1e-4, (w, v, o)
    for k in PARAMS:
        print(k, "grad rel", rel(grads[k], grads_o[k]))
        assert rel(grads[k], grads_o[k]) < 2e-3, k
    assert sorted(objs) == ["betas", "joint", "pose", "sil_reproj", "splay"]
    assert all(not v.requires_grad and v.dim() == 0 for v in objs.values())
    assert abs(sum(float(v) for v in objs.values()) - vals[-1]) < 1e-5 * abs(vals[-1])


@pytest.mark.parametrize("upstream", [(1.0, 3.0), (0.0, 1.0)])
def test_non_uniform_upstream_weights(sil_case, upstream):
    """(1 L0 + 3 L1).backward() and L1.backward() alone: every window's own share of the shared gradients is handed out -- the
    summed shared gradient would fail both"""
    c = sil_case
    f = c["make"]()
    losses = [f(br, c["weights"], 2)[0] for br in _windows(f)]
    if upstream == (0.0, 1.0):
        losses[1].backward()
    else:
        (upstream[0] * losses[0] + upstream[1] * losses[1]).backward()
    assert f.engine_evaluations == 1
    _, grads_o = _oracle_expression(c, upstream, None)
    grads = _grads(f)
    for k in PARAMS:
        print(upstream, k, "grad rel", rel(grads[k], grads_o[k]))
        assert rel(grads[k], grads_o[k]) < 2e-3, k
    if upstream == (0.0, 1.0):        # frames of the window that was not asked for: exactly nothing
        assert not grads["trans"][:2].any() and not grads["joint_rotations"][:2].any()


# ---- the cached evaluation turns over exactly when it must ------------------------------------------------------------
def _checkpoint(tmp_path, f, golden):
    keys = ("betas", "global_rotation", "joint_rotations", "log_betascale", "trans")
    for i in range(f.num_images):
        os.makedirs(tmp_path / ("%04d" % i), exist_ok=True)
        with open(tmp_path / ("%04d" % i) / "st10_ep0.pkl", "wb") as fh:
            pickle.dump({k: golden["g9_frames_" + k][i] for k in keys}, fh)
    return str(tmp_path)


EVENTS = ("visibility_in_place", "visibility_item", "visibility_cpu_tensor", "optimizer_step", "trans_add", "weights", "load_checkpoint")


@pytest.mark.parametrize("event", EVENTS)
def test_each_invalidating_event_costs_exactly_one_more_evaluation(golden, md, tmp_path, event):
    w1 = [float(x) for x in golden["g6_w1"]]
    f = _golden_fitter(golden, md, 2, True)
    fresh = _golden_fitter(golden, md, 2, True)
    opts = [torch.optim.Adam(m.parameters(), lr=0.01, betas=(0.5, 0.999)) for m in (f, fresh)]
    if event == "optimizer_step":                         # both take the same step from the same gradients
        for m in (f, fresh):
            _epoch(m, w1)
    br = _windows(f)
    f(br[0], w1, 1)
    before = f.engine_evaluations
    assert before == 1                                     # (the epoch before an optimiser step and this call: one evaluation)
    f(br[0], w1, 1)
    f(br[1], w1, 1)
    assert f.engine_evaluations == before                  # served from the cache, in any order, as often as asked
    weights = w1

    def apply(m, opt):
        nonlocal weights
        if event == "visibility_in_place":
            m.target_visibility *= 0
        elif event == "visibility_item":
            m.target_visibility[:, cfg.TORSO_JOINTS] = 0
        elif event == "visibility_cpu_tensor":
            m.target_visibility = torch.from_numpy(golden["g6_visibility"]).clone() * torch.tensor([1.0, 0.0] * 12 + [1.0])
        elif event == "optimizer_step":
            opt.step()
        elif event == "trans_add":
            with torch.no_grad():
                m.trans.add_(0.01)
        elif event == "weights":
            weights = [w1[0] * 2.0] + w1[1:]
        elif event == "load_checkpoint":
            m.load_checkpoint(_checkpoint(tmp_path, m, golden), "st10_ep0")

    apply(f, opts[0])
    apply(fresh, opts[1])
    vals, _, grads = _epoch(f, weights, w_temp=100.0)
    assert f.engine_evaluations == before + 1
    f(br[1], weights, 1)
    assert f.engine_evaluations == before + 1
    had = fresh.engine_evaluations
    vals_f, _, grads_f = _epoch(fresh, weights, w_temp=100.0)
    assert fresh.engine_evaluations == had + 1
    assert vals == vals_f
    _same(grads, grads_f)


def test_requires_grad_flip_keeps_the_evaluation_and_frozen_parameters_get_no_gradient(golden, md):
    """the stage-0 pattern: frozen parameters end with .grad None; thawing them changes no value, so nothing is evaluated again,
    and they get their gradients from the evaluation already made"""
    w1 = [float(x) for x in golden["g6_w1"]]
    f = _golden_fitter(golden, md, 2, True)
    for k in ("joint_rotations", "betas", "log_beta_scales"):
        getattr(f, k).requires_grad = False
    _, _, grads = _epoch(f, w1, w_temp=100.0)
    assert grads["betas"] is None and grads["joint_rotations"] is None and grads["log_beta_scales"] is None
    assert grads["trans"] is not None and grads["global_rotation"] is not None
    for k in ("joint_rotations", "betas", "log_beta_scales"):
        getattr(f, k).requires_grad = True
    _, _, thawed = _epoch(f, w1, w_temp=100.0)
    assert f.engine_evaluations == 1
    twin = _golden_fitter(golden, md, 2, True)
    _, _, want = _epoch(twin, w1, w_temp=100.0)
    _same(thawed, want)
    assert np.array_equal(grads["trans"], want["trans"])


def test_an_older_loss_keeps_its_gradients(golden, md):
    w1 = [float(x) for x in golden["g6_w1"]]
    f, twin = _golden_fitter(golden, md, 2, True), _golden_fitter(golden, md, 2, True)
    br = _windows(f)
    loss_a = f(br[1], w1, 1)[0]
    with torch.no_grad():                                  # epoch B at other parameters
        f.trans.add_(0.05)
        f.betas.add_(0.1)
    loss_b = f(br[1], w1, 1)[0]
    assert f.engine_evaluations == 2 and float(loss_a) != float(loss_b)
    loss_a.backward()
    twin(br[1], w1, 1)[0].backward()
    _same(_grads(f), _grads(twin))


def test_unaligned_range_takes_the_window_alone_path(golden, md):
    w1 = [float(x) for x in golden["g6_w1"]]
    on, off = _golden_fitter(golden, md, 2, True), _golden_fitter(golden, md, 2, False)
    out = []
    for f in (on, off):
        loss, objs = f([1, 2], w1, 1)
        loss.backward()
        out.append((float(loss), {k: float(v) for k, v in objs.items()}, _grads(f)))
    assert on.engine_evaluations == 1 and on._epoch is None
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1]
    _same(out[0][2], out[1][2])


def test_ragged_sequence_matches_the_window_alone_path(golden, md):
    """N = 5, windows of 2: the last window holds one frame, normalised by its own size as the reference does"""
    w1 = [float(x) for x in golden["g6_w1"]]
    on, off = _golden_fitter(golden, md, 2, True, frames=5), _golden_fitter(golden, md, 2, False, frames=5)
    assert len(_windows(on)) == 3
    vals_on, _, g_on = _epoch(on, w1, w_temp=100.0, upstream=(1.0, 2.0, 0.5))
    vals_off, _, g_off = _epoch(off, w1, w_temp=100.0, upstream=(1.0, 2.0, 0.5))
    assert on.engine_evaluations == 1 and off.engine_evaluations == 3
    # two routes through the same kernels' float32 sums (frames summed per window here, per call there)
    assert np.allclose(vals_on, vals_off, rtol=2e-6)
    for k in PARAMS:
        assert rel(g_on[k], g_off[k]) < 2e-5, (k, rel(g_on[k], g_off[k]))
