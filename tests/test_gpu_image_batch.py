"""A batch of unrelated images, each with its own shape (smalfit_fit_args.subject_frames = 1, losses_per_frame,
smalify_amd.image_batch.ImageBatchFitter) against N separate one-frame problems of the float64 oracle (-m gpu).

Bounds are the project's existing ones: 1e-4 relative on every loss term (of itself, or of 1e-3 x the image's objective
when the term is a negligible part of it -- tests/test_gpu_eval_fixtures.py's rule), max(5e-4, 2 x the float32 oracle's own
deviation) relative L2 on every gradient tensor, 1e-4 relative L2 on parameters after 13 iterations
(tests/test_gpu_parity.py's bound for 8 / 5 iterations).  Tables are printed past pytest's capture.
"""
import ctypes as C
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TERM_TOL = 1e-4
GRAD_TOL = 5e-4
YARD = 2.0
LOOP_TOL = 1e-4
SENTINEL = -12345.0


def _rel(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _engine(max_frames, S, unity=True):
    from smalify_amd import engine as eng, synthetic
    from tests import image_batch_cases as ic
    md = synthetic.synthetic_model(seed=0, shape_family_id=1)
    e = eng.Engine(eng.DeviceModel(md), max_frames, S)
    e.set_pose_prior(*synthetic.synthetic_pose_prior())
    e.set_shape_prior(*(synthetic.synthetic_shape_prior() if unity else ic.shape_prior_20()))
    return e


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).cuda()


def _batch_eval(e, state, tg, stage, unity=True, rows=True, sil_u8=True):
    """one smalfit_fit_eval of the batch -> (losses (9,), rows (N,9) or None, grads)"""
    from tests import image_batch_cases as ic
    from oracle import smal_oracle as so
    weights, _, _ = ic.stage_weights(stage)
    N = state["trans"].shape[0]
    d = {k: _dev(v) for k, v in state.items()}
    lpf = torch.full((N, 9), SENTINEL, device="cuda") if rows else None
    tsil = torch.as_tensor(np.round(tg["tsil"] * 255.0).astype(np.uint8)).cuda() if sil_u8 else _dev(tg["tsil"])
    names = so.trainable_names(stage) if unity else tuple(k for k in so.trainable_names(stage) if k != "log_beta_scales")
    losses, grads = e.fit_eval(betas=d["betas"], log_beta_scales=d["log_beta_scales"] if unity else None,
                               global_rotation=d["global_rotation"], joint_rotations=d["joint_rotations"], trans=d["trans"],
                               target_joints=_dev(tg["tj"]), target_visibility=_dev(tg["vis"]), target_sil=tsil,
                               weights=weights, w_temp=0.0, window=1, temporal=False, want=names,
                               subject_frames=1, losses_per_frame=lpf)
    assert e.status() == 0
    return losses.cpu().numpy().astype(np.float64), None if lpf is None else lpf.cpu().numpy().astype(np.float64), \
        {k: g.cpu().numpy().astype(np.float64) for k, g in grads.items()}


def _check_against_oracle(tag, images, states, rows, grads, stage, lines, bad, names=None):
    from tests import image_batch_cases as ic
    for n, (im, st) in enumerate(zip(images, states)):
        ref, g64 = ic.oracle_eval(im["prob"], st, stage, names)
        _, g32 = ic.oracle_eval(ic.as_dtype(im, torch.float32), st, stage, names, dtype=torch.float32)
        scale = abs(ref.sum())
        for i, t in enumerate(ic.TERMS):
            if ref[i] == 0.0 and rows[n, i] == 0.0:
                continue
            err = abs(rows[n, i] - ref[i]) / max(abs(ref[i]), 1e-3 * scale)
            lines.append("%-14s image %2d %-11s hip %.8g  f64 %.8g  rel %.2e" % (tag, n, t, rows[n, i], ref[i], err))
            if err > TERM_TOL:
                bad.append(lines[-1])
        for k, g in g64.items():
            mine = grads[k][n] if k in ("betas", "log_beta_scales") else grads[k][n:n + 1]
            err, y = _rel(mine, g), _rel(g32[k], g)
            lines.append("%-14s image %2d d/d%-16s rel-L2 %.2e  (f32 oracle %.2e)" % (tag, n, k, err, y))
            if err > max(GRAD_TOL, YARD * y):
                bad.append(lines[-1])


@pytest.mark.parametrize("N,form", [(1, "plain"), (3, "plain"), (6, "split"), (20, "split"), (64, "wide")])
def test_one_evaluation_matches_the_oracle_per_image(N, form, capsys):
    """1. every row of losses_per_frame and every image's gradients against that image's own one-frame oracle problem, at the
    initial state and near each image's ground truth, stage-2 weights, 26-dim prior with per-image limb scales; one case per
    skinning launch of run_lbs_forward"""
    from tests import image_batch_cases as ic
    assert (N, form) in ic.EVAL_CASES and ic.skin_form(N) == form
    images = ic.make_images(N, ic.S_EVAL)
    e = _engine(N, ic.S_EVAL)
    tg = ic.targets(images)
    lines, bad = [], []
    for name, states in (("initial", [ic.initial_state() for _ in images]), ("near_gt", [im["near"] for im in images])):
        e.reset_raster_cache()
        losses, rows, grads = _batch_eval(e, ic.stack(states), tg, 2)
        _check_against_oracle("N=%d %s" % (N, name), images, states, rows, grads, 2, lines, bad)
        col = np.abs(rows.sum(0) - losses) / np.maximum(np.abs(losses), 1e-30)
        lines.append("N=%d %s column sums vs losses: max rel %.2e" % (N, name, col[losses != 0].max()))
        assert (col[losses != 0] <= max(1e-6, N * 2.0 ** -23)).all(), lines[-1]
    with capsys.disabled():
        print("\n[image batch: one evaluation, HIP vs float64 oracle per image, %s skinning]\n" % form + "\n".join(lines))
    assert not bad, "\n".join(bad)


def test_one_evaluation_with_the_20_dim_prior_and_no_limb_scales(capsys):
    """1b. the non-unity case: 20-dim prior over betas_n alone, logscale_mode 0"""
    from tests import image_batch_cases as ic
    N = 6
    images = ic.make_images(N, ic.S_EVAL, unity=False)
    e = _engine(N, ic.S_EVAL, unity=False)
    states = [im["near"] for im in images]
    losses, rows, grads = _batch_eval(e, ic.stack(states), ic.targets(images), 2, unity=False)
    lines, bad = [], []
    names = ("betas", "global_rotation", "trans", "joint_rotations")
    _check_against_oracle("N=6 20-dim", images, states, rows, grads, 2, lines, bad, names)
    with capsys.disabled():
        print("\n[image batch: 20-dim prior, no limb scales]\n" + "\n".join(lines))
    assert not bad, "\n".join(bad)


def test_rows_add_up_and_change_nothing_else(capsys):
    """2. both modes: the column sums of losses_per_frame are `losses`; for one subject (8-frame clip, windows of 3, temporal on)
    losses and gradients are bit-identical with and without the rows, and each row is the oracle's window_loss of that frame"""
    from oracle import smal_oracle as so
    from smalify_amd import config as cfg
    from tests import image_batch_cases as ic
    from tests import parity_cases as pc
    M, S, window, stage = 8, 64, 3, 2
    W = np.array(cfg.OPT_WEIGHTS).T
    weights, w_temp = W[stage][:6].copy(), float(W[stage][6])
    e, prob, cur, tg = pc.make_problem(M, S, window, seed=21)
    d = {k: _dev(v) for k, v in cur.items()}
    names = so.trainable_names(stage)

    def run(lpf):
        e.reset_raster_cache()
        losses, grads = e.fit_eval(betas=d["betas"], log_beta_scales=d["log_beta_scales"], global_rotation=d["global_rotation"],
                                   joint_rotations=d["joint_rotations"], trans=d["trans"], target_joints=_dev(tg["tj"]),
                                   target_visibility=_dev(tg["vis"]), target_sil=_dev(tg["tsil"]), weights=weights, w_temp=w_temp,
                                   window=window, want=names, losses_per_frame=lpf)
        assert e.status() == 0
        return losses.clone(), {k: g.clone() for k, g in grads.items()}
    plain_l, plain_g = run(None)
    lpf = torch.full((M, 9), SENTINEL, device="cuda")
    rows_l, rows_g = run(lpf)
    assert torch.equal(plain_l, rows_l), (plain_l, rows_l)
    for k in names:
        assert torch.equal(plain_g[k], rows_g[k]), k
    rows, losses = lpf.cpu().numpy().astype(np.float64), rows_l.cpu().numpy().astype(np.float64)
    lines = []
    for i, t in enumerate(ic.TERMS):
        if losses[i] != 0.0:
            err = abs(rows[:, i].sum() - losses[i]) / abs(losses[i])
            lines.append("clip   %-11s sum of rows %.9g  losses %.9g  rel %.2e" % (t, rows[:, i].sum(), losses[i], err))
            assert err <= 1e-6, lines[-1]
    # each row against the oracle's share of that frame
    p64 = {k: torch.from_numpy(v).double() for k, v in cur.items()}
    bad = []
    with torch.no_grad():
        for n in range(M):
            start = (n // window) * window
            _, terms = so.window_loss(prob, p64, [n], weights, full_size=min(window, M - start), owns_prior=(n % window == 0))
            ref = {k: float(v) for k, v in terms.items()}
            if n + 1 < M:
                pair = {k: v[n:n + 2] for k, v in p64.items() if k in ("global_rotation", "joint_rotations", "trans")}
                ref["temp_joint"], ref["temp_global"], ref["temp_trans"] = (float(x) for x in so.temporal_terms(pair, w_temp))
            scale = sum(abs(v) for v in ref.values())
            for i, t in enumerate(ic.TERMS):
                r = ref.get(t, 0.0)
                if r == 0.0 and rows[n, i] == 0.0:
                    continue
                err = abs(rows[n, i] - r) / max(abs(r), 1e-3 * scale)
                lines.append("clip   frame %d %-11s hip %.8g  f64 %.8g  rel %.2e" % (n, t, rows[n, i], r, err))
                if err > TERM_TOL:
                    bad.append(lines[-1])
    assert (rows[[1, 2, 4, 5, 7], 3] == 0.0).all() and (rows[[0, 3, 6], 3] > 0.0).all()     # the prior sits with each window's first frame
    assert (rows[M - 1, 5:8] == 0.0).all()                                                   # the last frame owns no pair
    # independent images
    images = ic.make_images(6, S)
    e2 = _engine(6, S)
    losses, rows, _ = _batch_eval(e2, ic.stack([im["near"] for im in images]), ic.targets(images), stage)
    for i, t in enumerate(ic.TERMS):
        if losses[i] != 0.0:
            err = abs(rows[:, i].sum() - losses[i]) / abs(losses[i])
            lines.append("images %-11s sum of rows %.9g  losses %.9g  rel %.2e" % (t, rows[:, i].sum(), losses[i], err))
            assert err <= 1e-6, lines[-1]
    assert (rows[:, 5:8] == 0.0).all()
    with capsys.disabled():
        print("\n[losses_per_frame: rows add up]\n" + "\n".join(lines))
    assert not bad, "\n".join(bad)


def _fitter(e, images, **kw):
    from smalify_amd import image_batch, synthetic
    from tests import image_batch_cases as ic
    sp = synthetic.synthetic_shape_prior()
    tg = ic.targets(images)
    return image_batch.ImageBatchFitter(e, tg["tj"], tg["vis"], tg["tsil"], True, sp[1][:20], sp[1][20:26], **kw)


def _set_state(f, state):
    for k, v in state.items():
        f.p[k].copy_(_dev(v).reshape(f.p[k].shape))


def test_image_zero_does_not_see_its_neighbours():
    """3. image 0's loss row, gradients and parameters after 10 iterations of stage 2 are bit-identical whichever five other
    images share its batch"""
    from tests import image_batch_cases as ic
    N, S = 6, ic.S_EVAL
    a = ic.make_images(N, S)
    b = [a[0]] + ic.make_images(N, S, seed=900)[1:]
    weights, _, lr = ic.stage_weights(2)
    got = []
    for images in (a, b):
        e = _engine(N, S)
        f = _fitter(e, images)
        _set_state(f, ic.stack([im["near"] for im in images]))
        f.begin_stage(2)
        rows = f.image_losses(weights, 2).clone()
        grads = {k: f.g[k][0].clone() for k in f.trainable(2)}
        f.run_iterations(weights, 0.0, lr, 2, 10)
        assert e.status() == 0
        got.append((rows, grads, {k: f.p[k][0].clone() for k in f.p}))
    assert not torch.equal(got[0][0][1:], got[1][0][1:])                     # the neighbours really differ
    assert torch.equal(got[0][0][0], got[1][0][0]), (got[0][0][0], got[1][0][0])
    for k in got[0][1]:
        assert torch.equal(got[0][1][k], got[1][1][k]), "gradient of %s of image 0 depends on its neighbours" % k
    for k in got[0][2]:
        assert torch.equal(got[0][2][k], got[1][2][k]), "%s of image 0 after 10 iterations depends on its neighbours" % k


SCHEDULE = ((0, 5), (1, 8))


def _opt_weights():
    from smalify_amd import config as cfg
    ow = np.array(cfg.OPT_WEIGHTS, np.float64)[:, :2].copy()
    ow[7] = [it for _, it in SCHEDULE]
    return ow


@pytest.fixture(scope="module")
def loop_case():
    """six images, their float64 oracle loops (5 iterations of stage 0, 8 of stage 1) and the batch fitted by run_schedule"""
    from tests import image_batch_cases as ic
    N, S = 6, ic.S_EVAL
    images = ic.make_images(N, S)
    ref = [ic.oracle_loop(im["prob"], ic.initial_state(), SCHEDULE) for im in images]
    e = _engine(N, S)
    f = _fitter(e, images)
    f.run_schedule(_opt_weights())
    assert e.status() == 0
    return images, ref, f


def test_the_loop_follows_each_images_oracle(loop_case, capsys):
    """4. 5 + 8 iterations through run_schedule: every image's tensors within 1e-4 relative L2 of its own float64 oracle loop,
    and K iterations in one smalfit_fit_run call equal K calls of one, bit for bit"""
    from tests import image_batch_cases as ic
    images, ref, f = loop_case
    lines, bad = [], []
    for n in range(len(images)):
        for k in ic.PARAMS:
            err = _rel(f.p[k][n].cpu().numpy(), ref[n][k])
            lines.append("image %d %-16s rel-L2 %.2e" % (n, k, err))
            if err > LOOP_TOL:
                bad.append(lines[-1])
    with capsys.disabled():
        print("\n[image batch: 5 + 8 iterations vs each image's float64 oracle loop]\n" + "\n".join(lines))
    assert not bad, "\n".join(bad)
    g = _fitter(_engine(len(images), ic.S_EVAL), images)
    for stage, iters in SCHEDULE:
        weights, _, lr = ic.stage_weights(stage)
        g.begin_stage(stage)
        for _ in range(iters):
            g.step(weights, 0.0, lr, stage)
    assert torch.equal(g.flat, f.flat) and torch.equal(g.exp_avg, f.exp_avg) and torch.equal(g.exp_avg_sq, f.exp_avg_sq)
    assert torch.equal(g.losses, f.losses)


def test_a_batch_equals_separate_one_image_fits(loop_case, capsys, tmp_path):
    """5. the same images fitted one at a time by FusedFitter(N = 1, window 1): each within the loop bound of the image's
    oracle, the batch's checkpoint of image n has the one-image fit's keys and shapes and loads through
    SMALFitter.load_checkpoint"""
    from smalify_amd import fitter as fit, synthetic
    from smalify_amd.smal_fitter.smal_fitter import SMALFitter
    from tests import image_batch_cases as ic
    images, ref, f = loop_case
    S = ic.S_EVAL
    sp = synthetic.synthetic_shape_prior()
    e1 = _engine(1, S)
    md = synthetic.synthetic_model(seed=0, shape_family_id=1)
    f.export_checkpoints([str(tmp_path / ("batch%d" % n) / "0000") for n in range(len(images))], 10, 0)
    lines, bad = [], []
    for n, im in enumerate(images):
        e1.reset_raster_cache()
        s = fit.FusedFitter(e1, im["tg"]["tj"], im["tg"]["vis"], im["tg"]["tsil"], 1, True, sp[1][:20], sp[1][20:26])
        s.run_schedule(_opt_weights())
        assert e1.status() == 0
        for k in ic.PARAMS:
            single = s.p[k].cpu().numpy().reshape(-1)
            err_s, err_b = _rel(single, ref[n][k]), _rel(f.p[k][n].cpu().numpy(), ref[n][k])
            lines.append("image %d %-16s one-image fit vs oracle %.2e   batch vs oracle %.2e   batch vs one-image fit %.2e"
                         % (n, k, err_s, err_b, _rel(f.p[k][n].cpu().numpy(), single)))
            if err_s > LOOP_TOL or err_b > LOOP_TOL:
                bad.append(lines[-1])
        s.export_checkpoints([str(tmp_path / ("single%d" % n) / "0000")], 10, 0)
        with open(tmp_path / ("single%d" % n) / "0000" / "st10_ep0.pkl", "rb") as fh:
            want = pickle.load(fh)
        with open(tmp_path / ("batch%d" % n) / "0000" / "st10_ep0.pkl", "rb") as fh:
            got = pickle.load(fh)
        assert sorted(got) == sorted(want)
        for k in want:
            assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        data = (torch.zeros(1, 3, S, S), torch.zeros(1, 1, S, S), torch.from_numpy(im["tg"]["tj"]), torch.from_numpy(im["tg"]["vis"]))
        m = SMALFitter("cuda", data, 1, 1, True, model_data=md, pose_prior_data=synthetic.synthetic_pose_prior(), shape_prior_data=sp)
        m.load_checkpoint(str(tmp_path / ("batch%d" % n)), "st10_ep0")
        assert np.array_equal(m.betas.detach().cpu().numpy(), f.p["betas"][n].cpu().numpy())
        assert np.array_equal(m.log_beta_scales.detach().cpu().numpy(), f.p["log_beta_scales"][n].cpu().numpy())
        assert np.array_equal(m.trans.detach().cpu().numpy()[0], f.p["trans"][n].cpu().numpy())
    with capsys.disabled():
        print("\n[image batch vs one-image fits, 5 + 8 iterations]\n" + "\n".join(lines))
    assert not bad, "\n".join(bad)


def _refusal_args(e, keep, **change):
    """a valid block of 4 independent images, then one field changed; every output pre-filled with a sentinel"""
    from tests import image_batch_cases as ic
    N = 4
    images = ic.make_images(N, ic.S_EVAL)
    st, tg = ic.stack([im["near"] for im in images]), ic.targets(images)
    weights, _, _ = ic.stage_weights(2)
    d = {k: _dev(v) for k, v in st.items()}
    if change.pop("shared_scales", False):
        d["log_beta_scales"] = d["log_beta_scales"][0].contiguous()
    outs = dict(losses=torch.full((9,), SENTINEL, device="cuda"), lpf=torch.full((N, 9), SENTINEL, device="cuda"),
                grads={k: torch.full_like(v, SENTINEL) for k, v in d.items()})
    halo = change.pop("halo", False)
    a, _, _, held = e.build_fit_args(betas=d["betas"], log_beta_scales=d["log_beta_scales"], global_rotation=d["global_rotation"],
                                     joint_rotations=d["joint_rotations"], trans=d["trans"], target_joints=_dev(tg["tj"]),
                                     target_visibility=_dev(tg["vis"]), target_sil=_dev(tg["tsil"]), weights=weights, w_temp=0.0,
                                     window=change.pop("window", 1), temporal=change.pop("temporal", False),
                                     halo_prev=torch.zeros(108, device="cuda") if halo else None,
                                     losses=outs["losses"], grads=outs["grads"], subject_frames=change.pop("subject_frames", 1),
                                     losses_per_frame=outs["lpf"])
    assert not change
    keep.append(held)
    return a, outs


@pytest.mark.parametrize("change,field", [(dict(subject_frames=2), "subject_frames"), (dict(window=8), "window"),
                                          (dict(temporal=True), "temporal"), (dict(shared_scales=True), "logscale_mode"),
                                          (dict(halo=True), "halo_prev")])
def test_what_couples_images_is_refused_before_the_first_launch(change, field):
    """6. each returns non-zero, smalfit_last_error() names the offending field, no output is touched"""
    from smalify_amd import engine as eng
    from tests import image_batch_cases as ic
    e = _engine(4, ic.S_EVAL)
    keep = []
    a, outs = _refusal_args(e, keep, **change)
    rc = e.lib.smalfit_fit_eval(e.handle, eng._stream(), C.byref(a))
    msg = e.lib.smalfit_last_error().decode()
    torch.cuda.synchronize()
    assert rc != 0 and field in msg, (rc, msg)
    if change.get("subject_frames") == 2:
        assert "not implemented" in msg
    for t in [outs["losses"], outs["lpf"]] + list(outs["grads"].values()):
        assert bool((t == SENTINEL).all()), msg


def test_independent_images_are_not_sharded():
    """6b. smalfit_shard_run refuses the mode, naming the field, before any launch"""
    from smalify_amd import _lib, engine as eng
    from tests import image_batch_cases as ic
    e = _engine(4, ic.S_EVAL)
    keep = []
    a, outs = _refusal_args(e, keep)
    n = sum(t.numel() for t in outs["grads"].values())
    flat = [torch.full((n,), SENTINEL, device="cuda") for _ in range(4)]
    al = eng.make_adam_args(flat[0], flat[1], flat[2], flat[3], [(0, 8)], 1e-3)
    ash = eng.make_adam_args(flat[0], flat[1], flat[2], flat[3], [], 1e-3)
    record, gathered = torch.full((20 + 216,), SENTINEL, device="cuda"), torch.full((1, 20 + 216), SENTINEL, device="cuda")
    sa = eng.ShardArgs()
    sa.world_size, sa.rank, sa.num_shared, sa.num_trainable_shared = 1, 0, 20, 20
    sa.shared_grad, sa.record, sa.gathered = eng._ptr(flat[1]), eng._ptr(record), eng._ptr(gathered)
    called = []
    fn = _lib.ALLGATHER_FN(lambda *args: called.append(1) or 0)
    sa.allgather, sa.allgather_ctx = C.cast(fn, C.c_void_p).value, None
    with pytest.raises(eng.SmalfitError) as err:
        eng.shard_run(e, a, al, ash, sa, 2)
    torch.cuda.synchronize()
    assert "subject_frames" in str(err.value) and not called
    for t in [outs["losses"], outs["lpf"], record, gathered] + flat + list(outs["grads"].values()):
        assert bool((t == SENTINEL).all())


def test_a_shared_shape_tensor_is_not_read_as_a_batch():
    """the library cannot know the extent of a device pointer: (20,) betas with subject_frames = 1 must not reach it"""
    from smalify_amd import engine as eng
    from tests import image_batch_cases as ic
    e = _engine(4, ic.S_EVAL)
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    common = dict(global_rotation=z(4, 3), joint_rotations=z(4, 34, 3), trans=z(4, 3), target_joints=z(4, 25, 2),
                  target_visibility=z(4, 25), target_sil=None, weights=(1, 0, 0, 0, 0, 0), w_temp=0.0, window=1, temporal=False)
    with pytest.raises(eng.SmalfitError, match="betas"):
        e.build_fit_args(betas=z(20), log_beta_scales=z(4, 6), subject_frames=1, **common)
    with pytest.raises(eng.SmalfitError, match="log_beta_scales"):
        e.build_fit_args(betas=z(4, 20), log_beta_scales=z(3, 6), subject_frames=1, **common)
    with pytest.raises(eng.SmalfitError, match="losses_per_frame"):
        e.build_fit_args(betas=z(4, 20), log_beta_scales=z(4, 6), subject_frames=1, losses_per_frame=z(3, 9), **common)
    a, _, _, _keep = e.build_fit_args(betas=z(4, 20), log_beta_scales=z(4, 6), subject_frames=1, **common)
    assert a.subject_frames == 1


def test_fit_run_checks_the_block_before_it_reads_its_tail():
    """smalfit_fit_run reads subject_frames, the block's last field but one: a block of another header is refused by its
    struct_size first, as smalfit_fit_eval does"""
    from smalify_amd import engine as eng
    from tests import image_batch_cases as ic
    e = _engine(4, ic.S_EVAL)
    keep = []
    a, outs = _refusal_args(e, keep)
    n = sum(t.numel() for t in outs["grads"].values())
    flat = [torch.full((n,), SENTINEL, device="cuda") for _ in range(4)]
    aa = eng.make_adam_args(flat[0], flat[1], flat[2], flat[3], [(0, 8)], 1e-3)
    a.struct_size -= 16                                    # ABI 5's block: ends before subject_frames
    for graph in (0, 1):
        e.lib.smalfit_engine_set_graph(e.handle, graph)
        rc = e.lib.smalfit_fit_run(e.handle, eng._stream(), C.byref(a), C.byref(aa), 3)
        assert rc != 0 and b"struct_size" in e.lib.smalfit_last_error(), e.lib.smalfit_last_error()
    e.lib.smalfit_engine_set_graph(e.handle, 0)
    torch.cuda.synchronize()
    for t in [outs["losses"], outs["lpf"]] + flat + list(outs["grads"].values()):
        assert bool((t == SENTINEL).all())


def test_prepare_schedule_builds_the_blocks_the_loop_uses():
    from tests import image_batch_cases as ic
    images = ic.make_images(2, ic.S_EVAL)
    f = _fitter(_engine(2, ic.S_EVAL), images)
    ow = _opt_weights()
    f.prepare_schedule(ow)
    keys = set(f._plan)
    assert len(keys) == len(SCHEDULE)
    f.run_schedule(ow)
    assert set(f._plan) == keys, "run_iterations looked up other blocks than prepare_schedule built"
    assert f.e.status() == 0


def test_fit_images_batches_a_dataset_and_exports_per_image(tmp_path):
    """optimize_to_joints.fit_images: 5 images in batches of 2 (the last batch smaller than the engine's max_frames), a tiny
    schedule; every image gets its own st10_ep0.pkl / .ply, the .pkl with the one-image fit's layout, and the images'
    results do not depend on the batching"""
    from smalify_amd import synthetic
    from smalify_amd.smal_fitter.optimize_to_joints import fit_images
    from tests import image_batch_cases as ic
    N, S = 5, ic.S_EVAL
    images = ic.make_images(N, S)
    tg = ic.targets(images)
    data = (np.zeros((N, 3, S, S), np.float32), tg["tsil"][:, None], tg["tj"], tg["vis"])
    names = ["dog%d.png" % n for n in range(N)]
    md = synthetic.synthetic_model(seed=0, shape_family_id=1)
    pri = (synthetic.synthetic_pose_prior(), synthetic.synthetic_shape_prior())
    out = fit_images(data, names, md, pri[0], pri[1], output_dir=str(tmp_path / "b2"), iters_scale=0.01, max_batch=2)
    whole = fit_images(data, names, md, pri[0], pri[1], output_dir=None, iters_scale=0.01, max_batch=8)
    assert len(out) == len(whole) == N
    for n in range(N):
        stem = tmp_path / "b2" / ("dog%d" % n) / "st10_ep0"
        with open(str(stem) + ".pkl", "rb") as fh:
            d = pickle.load(fh)
        assert sorted(d) == ["betas", "global_rotation", "joint_rotations", "log_betascale", "trans"]
        assert d["betas"].shape == (20,) and d["log_betascale"].shape == (6,) and d["joint_rotations"].shape == (34, 3)
        assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in d.values())
        assert os.path.getsize(str(stem) + ".ply") > md.num_verts * 12
        for k in d:
            assert np.array_equal(d[k], out[n][k])
            # batches of 2 and one batch of 5 take different skinning launches: equal as far as float32 allows
            assert _rel(out[n][k], whole[n][k]) < 1e-3, (n, k)
    assert not np.array_equal(out[0]["trans"], out[1]["trans"])
