"""The scan-sequence block on the GPU (include/smalfit.h, "scan sequences"): smalfit_scan_sequence_couple against the host shim,
smalfit_scan_sequence_step against the same iterations composed from the component calls, the block off against the plain step,
one shape per clip after a few steps, no state left behind, refusals, Stage end to end.  Synthetic model, S = 64 points per mesh.

Bit equality everywhere except the losses of couple against the float64 restatement, which take the float32 bar of
tests/sequence_cases.py (three times the deviation of a plain float32 torch restatement; tests/golden/hip_fit3d_sequence_measured.json)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from smalify_amd import _lib, engine as eng, synthetic  # noqa: E402
from smalify_amd.fitter_3d import trainer  # noqa: E402
from tests import host_sequence as hs  # noqa: E402
from tests import mesh3d_cases as mc  # noqa: E402
from tests import sequence_cases as sc  # noqa: E402

S = 64
MAX_FRAMES_CLIPS = (5, 1, 7, 3)                     # N = 16: the capacity the runtime gives a fitter's engine
SHAPES = sc.CLIPS + (MAX_FRAMES_CLIPS,)
TEMPORAL = dict(w_temp_joint=0.7, w_temp_global=1.3, w_temp_trans=2.1)
PARAMS = ("betas", "log_beta_scales", "global_rot", "joint_rot", "trans", "deform_verts")
ALL_BLOCKS = dict(loss_weights=dict(w_point_surface=0.5, w_vert_surface=0.5), surface_gates=dict(max_dist_point=0.5, min_cos_vert=0.0),
                  chamfer_gates=dict(max_dist_vert=0.5), robust=dict(sigma_chamfer_point=0.2, sigma_surface_vert=0.2))
_CACHE = {}


def dev(x):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).cuda()


@pytest.fixture(autouse=True)
def _few_points(monkeypatch):
    monkeypatch.setattr(trainer, "N_SAMPLE_POINTS", S)


def _problem(clips, seed=3):
    """a fitter of sum(clips) meshes away from its start -- poses that differ from mesh to mesh, one shape per clip -- and its
    targets (posed synthetic SMAL meshes, computed once per N)"""
    N = int(sum(clips))
    if "md" not in _CACHE:
        _CACHE["md"], _CACHE["smal"] = synthetic.synthetic_model(seed=0, shape_family_id=-1), mc.synthetic_smal_data()
    md = _CACHE["md"]
    if N not in _CACHE:
        _CACHE[N] = mc.target_meshes_from_smal(md, N, seed=seed + 1)
    tv, tf = _CACHE[N]
    fit = trainer.SMAL3DFitter(batch_size=N, shape_family=-1, model_data=md, smal_data=_CACHE["smal"])
    from smalify_amd.fitter_3d import TargetMeshes
    rng = np.random.default_rng(seed)
    rows = 0.3 * rng.standard_normal((len(clips), int(fit.betas.shape[1])))
    with torch.no_grad():
        fit.global_rot.copy_(dev(0.1 * rng.standard_normal((N, 3))))
        fit.joint_rot.copy_(dev(0.05 * rng.standard_normal((N, 34, 3))))
        fit.trans.copy_(dev(0.05 * rng.standard_normal((N, 3))))
        fit.betas.add_(dev(np.repeat(rows, clips, axis=0)))
    return fit, TargetMeshes(tv, [tf] * N)


def _stage(fit, targets, scheme, clips, iters=3, **kw):
    lr = 2e-4 if scheme == "deform" else 0.02
    kw.setdefault("temporal", TEMPORAL)
    return trainer.Stage(iters, scheme, fit, targets, lr=lr, custom_lrs=dict(mc.DEFAULT_CUSTOM_LRS), seed=11, clip_lengths=clips, **kw)


def _snapshot(fit, stage):
    out = {k: getattr(fit, k).detach().clone() for k in PARAMS}
    for name, st in stage._adam.items():
        out["m_" + name], out["v_" + name] = st["m"].clone(), st["v"].clone()
    return out


def _run(clips, scheme, fused, iters=3, **kw):
    """`iters` iterations from a fresh fitter -> (per iteration: total, the five terms, the four temporal figures [, the surface
    term's three], parameters and moments after the last)"""
    fit, targets = _problem(clips)
    stage = _stage(fit, targets, scheme, clips, iters, **kw)
    rec = []
    for it in range(iters):
        total = (stage.step(it) if fused else stage.step_unfused(it)).clone()
        row = dict(total=total, terms=stage.last_terms.clone())
        if stage.last_temporal_losses is not None:
            row["temporal"] = stage.last_temporal_losses.clone()
        if stage.last_surface_terms is not None:
            row["surface"] = stage.last_surface_terms.clone()
        rec.append(row)
    torch.cuda.synchronize()
    return rec, _snapshot(fit, stage), stage


def _assert_same_bits(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        same = torch.equal(a[k], b[k])
        if not same:
            print(what, k, "max |a - b| =", float((a[k] - b[k]).abs().max()), "max |b| =", float(b[k].abs().max()))
        assert same, (what, k)


def _assert_same_run(ra, rb, what):
    (rec_a, snap_a, _), (rec_b, snap_b, _) = ra, rb
    assert len(rec_a) == len(rec_b)
    for it, (x, y) in enumerate(zip(rec_a, rec_b)):
        _assert_same_bits(x, y, "%s iteration %d" % (what, it))
    _assert_same_bits(snap_a, snap_b, what + " final state")


# ---- 1. couple against the shim -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clips", SHAPES, ids=sc.clip_id)
def test_couple_matches_the_shim(clips):
    st, bar = sc.state(clips), sc.bars()
    want = hs.couple(clips, st, True, sc.WEIGHTS)
    ref = sc.reference64(clips, st, True, sc.WEIGHTS)
    seq = eng.ScanSequence(clips)
    runs = []
    for _ in range(2):
        g = {k: dev(st[k]) for k in ("g_betas", "g_theta", "g_trans")}
        losses = seq.couple(dev(st["global_rot"]), dev(st["joint_rot"]), dev(st["trans"]), share_shape=True,
                            temporal=dict(zip(hs.WEIGHT_KEYS, sc.WEIGHTS)), losses=torch.full((4,), float("nan"), device="cuda"), **g)
        torch.cuda.synchronize()
        runs.append({k: v.cpu().numpy() for k, v in dict(g, losses=losses).items()})
    for k in ("g_betas", "g_theta", "g_trans"):
        assert np.array_equal(sc.bits(runs[0][k]), sc.bits(want[k])), k                      # gradients: bit for bit
        assert sc.deviation(runs[0][k], ref[k]) <= bar["grad"], k
    for t in range(4):
        d = sc.deviation(runs[0]["losses"][t], ref["losses"][t])
        print(clips, "loss", t, "gpu vs float64", d, "bits equal to the shim:", sc.bits(runs[0]["losses"][t]) == sc.bits(want["losses"][t]))
        assert d <= bar["loss"], (t, d)
    for k in runs[0]:
        assert np.array_equal(sc.bits(runs[0][k]), sc.bits(runs[1][k])), k                   # the same bits every run


def test_couple_takes_any_subset_of_the_gradients_and_the_dyadic_case():
    clips, st = sc.DYADIC_CLIPS, sc.dyadic_state()
    want = sc.dyadic_closed_form()
    seq = eng.ScanSequence(clips)
    w = dict(zip(hs.WEIGHT_KEYS, sc.DYADIC_WEIGHTS))
    x = [dev(st[k]) for k in ("global_rot", "joint_rot", "trans")]
    g = {k: dev(st[k]) for k in ("g_betas", "g_theta", "g_trans")}
    losses = seq.couple(*x, temporal=w, **g)
    for k in g:
        assert np.array_equal(sc.bits(g[k].cpu().numpy()), sc.bits(want[k])), k
    assert np.array_equal(sc.bits(losses.cpu().numpy()), sc.bits(want["losses"]))              # exact sums: one result in any order
    for keep in ("g_betas", "g_theta", "g_trans"):
        one = {keep: dev(st[keep])}
        again = seq.couple(*x, temporal=w, **one)
        assert np.array_equal(sc.bits(one[keep].cpu().numpy()), sc.bits(want[keep])), keep
        assert torch.equal(again, losses)                                                      # the loss is reported either way
    only = dev(st["g_betas"])
    assert not seq.couple(g_betas=only).any() and np.array_equal(sc.bits(only.cpu().numpy()), sc.bits(want["g_betas"]))
    off = dev(st["g_betas"])
    assert not seq.couple(g_betas=off, share_shape=False).any() and np.array_equal(sc.bits(off.cpu().numpy()), sc.bits(st["g_betas"]))


# ---- 2. the fused step against the component calls ------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme,clips,blocks", [("default", c, {}) for c in SHAPES] +
                         [(s, (1, 3, 1), {}) for s in ("shape", "pose", "init", "deform")] + [("default", (2, 1), ALL_BLOCKS)],
                         ids=lambda v: sc.clip_id(v) if isinstance(v, tuple) else ("blocks" if v else "plain") if isinstance(v, dict) else v)
def test_fused_step_equals_the_component_calls(scheme, clips, blocks):
    fused = _run(clips, scheme, True, **blocks)
    parts = _run(clips, scheme, False, **blocks)
    _assert_same_run(fused, parts, "%s %s" % (scheme, clips))
    rec, snap, stage = fused
    if sum(clips) > len(clips):
        assert float(rec[-1]["temporal"][3]) > 0                                             # the terms were on and saw a difference
        assert float(rec[0]["total"]) == float(np.float32(float(rec[0]["terms"][4]) + (float(rec[0]["surface"][2]) if blocks else 0.0))
                                                + np.float32(float(rec[0]["temporal"][3])))
    else:
        assert not rec[-1]["temporal"].any()


# ---- 3. nothing coupled: the step of before ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocks", [{}, ALL_BLOCKS], ids=["plain", "blocks"])
def test_clips_of_length_one_are_the_step_without_the_block(blocks):
    clips = (1, 1, 1)
    with_block = _run(clips, "default", True, **blocks)
    fit, targets = _problem(clips)
    stage = trainer.Stage(3, "default", fit, targets, lr=0.02, custom_lrs=dict(mc.DEFAULT_CUSTOM_LRS), seed=11, **blocks)
    rec = []
    for it in range(3):
        total = stage.step(it).clone()
        row = dict(total=total, terms=stage.last_terms.clone(), temporal=torch.zeros(4, device="cuda"))
        if stage.last_surface_terms is not None:
            row["surface"] = stage.last_surface_terms.clone()
        rec.append(row)
    torch.cuda.synchronize()
    _assert_same_run(with_block, (rec, _snapshot(fit, stage), stage), "clips of one")


# ---- 4. one shape per clip ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clips", [(1, 3, 1), (2, 1), MAX_FRAMES_CLIPS], ids=sc.clip_id)
def test_shapes_stay_tied_within_a_clip_and_differ_between_clips(clips):
    _, snap, _ = _run(clips, "default", True, iters=5)
    start = 0
    firsts = []
    for length in clips:
        for k in ("betas", "m_betas", "v_betas"):
            rows = snap[k][start:start + length]
            assert torch.equal(rows, rows[:1].expand_as(rows)), (k, start)
        firsts.append(start)
        start += length
    for k in ("betas", "m_betas", "v_betas"):
        for a in firsts:
            for b in firsts:
                assert a == b or not torch.equal(snap[k][a], snap[k][b]), (k, a, b)


# ---- 5. no state left behind ----------------------------------------------------------------------------------------------------------
def test_the_block_leaves_no_state_in_the_engine_or_the_objective():
    clips = (2, 1)
    fit, targets = _problem(clips)
    plain = trainer.Stage(2, "default", fit, targets, lr=0.02, seed=11)
    coupled = _stage(fit, targets, "default", clips, 2)
    start = _snapshot(fit, plain)

    def restore(stage):
        with torch.no_grad():
            for k in PARAMS:
                getattr(fit, k).copy_(start[k])
        for st in stage._adam.values():
            st["m"].zero_()
            st["v"].zero_()
        stage._t = 0

    first = (plain.step(0).clone(), _snapshot(fit, plain))
    restore(coupled)
    coupled.step(0)
    assert not torch.equal(coupled._adam["betas"]["m"], first[1]["m_betas"])                # the block did couple something
    restore(plain)
    again = (plain.step(0).clone(), _snapshot(fit, plain))
    torch.cuda.synchronize()
    assert torch.equal(first[0], again[0])
    _assert_same_bits(first[1], again[1], "plain step after a coupled one")


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_entry_point_and_change_nothing():
    clips = (2, 1)
    lib = _lib.load()
    couple = _lib.resolve(lib, "smalfit_scan_sequence_couple")
    create = _lib.resolve(lib, "smalfit_scan_sequence_create")
    h = C.c_void_p()
    assert create(3, 2, (C.c_int * 2)(2, 2), C.byref(h)) == 1 and not h.value
    assert b"smalfit_scan_sequence_create: clip_lengths do not sum to num_meshes" in lib.smalfit_last_error()
    assert create(3, 2, (C.c_int * 2)(3, 0), C.byref(h)) == 1 and b"every clip length must be positive" in lib.smalfit_last_error()
    seq = eng.ScanSequence(clips)
    st = sc.state(clips)
    x = [dev(st[k]) for k in ("global_rot", "joint_rot", "trans")]
    g = [dev(st[k]) for k in ("g_betas", "g_theta", "g_trans")]
    before = [t.clone() for t in g]
    losses = torch.full((4,), 7.0, device="cuda")
    total = torch.zeros(1, device="cuda")

    def refused(q, text, xs=x):
        rc = couple(seq.handle, eng._stream(), C.byref(q), sc.NUM_BETAS, *[eng._ptr(t) for t in xs], *[eng._ptr(t) for t in g])
        msg = lib.smalfit_last_error()
        torch.cuda.synchronize()
        assert rc == 1 and msg.startswith(b"smalfit_scan_sequence_couple: ") and text in msg, msg
        assert all(torch.equal(a, b) for a, b in zip(g, before)) and bool((losses == 7.0).all())

    refused(seq.block(True, dict(w_temp_joint=float("nan")), losses)[0], b"w_temp_joint is not finite")
    refused(seq.block(True, dict(w_temp_trans=float("inf")), losses)[0], b"w_temp_trans is not finite")
    q = seq.block(True, TEMPORAL, losses)[0]
    q.losses = None
    refused(q, b"losses is NULL")
    refused(seq.block(True, TEMPORAL, losses, total)[0], b"step_total given outside a step")
    refused(seq.block(True, TEMPORAL, losses)[0], b"w_temp_global > 0 but global_rot is missing", xs=[None, x[1], x[2]])
    assert couple(None, eng._stream(), C.byref(q), sc.NUM_BETAS, *[None] * 6) == 1 and b"null argument" in lib.smalfit_last_error()

    # the step: a handle built for another N, a bad block; parameters, moments and every loss buffer keep their bits
    fit, targets = _problem(clips)
    stage = _stage(fit, targets, "default", clips)
    stage.step(0)
    torch.cuda.synchronize()
    a, q = stage._step_args(), stage._sequence_block()
    e = fit._engine()
    step = _lib.resolve(lib, "smalfit_scan_sequence_step")
    held = _snapshot(fit, stage)
    held.update(losses=stage.last_terms.clone(), temporal=stage.last_temporal_losses.clone(), total=stage._seq_total.clone())
    other = eng.ScanSequence((2, 2))

    def step_refused(handle, block, text):
        rc = step(handle, e.handle, stage._objective.handle, targets._dev.handle, eng._stream(), C.byref(a), None, None, None, None,
                  C.byref(block) if block is not None else None)
        msg = lib.smalfit_last_error()
        torch.cuda.synchronize()
        assert rc == 1 and msg.startswith(b"smalfit_scan_sequence_step: ") and text in msg, msg
        now = _snapshot(fit, stage)
        now.update(losses=stage.last_terms, temporal=stage.last_temporal_losses, total=stage._seq_total)
        _assert_same_bits(now, held, "refused step")

    a.adam_t = 2
    step_refused(other.handle, q, b"the sequence handle was built for another num_meshes")
    bad = seq.block(True, dict(w_temp_global=float("-inf")), stage._seq_step_losses, stage._seq_total)[0]
    step_refused(stage._sequence.handle, bad, b"w_temp_global is not finite")
    step_refused(stage._sequence.handle, None, b"null argument")
    a.adam_t = 0
    step_refused(stage._sequence.handle, q, b"adam_t")                                           # the step's own refusals, under this name


# ---- 7. Stage end to end ----------------------------------------------------------------------------------------------------------------
def test_stage_refuses_untied_rows_and_writes_clip_lengths(tmp_path):
    clips = (2, 1)
    fit, targets = _problem(clips)
    with torch.no_grad():
        fit.betas[1, 0] += 0.5
    with pytest.raises(ValueError, match="tie_shapes"):
        _stage(fit, targets, "default", clips)
    _stage(fit, targets, "pose", clips)                                       # betas is not trained: nothing to tie
    _stage(fit, targets, "default", clips, share_shape=False)
    trainer.tie_shapes(fit, clips)
    stage = _stage(fit, targets, "default", clips, 2, out_dir=str(tmp_path), name="seq")
    assert stage.last_temporal_losses is None
    total = stage.step(0)
    assert float(total) == float(stage._seq_total[0]) and float(stage.last_temporal_losses[3]) > 0
    stage.save_npz()
    z = np.load(tmp_path / "seq.npz", allow_pickle=True)
    assert z["clip_lengths"].tolist() == [2, 1] and z["betas"].shape == (3, 20)
    assert np.array_equal(z["betas"][0], z["betas"][1]) and not np.array_equal(z["betas"][0], z["betas"][2])
    plain = trainer.Stage(1, "default", fit, targets, out_dir=str(tmp_path), name="plain")
    plain.save_npz()
    assert "clip_lengths" not in np.load(tmp_path / "plain.npz", allow_pickle=True).files
    with pytest.raises(ValueError, match="sum 3"):
        _stage(fit, targets, "default", (2, 2))
