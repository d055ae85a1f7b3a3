"""The temporal terms on posed vertices on the GPU (include/smalfit.h, "scan sequences", the vertex terms):
smalfit_scan_sequence_vertex_term against the host shim, smalfit_scan_sequence_vertex_step against the same iterations composed
from the component calls, the block off against the sequence step, clips of length 1 against the plain step, no state left
behind, refusals, Stage end to end.  Synthetic model, S = 64 points per mesh.

Bit equality everywhere except the losses and d trans of the stand-alone call against the float64 restatement, which take the
float32 bar of tests/sequence_vertex_cases.py (three times the deviation of a plain float32 torch restatement;
tests/golden/hip_fit3d_sequence_vertex_measured.json)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from smalify_amd import _lib, engine as eng, synthetic  # noqa: E402
from smalify_amd.fitter_3d import trainer  # noqa: E402
from tests import host_sequence_vertex as hv  # noqa: E402
from tests import mesh3d_cases as mc  # noqa: E402
from tests import sequence_vertex_cases as vc  # noqa: E402

S = 64
GPU_VERTS = (1, 64, 255, 256, 257, 3889)
GPU_CLIPS = vc.CLIPS + ((5, 1, 7, 3), (16,))        # N = 16: the capacity the runtime gives a fitter's engine
TEMPORAL = dict(w_temp_joint=0.7, w_temp_global=1.3, w_temp_trans=2.1)
# (the step's vertices are about a unit across and move by a few hundredths between meshes: weights that make the terms count)
TEMPORAL_VERTS = dict(w_temp_vert_vel=30.0, w_temp_vert_acc=50.0)
PARAMS = ("betas", "log_beta_scales", "global_rot", "joint_rot", "trans", "deform_verts")
ALL_BLOCKS = dict(loss_weights=dict(w_point_surface=0.5, w_vert_surface=0.5), surface_gates=dict(max_dist_point=0.5, min_cos_vert=0.0),
                  chamfer_gates=dict(max_dist_vert=0.5), robust=dict(sigma_chamfer_point=0.2, sigma_surface_vert=0.2))
_CACHE = {}
_GPU_RECORD = {}


def dev(x):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).cuda()


def host(out):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


def weights_dict(w):
    return dict(zip(hv.WEIGHT_KEYS, w))


@pytest.fixture(autouse=True)
def _few_points(monkeypatch):
    monkeypatch.setattr(trainer, "N_SAMPLE_POINTS", S)


# ---- 1. the stand-alone call against the shim and float64 ------------------------------------------------------------------------
@pytest.mark.parametrize("V", GPU_VERTS)
def test_vertex_term_matches_the_shim(V):
    bar = vc.bars()
    worst, loss_bits, dtrans_bits = dict(loss=0.0, dtrans=0.0, grad=0.0), True, True
    for clips in GPU_CLIPS:
        seq = eng.ScanSequence(clips)
        x = vc.verts(clips, V)
        xd = dev(x)
        for w in vc.WEIGHT_SETS:
            want, ref = hv.term(clips, x, w), vc.reference64(clips, x, w)
            runs = []
            for _ in range(2):
                fill = dict(losses=torch.full((3,), float("nan"), device="cuda"), dverts=torch.full((len(x), V, 3), float("nan"), device="cuda"),
                            dtrans=torch.full((len(x), 3), float("nan"), device="cuda"))
                runs.append(host(seq.vertex_term(xd, weights_dict(w), out=fill)))
            got = runs[0]
            assert np.array_equal(vc.bits(got["dverts"]), vc.bits(want["dverts"])), (clips, w)        # no reduction: bit for bit
            d = vc.worst([(got, ref)])
            same_l = np.array_equal(vc.bits(got["losses"]), vc.bits(want["losses"]))
            same_t = np.array_equal(vc.bits(got["dtrans"]), vc.bits(want["dtrans"]))
            print(V, clips, w, "gpu vs float64", d, "bits equal to the shim: losses", same_l, "dtrans", same_t)
            loss_bits, dtrans_bits = loss_bits and same_l, dtrans_bits and same_t
            for k in worst:
                worst[k] = max(worst[k], d[k])
            assert d["loss"] <= bar["loss"] and d["dtrans"] <= bar["dtrans"] and d["grad"] <= bar["grad"], (clips, w, d)
            for k in got:
                assert np.array_equal(vc.bits(got[k]), vc.bits(runs[1][k])), k                        # the same bits every run
    _GPU_RECORD["V=%d" % V] = dict(worst, losses_bit_equal_to_shim=loss_bits, dtrans_bit_equal_to_shim=dtrans_bits,
                                   gradients_bit_equal_to_shim=True)
    vc.record({"gpu_vs_float64": dict(device=torch.cuda.get_device_name(0), **_GPU_RECORD)})


@pytest.mark.parametrize("V", vc.DYADIC_VERTS)
def test_dyadic_case_and_optional_outputs(V):
    clips, x, w = vc.DYADIC_CLIPS, vc.dyadic_verts(V), weights_dict(vc.dyadic_weights(V))
    want = vc.dyadic_closed_form(V)
    seq = eng.ScanSequence(clips)
    full = host(seq.vertex_term(dev(x), w))
    for k in ("dverts", "dtrans", "losses"):
        assert np.array_equal(vc.bits(full[k]), vc.bits(want[k])), k                                  # exact sums: one result in any order
    for dv, dt in ((False, True), (True, False), (False, False)):
        part = host(seq.vertex_term(dev(x), w, want_dverts=dv, want_dtrans=dt))
        assert np.array_equal(vc.bits(part["losses"]), vc.bits(want["losses"]))                       # the loss is reported either way
        assert (part["dverts"] is None) == (not dv) and (part["dtrans"] is None) == (not dt)
        assert not dv or np.array_equal(vc.bits(part["dverts"]), vc.bits(want["dverts"]))
        assert not dt or np.array_equal(vc.bits(part["dtrans"]), vc.bits(want["dtrans"]))
    # off: nothing is launched, the losses and the gradients given read 0
    off = seq.vertex_term(dev(x), None, out=dict(losses=torch.full((3,), 7.0, device="cuda"), dverts=torch.full(x.shape, 7.0, device="cuda"),
                                                 dtrans=torch.full((len(x), 3), 7.0, device="cuda")))
    assert not off["losses"].any() and not off["dverts"].any() and not off["dtrans"].any()
    short = eng.ScanSequence((2,) * (len(x) // 2) + (1,) * (len(x) % 2))                               # no clip holds a triple
    assert not short.vertex_term(dev(x), dict(w_temp_vert_acc=1.0))["losses"].any()


def test_chained_calls_leave_no_state_and_the_partials_regrow():
    clips = (1, 3, 1)
    seq = eng.ScanSequence(clips)
    w = weights_dict(vc.WEIGHTS)
    first = {V: host(seq.vertex_term(dev(vc.verts(clips, V)), w)) for V in (257, 64, 3889, 255)}       # grows at 3889, reused at 255
    for V in (255, 3889, 64, 257):
        again = host(seq.vertex_term(dev(vc.verts(clips, V)), w))
        fresh = host(eng.ScanSequence(clips).vertex_term(dev(vc.verts(clips, V)), w))
        for k in again:
            assert np.array_equal(vc.bits(again[k]), vc.bits(first[V][k])) and np.array_equal(vc.bits(again[k]), vc.bits(fresh[k])), (V, k)
    # ... and the parameter terms of the same handle are what they were
    from tests import host_sequence as hs, sequence_cases as sc
    st = sc.state(clips)
    g = {k: dev(st[k]) for k in ("g_betas", "g_theta", "g_trans")}
    seq.couple(dev(st["global_rot"]), dev(st["joint_rot"]), dev(st["trans"]), temporal=dict(zip(hs.WEIGHT_KEYS, sc.WEIGHTS)), **g)
    want = hs.couple(clips, st, True, sc.WEIGHTS)
    assert all(np.array_equal(sc.bits(g[k].cpu().numpy()), sc.bits(want[k])) for k in g)


# ---- 2. the fused step against the component calls ------------------------------------------------------------------------------
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
    kw.setdefault("temporal_verts", TEMPORAL_VERTS)
    return trainer.Stage(iters, scheme, fit, targets, lr=lr, custom_lrs=dict(mc.DEFAULT_CUSTOM_LRS), seed=11, clip_lengths=clips, **kw)


def _snapshot(fit, stage):
    out = {k: getattr(fit, k).detach().clone() for k in PARAMS}
    for name, st in stage._adam.items():
        out["m_" + name], out["v_" + name] = st["m"].clone(), st["v"].clone()
    return out


def _record(stage, total, vertex=True):
    row = dict(total=total.clone(), terms=stage.last_terms.clone())
    if stage.last_temporal_losses is not None:
        row["temporal"] = stage.last_temporal_losses.clone()
    if vertex:
        got = stage.last_temporal_vertex_losses
        row["vertex"] = got.clone() if got is not None else torch.zeros(3, device="cuda")
    if stage.last_surface_terms is not None:
        row["surface"] = stage.last_surface_terms.clone()
    return row


def _run(clips, scheme, fused, iters=3, stage=None, fit=None, **kw):
    """`iters` iterations from a fresh fitter -> (per iteration: total, the five terms, the four temporal figures, the three vertex
    figures [, the surface term's three], parameters and moments after the last)"""
    if stage is None:
        fit, targets = _problem(clips)
        stage = _stage(fit, targets, scheme, clips, iters, **kw)
    rec = [_record(stage, stage.step(it) if fused else stage.step_unfused(it)) for it in range(iters)]
    torch.cuda.synchronize()
    return rec, _snapshot(fit, stage), stage


def _assert_same_bits(a, b, what):
    assert set(a) == set(b), (what, sorted(a), sorted(b))
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


@pytest.mark.parametrize("scheme,clips,kw", [("default", c, {}) for c in ((5,), (2, 1), (5, 1, 7, 3))] +
                         [(s, (1, 3, 1), {}) for s in ("shape", "pose", "init", "deform")] + [("default", (3, 1), ALL_BLOCKS)] +
                         [("default", (4,), dict(temporal_verts=dict(w_temp_vert_vel=30.0))),
                          ("default", (4,), dict(temporal_verts=dict(w_temp_vert_acc=50.0))),
                          ("default", (3, 2), dict(temporal=None, share_shape=False))],
                         ids=lambda v: vc.clip_id(v) if isinstance(v, tuple) else ("-".join(sorted(v)) or "plain") if isinstance(v, dict) else v)
def test_fused_step_equals_the_component_calls(scheme, clips, kw):
    fused = _run(clips, scheme, True, **kw)
    parts = _run(clips, scheme, False, **kw)
    _assert_same_run(fused, parts, "%s %s" % (scheme, clips))
    rec, snap, stage = fused
    f = lambda t: np.float32(float(t))
    surface = f(rec[0]["surface"][2]) if "surface" in rec[0] else None
    base = f(rec[0]["terms"][4]) if surface is None else np.float32(f(rec[0]["terms"][4]) + surface)
    assert float(rec[0]["total"]) == float(np.float32(np.float32(base + f(rec[0]["temporal"][3])) + f(rec[0]["vertex"][2])))
    on = eng.temporal_vertex_weights(kw.get("temporal_verts", TEMPORAL_VERTS))
    assert (float(rec[-1]["vertex"][0]) > 0) == (on["w_temp_vert_vel"] > 0) and (float(rec[-1]["vertex"][1]) > 0) == (on["w_temp_vert_acc"] > 0 and max(clips) >= 3)
    # the terms pull: the same run without them ends elsewhere
    without = _run(clips, scheme, True, **dict(kw, temporal_verts=None))
    trained = [k for k in PARAMS if k in stage._adam]
    assert any(not torch.equal(snap[k], without[1][k]) for k in trained)


# ---- 3. the block off: the sequence step; clips of length 1: the plain step -----------------------------------------------------
@pytest.mark.parametrize("blocks", [{}, ALL_BLOCKS], ids=["plain", "blocks"])
def test_both_weights_zero_is_the_sequence_step(blocks, monkeypatch):
    clips = (3, 1)
    sequence = _run(clips, "default", True, temporal_verts=None, **blocks)                 # smalfit_scan_sequence_step
    fit, targets = _problem(clips)
    stage = _stage(fit, targets, "default", clips, temporal_verts=dict(w_temp_vert_vel=0.0, w_temp_vert_acc=-1.0), **blocks)
    monkeypatch.setattr(stage, "_vertex_terms_on", lambda: True)                           # the vertex entry point, both weights <= 0
    off = _run(clips, "default", True, stage=stage, fit=fit)
    assert stage._vert_args is not None and not stage.last_temporal_vertex_losses.any()
    _assert_same_run(off, sequence, "vertex block off")
    assert torch.equal(stage._vert_total, stage._seq_total)                               # its step_total is the sequence step's


@pytest.mark.parametrize("blocks", [{}, ALL_BLOCKS], ids=["plain", "blocks"])
def test_clips_of_length_one_are_the_plain_step(blocks):
    clips = (1, 1, 1)
    with_block = _run(clips, "default", True, **blocks)
    assert with_block[2]._vert_args is not None
    fit, targets = _problem(clips)
    stage = trainer.Stage(3, "default", fit, targets, lr=0.02, custom_lrs=dict(mc.DEFAULT_CUSTOM_LRS), seed=11, **blocks)
    rec = []
    for it in range(3):
        row = _record(stage, stage.step(it))
        row["temporal"] = torch.zeros(4, device="cuda")
        rec.append(row)
    torch.cuda.synchronize()
    _assert_same_run(with_block, (rec, _snapshot(fit, stage), stage), "clips of one")


def test_the_block_leaves_no_state_in_the_engine_or_the_objective():
    clips = (3, 1)
    fit, targets = _problem(clips)
    plain = trainer.Stage(2, "default", fit, targets, lr=0.02, seed=11)
    tied = _stage(fit, targets, "default", clips, 2)
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
    restore(tied)
    tied.step(0)
    assert not torch.equal(tied._adam["joint_rot"]["m"], first[1]["m_joint_rot"])          # the block did pull on something
    restore(plain)
    again = (plain.step(0).clone(), _snapshot(fit, plain))
    torch.cuda.synchronize()
    assert torch.equal(first[0], again[0])
    _assert_same_bits(first[1], again[1], "plain step after a tied one")


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_entry_point_and_change_nothing():
    clips, V = (3, 1), 70
    lib = _lib.load()
    term = _lib.resolve(lib, "smalfit_scan_sequence_vertex_term")
    seq = eng.ScanSequence(clips)
    x = dev(vc.verts(clips, V))
    losses, total = torch.full((3,), 7.0, device="cuda"), torch.zeros(1, device="cuda")
    dverts, dtrans = torch.full((4, V, 3), 7.0, device="cuda"), torch.full((4, 3), 7.0, device="cuda")

    def refused(q, text, verts=x, num_verts=V, handle=seq.handle):
        rc = term(handle, eng._stream(), None if q is None else C.byref(q), num_verts, eng._ptr(verts), eng._ptr(dverts), eng._ptr(dtrans))
        msg = lib.smalfit_last_error()
        torch.cuda.synchronize()
        assert rc == 1 and msg.startswith(b"smalfit_scan_sequence_vertex_term: ") and text in msg, msg
        assert all(bool((t == 7.0).all()) for t in (losses, dverts, dtrans))

    refused(None, b"the vertex block is NULL")
    q = seq.vertex_block(TEMPORAL_VERTS, losses)[0]
    q.losses = None
    refused(q, b"losses is NULL")
    refused(seq.vertex_block(dict(w_temp_vert_vel=float("nan")), losses)[0], b"w_temp_vert_vel is not finite")
    refused(seq.vertex_block(dict(w_temp_vert_acc=float("inf")), losses)[0], b"w_temp_vert_acc is not finite")
    refused(seq.vertex_block(TEMPORAL_VERTS, losses, total)[0], b"step_total given outside a step")
    ok = seq.vertex_block(TEMPORAL_VERTS, losses)[0]
    refused(ok, b"num_verts must be positive", num_verts=0)
    refused(ok, b"verts is NULL", verts=None)
    refused(ok, b"null argument", handle=None)

    # the step: a handle built for another N, a bad block; parameters, moments and every loss buffer keep their bits
    fit, targets = _problem(clips)
    stage = _stage(fit, targets, "default", clips)
    stage.step(0)
    torch.cuda.synchronize()
    a, sq, vq = stage._step_args(), stage._sequence_block(), stage._vertex_block()
    e = fit._engine()
    step = _lib.resolve(lib, "smalfit_scan_sequence_vertex_step")
    held = _snapshot(fit, stage)
    held.update(losses=stage.last_terms.clone(), temporal=stage.last_temporal_losses.clone(), vertex=stage.last_temporal_vertex_losses.clone(),
                total=stage._seq_total.clone(), vertex_total=stage._vert_total.clone())
    other = eng.ScanSequence((2, 3))

    def step_refused(handle, block, vblock, text):
        rc = step(handle, e.handle, stage._objective.handle, targets._dev.handle, eng._stream(), C.byref(a), None, None, None, None,
                  C.byref(block) if block is not None else None, C.byref(vblock) if vblock is not None else None)
        msg = lib.smalfit_last_error()
        torch.cuda.synchronize()
        assert rc == 1 and msg.startswith(b"smalfit_scan_sequence_vertex_step: ") and text in msg, msg
        now = _snapshot(fit, stage)
        now.update(losses=stage.last_terms, temporal=stage.last_temporal_losses, vertex=stage.last_temporal_vertex_losses,
                   total=stage._seq_total, vertex_total=stage._vert_total)
        _assert_same_bits(now, held, "refused step")

    a.adam_t = 2
    step_refused(other.handle, sq, vq, b"the sequence handle was built for another num_meshes")
    bad = seq.vertex_block(dict(w_temp_vert_acc=float("-inf")), stage._vert_step_losses, stage._vert_total)[0]
    step_refused(stage._sequence.handle, sq, bad, b"w_temp_vert_acc is not finite")
    step_refused(stage._sequence.handle, sq, None, b"the vertex block is NULL")
    step_refused(stage._sequence.handle, None, vq, b"null argument")
    a.adam_t = 0
    step_refused(stage._sequence.handle, sq, vq, b"adam_t")                                     # the step's own refusals, under this name


# ---- 5. Stage end to end ----------------------------------------------------------------------------------------------------------------
def test_stage_end_to_end(tmp_path):
    clips = (3, 1)
    fit, targets = _problem(clips)
    with pytest.raises(ValueError, match="clip_lengths"):
        trainer.Stage(1, "default", fit, targets, temporal_verts=TEMPORAL_VERTS)
    with pytest.raises(KeyError, match="unknown temporal vertex weight"):
        _stage(fit, targets, "default", clips, temporal_verts=dict(w_temp_vert=1.0))
    stage = _stage(fit, targets, "default", clips, 2, out_dir=str(tmp_path), name="tied")
    assert stage.last_temporal_vertex_losses is None
    total = stage.step(0)
    got = stage.last_temporal_vertex_losses
    assert float(total) == float(stage._vert_total[0]) and float(got[0]) > 0 and float(got[1]) > 0
    assert float(got[2]) == float(np.float32(float(got[0])) + np.float32(float(got[1])))
    assert float(stage._vert_total[0]) == float(np.float32(float(stage._seq_total[0])) + np.float32(float(got[2])))
    assert float(stage.evaluate(1)[0]) > 0 and stage.last_temporal_vertex_losses.shape == (3,)
    stage.save_npz()
    quiet = _stage(fit, targets, "default", clips, 1, temporal_verts=None, out_dir=str(tmp_path), name="quiet")
    assert quiet.last_temporal_vertex_losses is None
    quiet.step(0)
    assert quiet._vert_args is None and quiet.last_temporal_vertex_losses is None          # nothing of the block is built or called
    quiet.save_npz()
    assert sorted(np.load(tmp_path / "tied.npz", allow_pickle=True).files) == sorted(np.load(tmp_path / "quiet.npz", allow_pickle=True).files)
