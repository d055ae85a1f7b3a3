"""The frame-sharded step on the device, in ONE process (-m gpu): the three shard entry points of the C ABI and their two kernels.

  A  shard_record_kernel and shard_reduce_adam_kernel against closed forms (tests/shard_cases.py): every float of a record in
     the bits of one float32 multiply; the cross-rank sum in the bits of the float32 rank-ordered accumulator -- the contract
     "add the partial gradients in rank order" -- with NaN in every float a correct kernel never reads (beyond num_shared of a
     gathered row, the moments at step 0); Adam against the float64 replica under test_adam_segments_at_value_edges' bar
  B  smalfit_shard_local_step is evaluate + Adam on the per-frame ranges + smalfit_shard_record, bit for bit, on a shard with
     both halos, at stages 0 and 2 and in the three parameter layouts (per-frame limb scales included)
  C  every one of the 32 contiguous splits of a 6-frame clip through shard_cases.RankSim over the whole four-stage schedule:
     the ranks agree in the bits of the shared state, hold their neighbours' stepped boundary frames and add up to the oracle
     loop's loss terms after every iteration;
     gradients and loss terms add up to the float64 oracle's; the final parameters follow the unsharded HIP fit and the float64
     oracle loop.  Variants (windows of 8 and 1, per-frame scales, frozen limb scales, joint limits, masks with zeros) on four cuts
  D  RankSim gives the bits of a real two-process world (gloo) on the same problem

Bounds are the project's existing bars, or YARD = 2 x the float32 oracle's own deviation where that is larger (value_forms.bound);
with tests/golden/hip_shard_step_measured.json present every deviation also stays within RATCHET = 3 x what was recorded.
SMALFIT_WRITE_SHARD_MEASURED=<path> writes what this run measured."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import parity_cases as pc   # noqa: E402
from tests import shard_cases as sc    # noqa: E402
from tests import value_forms as vf    # noqa: E402
from tests.test_gpu_value_forms import Padded, Table, dev, ptr, stream, _same_bits   # noqa: E402,F401
from tests.test_gpu_value_forms import _stop_after_a_device_error                    # noqa: E402,F401  (autouse, here too)

HERE = os.path.dirname(os.path.abspath(__file__))
MEASURED = os.path.join(HERE, "golden", "hip_shard_step_measured.json")
PER_FRAME = ("global_rotation", "joint_rotations", "trans")


class ShardTable(Table):
    """Table with this file's record of what was measured"""

    def __init__(self, title):
        super().__init__(title)
        self.recorded = json.load(open(MEASURED)) if os.path.exists(MEASURED) else {}

    def close(self, capsys):
        with capsys.disabled():
            print("\n[%s]\n" % self.title + "\n".join(self.lines))
        path = os.environ.get("SMALFIT_WRITE_SHARD_MEASURED")
        if path:
            doc = json.load(open(path)) if os.path.exists(path) else {}
            doc.update(self.measured)
            json.dump(doc, open(path, "w"), indent=1, sort_keys=True)
        assert not self.bad, "\n".join(self.bad)
        assert self.recorded, "tests/golden/hip_shard_step_measured.json is missing: run this file with SMALFIT_WRITE_SHARD_MEASURED=<path> on a GPU box and commit the result"


def f32(t):
    return t.detach().cpu().numpy().astype(np.float32, copy=True)


def _weights(stage_id):
    from smalify_amd import config as cfg
    W = np.array(cfg.OPT_WEIGHTS).T
    return W[stage_id][:6].copy(), float(W[stage_id][6]), float(W[stage_id][8])


# ------------------------------------------------------------------------------------------------
# A. the two kernels against closed forms
# ------------------------------------------------------------------------------------------------
_BLANK = {}


def _blank_fitter(M):
    """a FusedFitter of M frames whose targets are never looked at (boundary_records reads parameters and masks only)"""
    from smalify_amd import fitter as fit
    if M not in _BLANK:
        e, _, _ = pc.get_engine(8, 64)
        _BLANK[M] = fit.FusedFitter(e, np.zeros((M, 25, 2), np.float32), np.zeros((M, 25), np.float32),
                                    np.zeros((M, 64, 64), np.float32), 2)
    return _BLANK[M]


@pytest.mark.parametrize("M", sc.RECORD_NUM_FRAMES)
@pytest.mark.parametrize("ns", sc.RECORD_NUM_SHARED)
def test_record_is_one_multiply_per_float(ns, M):
    from smalify_amd import engine as eng
    c = sc.record_case(ns, M)
    d = {k: dev(v) for k, v in c.items()}
    out = Padded(ns + 216)
    eng.shard_record(ns, d["shared_grad"], M, d["grot"], d["jrot"], d["trans"], d["gmask"], d["rmask"], out.t)
    torch.cuda.synchronize()
    assert out.intact(), "a write outside the record"
    got, want = f32(out.t), sc.record_reference(ns, **c)
    assert _same_bits(got[:ns], want[:ns]), "the partial shared gradient is not copied verbatim"
    assert _same_bits(got[ns:ns + 108], want[ns:ns + 108]), "first frame's block"
    assert _same_bits(got[ns + 108:], want[ns + 108:]), "last frame's block"
    if M == 1:
        assert _same_bits(got[ns:ns + 108], got[ns + 108:])          # one frame is the first and the last
    else:
        assert not _same_bits(got[ns:ns + 108], got[ns + 108:])
    # FusedFitter.boundary_records (the torch path of the initial gather) on the same state: the same 216 floats
    f = _blank_fitter(M)
    f.p["global_rotation"].copy_(d["grot"])
    f.p["joint_rotations"].copy_(d["jrot"].view(M, 34, 3))
    f.p["trans"].copy_(d["trans"])
    f.global_mask.copy_(d["gmask"])
    f.rotation_mask.copy_(d["rmask"].view(34, 3))
    assert _same_bits(f32(f.boundary_records()).reshape(-1), want[ns:])
    into = Padded(216)
    f.boundary_records(out=into.t)
    assert into.intact() and _same_bits(f32(into.t), want[ns:])


@pytest.mark.parametrize("case", sc.REDUCE_CASES, ids=lambda c: "w%d-ns%d-%s-%s-step%d" % c)
def test_reduce_adds_in_rank_order_and_steps_the_trained_floats(case, capsys):
    from smalify_amd import engine as eng
    c = sc.reduce_case(*case)
    name = "w%d-ns%d-%s-%s-step%d" % case
    world, ns, stride, ntrain, step, rows = c["world"], c["ns"], c["stride"], c["ntrain"], c["step"], c["rows"]
    lr, b1, b2, eps = vf.ADAM_HYPER
    n = ns + 40
    g_before = np.random.RandomState(3).randn(n).astype(np.float32)
    P, Mo, V = Padded(n, fill=c["param"]), Padded(n, fill=c["exp_avg_in"]), Padded(n, fill=c["exp_avg_sq_in"])
    G = Padded(n, fill=g_before)
    gathered = dev(c["gathered"])
    assert bool(torch.isnan(gathered[:, ns:]).all())
    a = eng.make_adam_args(P.t, G.t, Mo.t, V.t, [], lr, step=step, beta1=b1, beta2=b2, eps=eps)
    eng.shard_reduce_step(world, stride, gathered, ns, ntrain, a)
    torch.cuda.synchronize()
    assert a.step == step                                            # the caller closes the iteration
    assert P.intact() and Mo.intact() and V.intact() and G.intact(), "a write outside a buffer"
    g = f32(G.t)
    # ---- the sum: the contract's bits, inside the standard bound of the float64 sum ---------------------------------
    want_g = sc.rank_ordered_sum_f32(rows)
    assert np.isfinite(g[:ns]).all(), "a float beyond num_shared of a gathered row entered a sum"
    assert _same_bits(g[:ns], want_g), "not the float32 sum in rank order: columns %s" % np.nonzero(g[:ns] != want_g)[0][:8]
    assert (np.abs(g[:ns].astype(np.float64) - sc.sum_f64(rows)) <= sc.sum_bound(rows)).all()
    assert _same_bits(g[ns:], g_before[ns:]), "the gradient beyond num_shared changed"
    # ---- Adam on [0, ntrain), nothing beyond ---------------------------------------------------------------------
    table = ShardTable("smalfit_shard_reduce_step / " + name)
    want = vf.adam_reference(c["param"][:ntrain], want_g[:ntrain], c["exp_avg"][:ntrain], c["exp_avg_sq"][:ntrain], step + 1)
    for nme, buf, ref, before in zip(("param", "exp_avg", "exp_avg_sq"), (P, Mo, V), want,
                                     (c["param"], c["exp_avg_in"], c["exp_avg_sq_in"])):
        got = f32(buf.t)
        if ntrain:
            assert np.isfinite(got[:ntrain]).all(), "%s: a stale moment was read at step 0" % nme
            table.add("reduce/%s/%s" % (name, nme), vf.rel(got[:ntrain], ref), float("nan"), "adam", False)
        assert _same_bits(got[ntrain:], before[ntrain:]), "%s changed beyond num_trainable" % nme
    still = c["zero"] & (np.arange(ns) < ntrain)                     # zero summed gradient on zero moments: the parameter's bits stay
    assert _same_bits(f32(P.t)[:ns][still], c["param"][:ns][still])
    if ntrain:
        table.close(capsys)


# ------------------------------------------------------------------------------------------------
# B. local_step is its parts
# ------------------------------------------------------------------------------------------------
def _priors(e, unity):
    from smalify_amd import synthetic
    from tests import image_batch_cases as ic
    e.set_pose_prior(*synthetic.synthetic_pose_prior())
    e.set_shape_prior(*(synthetic.synthetic_shape_prior() if unity else ic.shape_prior_20()))


def _new_engine(frames, unity=True, size=64):
    from smalify_amd import engine as eng
    _, _, dm = pc.get_model()
    e = eng.Engine(dm, frames, size)
    _priors(e, unity)
    return e


def _shard_fitter(e, cur, tg, lo, hi, total, window, unity=True, allow_limb_scaling=True, joint_limits=False, masks=None):
    """the FusedFitter of frames [lo, hi) of the clip (cur, tg) on engine e"""
    from smalify_amd import fitter as fit
    f = fit.FusedFitter(e, tg["tj"][lo:hi], tg["vis"][lo:hi], tg["tsil"][lo:hi], window, unity, cur["betas"],
                        cur["log_beta_scales"] if unity else None, allow_limb_scaling=allow_limb_scaling, frame_offset=lo, total_frames=total)
    for k in PER_FRAME:
        f.p[k].copy_(dev(cur[k][lo:hi]))
    if not unity:
        f.p["log_beta_scales"].copy_(dev(cur["log_beta_scales"][lo:hi]))
    if joint_limits:
        f.enable_joint_limits()
    if masks is not None:
        f.global_mask.copy_(dev(masks[0]))
        f.rotation_mask.copy_(dev(masks[1]))
    return f


@pytest.fixture(scope="module")
def clip8():
    """tests/test_gpu_sharded.py's 8-frame problem (targets rendered by the engine itself)"""
    from tests import test_gpu_sharded as tgs
    return tgs._problem(8)


def _frame_record(cur, n):
    return np.concatenate([cur["global_rotation"][n], cur["joint_rotations"][n].reshape(-1), cur["trans"][n]]).astype(np.float32)


@pytest.mark.parametrize("layout", sc.LOCAL_STEP_LAYOUTS, ids=lambda l: l[0])
@pytest.mark.parametrize("stage_id", sc.LOCAL_STEP_STAGES)
def test_local_step_is_evaluate_adam_and_record(stage_id, layout, clip8):
    from smalify_amd import engine as eng
    _, unity, limb = layout
    cur, tg = clip8
    cur = dict(cur)
    total, window, (lo, hi) = sc.LOCAL_STEP_CLIP["frames"], sc.LOCAL_STEP_CLIP["window"], sc.LOCAL_STEP_CLIP["shard"]
    if not unity:
        cur["log_beta_scales"] = (cur["log_beta_scales"][None] + 0.02 * np.random.RandomState(5).randn(total, 6)).astype(np.float32)
    weights, w_temp, lr = _weights(stage_id)
    rs = np.random.RandomState(17)
    pair = []
    for _ in range(2):                                               # the local_step fitter and its twin on a second engine
        f = _shard_fitter(_new_engine(hi - lo, unity), cur, tg, lo, hi, total, window, unity, limb)
        f.halo_prev, f.halo_next = dev(_frame_record(cur, lo - 1)), dev(_frame_record(cur, hi))
        f.begin_stage(stage_id)
        pair.append(f)
    one, twin = pair
    ns = one.num_shared()
    assert ns == (26 if unity else 20) and one.ls_shared == unity
    local, ntrain = one._split_trainable(one.trainable(stage_id))
    in_local = np.zeros(one.flat.numel(), bool)
    for b, e_ in one._segments(local):
        in_local[b:e_] = True
    assert not in_local[:ns].any() and in_local.any()
    stale = [rs.randn(one.flat.numel()).astype(np.float32) for _ in range(3)]
    for f in pair:                                                   # the same stale gradient and moments on both sides
        f.grad.copy_(dev(stale[0]))
        f.exp_avg.copy_(dev(stale[1]))
        f.exp_avg_sq.copy_(dev(np.abs(stale[2])))
    for step_count in (0, 1):                                        # a stage's first step (moments not read), then one that reads them
        one.step_count = twin.step_count = step_count
        before = {k: f32(t) for k, t in (("flat", one.flat), ("m", one.exp_avg), ("v", one.exp_avg_sq))}
        rec = Padded(ns + 216)
        one.local_step(weights, w_temp, lr, stage_id, rec.t)
        twin.evaluate(weights, w_temp, stage_id)
        twin.apply_adam(local, lr)
        twin.step_count = step_count
        rec2 = Padded(ns + 216)
        eng.shard_record(ns, twin.grad, twin.N, twin.p["global_rotation"], twin.p["joint_rotations"], twin.p["trans"],
                         twin.global_mask, twin.rotation_mask, rec2.t)
        torch.cuda.synchronize()
        assert one.e.status() == 0 and twin.e.status() == 0
        assert rec.intact() and rec2.intact()
        assert one.step_count == step_count                          # shared_step closes the iteration, not local_step
        flat, m, v = f32(one.flat), f32(one.exp_avg), f32(one.exp_avg_sq)
        assert _same_bits(flat, f32(twin.flat)), "parameters"
        assert _same_bits(m[in_local], f32(twin.exp_avg)[in_local]) and _same_bits(v[in_local], f32(twin.exp_avg_sq)[in_local]), "moments"
        assert _same_bits(f32(one.grad)[:ns], f32(twin.grad)[:ns]), "partial shared gradient"
        assert _same_bits(f32(rec.t), f32(rec2.t)), "record"
        assert _same_bits(f32(one.losses), f32(twin.losses)), "losses"
        # the shared parameters and their moments are the reduce step's to move
        assert _same_bits(flat[:ns], before["flat"][:ns]) and _same_bits(m[:ns], before["m"][:ns]) and _same_bits(v[:ns], before["v"][:ns])
        assert _same_bits(flat[~in_local], before["flat"][~in_local])
        assert (flat[in_local] != before["flat"][in_local]).mean() > 0.9, "the per-frame parameters did not move"
        # the record: the partial gradient as the evaluation left it, the boundary frames AFTER the step
        p = {k: f32(one.p[k]) for k in PER_FRAME}
        want = sc.record_reference(ns, f32(one.grad), p["global_rotation"], p["joint_rotations"], p["trans"],
                                   f32(one.global_mask), f32(one.rotation_mask))
        assert _same_bits(f32(rec.t), want)
        o_g = one.offsets["global_rotation"][0]
        assert not _same_bits(f32(rec.t)[ns:ns + 3], before["flat"][o_g:o_g + 3]), "the record holds the frames before the step"
        if stage_id == 0:
            assert _same_bits(f32(rec.t)[:ns], stale[0][:ns])        # stage 0 forms no shared gradient: the buffer travels as it is
        if not unity:
            o, cnt = one.offsets["log_beta_scales"]
            assert (o, cnt) == (20, (hi - lo) * 6)
            moved = flat[o:o + cnt] != before["flat"][o:o + cnt]
            assert moved.all() if stage_id else not moved.any()      # per-frame scales are stepped locally, from stage 1 on


# ------------------------------------------------------------------------------------------------
# C. every cut of a short clip
# ------------------------------------------------------------------------------------------------
_ENGINES = {}


def _pool_engine(frames, slot, unity):
    """one small engine per rank, kept across splits (a rank of n frames takes the next free engine of that size)"""
    key = (frames, slot, unity)
    if key not in _ENGINES:
        _ENGINES[key] = _new_engine(frames, unity)
    e = _ENGINES[key]
    e.reset_raster_cache()
    e.clear_joint_limits()
    return e


def _rank_fitters(split, cur, tg, total, window, **layout):
    used, out = {}, []
    unity = layout.get("unity", True)
    for lo, hi in split:
        slot = used[hi - lo] = used.get(hi - lo, -1) + 1
        out.append(_shard_fitter(_pool_engine(hi - lo, slot, unity), cur, tg, lo, hi, total, window, **layout))
    return out


def _rel(a, b):
    return vf.rel(np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1))


def _term_errs(terms, ref):
    """test_gpu_eval_fixtures' rule: a term is held to itself, or to 1e-3 x the objective when it is a negligible part of it"""
    scale = abs(ref.sum())
    return {t: abs(terms[i] - ref[i]) / max(abs(ref[i]), 1e-3 * scale) for i, t in enumerate(vf.LOSS_NAMES)
            if not (ref[i] == 0.0 and terms[i] == 0.0)}


class ClipRefs:
    """the references of one clip / layout, computed once: the float64 oracle loop, the float32 oracle loop (the yardstick), the
    oracle's evaluation of the start state in both precisions, and the unsharded HIP fit"""

    def __init__(self, frames=None, window=None, unity=True, allow_limb_scaling=True, joint_limits=False, masks=False):
        self.total = sc.CLIP["frames"] if frames is None else frames
        self.window = sc.CLIP["window"] if window is None else window
        self.masks = sc.variant_masks() if masks else None
        self.layout = dict(unity=unity, allow_limb_scaling=allow_limb_scaling, joint_limits=joint_limits, masks=self.masks)
        self.cur, self.tg, make_prob = sc.clip_problem(self.total, self.window, unity, joint_limits)
        p64, p32 = make_prob(torch.float64), make_prob(torch.float32)
        self.final64, self.trace64 = sc.oracle_loop(p64, self.cur, sc.SCHEDULE, allow_limb_scaling, self.masks)
        self.final32, self.trace32 = sc.oracle_loop(p32, self.cur, sc.SCHEDULE, allow_limb_scaling, self.masks)
        self.start64 = sc.oracle_eval(p64, self.cur, sc.START_STAGE, self.masks)
        self.start32 = sc.oracle_eval(p32, self.cur, sc.START_STAGE, self.masks)
        self.yard_final = {k: _rel(self.final32[k], self.final64[k]) for k in self.final64}
        # the unsharded HIP fit: one FusedFitter over the whole clip, one library call per iteration
        f = _shard_fitter(_pool_engine(self.total, 0, unity), self.cur, self.tg, 0, self.total, self.total, self.window, **self.layout)
        for stage_id, its in sc.SCHEDULE:
            f.begin_stage(stage_id)
            w, w_temp, lr = _weights(stage_id)
            for _ in range(its):
                f.step(w, w_temp, lr, stage_id)
        assert f.e.status() == 0
        self.hip = {k: f32(v) for k, v in f.p.items()}


_REFS = {}


def _refs(name=None):
    if name not in _REFS:
        _REFS[name] = ClipRefs(**(sc.VARIANTS[name] if name else {}))
    return _REFS[name]


def _bits_equal_on_device(tensors):
    stack = torch.stack([t.view(torch.int32) for t in tensors])
    return bool((stack == stack[0]).all())


def _run_split(split, refs, table, tag):
    """one RankSim over `split`: the checks after every iteration, the start state's evaluation against the oracle, the final
    parameters against the unsharded fit and the float64 oracle loop"""
    cur, total = refs.cur, refs.total
    fitters = _rank_fitters(split, cur, refs.tg, total, refs.window, **refs.layout)
    sim = sc.RankSim(fitters)
    assert not sim.generic
    ns = sim.start()
    world = len(split)
    assert tuple(sim.gather.shape) == (world, ns + 216) and ns == (26 if refs.layout["unity"] else 20)
    # ---- the start state, where every rank still holds the oracle's parameters: one evaluation with every term on ------------
    # (the run's own first iteration is stage 0's, which forms no shared gradient and no silhouette term: stage 2's weights on the
    # same state, halos in place, ask for all of them; part B ties local_step to this evaluation bit for bit)
    w, w_temp, _ = _weights(sc.START_STAGE)
    names = vf.PARAMS
    terms = np.zeros(9)
    shared = np.zeros(ns)
    per_frame = {k: [] for k in names if k not in ("betas",) and not (k == "log_beta_scales" and refs.layout["unity"])}
    for f in fitters:
        f.evaluate(w, w_temp, sc.START_STAGE, want=names)
        terms += f.losses.cpu().numpy().astype(np.float64)[:9]
        shared += f.grad[:ns].cpu().numpy().astype(np.float64)
        for k in per_frame:
            per_frame[k].append(f.g[k].cpu().numpy().astype(np.float64).reshape(f.N, -1))
        assert f.e.status() == 0
    t64, g64 = refs.start64
    t32, g32 = refs.start32
    cat = lambda g: np.concatenate([g["betas"].reshape(-1), g["log_beta_scales"].reshape(-1)])[:ns] if refs.layout["unity"] else g["betas"].reshape(-1)  # noqa: E731
    table.add("%s/start/d_shared" % tag, _rel(shared, cat(g64)), _rel(cat(g32), cat(g64)), "grad", True)
    for k, rows in per_frame.items():
        table.add("%s/start/d_%s" % (tag, k), _rel(np.concatenate(rows, 0), g64[k]), _rel(g32[k], g64[k]), "grad", True)
    e_hip, e_32 = _term_errs(terms, t64), _term_errs(t32, t64)
    for t, err in e_hip.items():
        table.add("%s/start/%s" % (tag, t), err, e_32.get(t, float("nan")), "term", False)
    # ---- the schedule --------------------------------------------------------------------------------------------
    done, worst = 0, {}
    for stage_id, its in sc.SCHEDULE:
        sim.begin_stage(stage_id)
        w, w_temp, lr = _weights(stage_id)
        for it in range(its):
            sim.step(w, w_temp, lr, stage_id)
            where = "%s stage %d iteration %d" % (tag, stage_id, it)
            # the ranks' loss terms of this iteration add up to the oracle loop's at the same iteration (largest deviation kept)
            summed = torch.stack(sim.losses).double().sum(0).cpu().numpy()[:9]
            e_hip = _term_errs(summed, refs.trace64[done]["terms"])
            e_32 = _term_errs(refs.trace32[done]["terms"], refs.trace64[done]["terms"])
            for t, err in e_hip.items():
                old = worst.get(t, (0.0, 0.0))
                worst[t] = (max(old[0], err), max(old[1], e_32.get(t, 0.0)))
            done += 1
            for buf in ("flat", "exp_avg", "exp_avg_sq"):            # the shared state: the same bits on every rank
                assert _bits_equal_on_device([getattr(f, buf)[:ns] for f in fitters]), (where, buf)
            gather = sim.gather.cpu().numpy()
            assert np.isfinite(gather).all(), where
            for r, f in enumerate(fitters):
                # the row's boundary part is rank r's first and last frame as they are NOW, masks applied
                p = {k: f32(f.p[k]) for k in PER_FRAME}
                want = sc.record_reference(0, np.zeros(1), p["global_rotation"], p["joint_rotations"], p["trans"],
                                           f32(f.global_mask), f32(f.rotation_mask))
                assert _same_bits(gather[r, ns:], want), (where, r)
                assert (f.halo_prev is None) == (r == 0) and (f.halo_next is None) == (r == world - 1), (where, r)
                if r > 0:                                            # ... and the neighbours hold exactly those blocks as their halos
                    assert f.halo_prev.data_ptr() == sim.gather[r - 1, ns + 108:].data_ptr()
                    assert _same_bits(f32(f.halo_prev), gather[r - 1, ns + 108:]), (where, r)
                if r + 1 < world:
                    assert f.halo_next.data_ptr() == sim.gather[r + 1, ns:].data_ptr()
                    assert _same_bits(f32(f.halo_next), gather[r + 1, ns:ns + 108]), (where, r)
                assert f.step_count == it + 1
    assert all(f.e.status() == 0 for f in fitters) and done == len(refs.trace64)
    for t, (err, yard) in worst.items():
        table.add("%s/loop/%s" % (tag, t), err, yard, "term", False)
    # ---- the final parameters ------------------------------------------------------------------------------------
    got = {k: np.concatenate([f32(f.p[k]).reshape(f.N, -1) for f in fitters], 0) for k in PER_FRAME}
    got["betas"] = f32(fitters[0].p["betas"])
    if refs.layout["unity"]:
        got["log_beta_scales"] = f32(fitters[0].p["log_beta_scales"])
    else:
        got["log_beta_scales"] = np.concatenate([f32(f.p["log_beta_scales"]) for f in fitters], 0)
    for k in vf.PARAMS:
        table.add("%s/final/%s/vs_unsharded" % (tag, k), _rel(got[k], refs.hip[k]), refs.yard_final[k], "sharded_vs_unsharded", False)
        table.add("%s/final/%s/vs_oracle" % (tag, k), _rel(got[k], refs.final64[k]), refs.yard_final[k], "fit_vs_oracle", False)


@pytest.mark.parametrize("split", sc.splits(sc.CLIP["frames"]), ids=sc.split_name)
def test_every_split_of_the_clip(split, capsys):
    refs = _refs()
    name = sc.split_name(split)
    table = ShardTable("6 frames, window 4, split %s: HIP ranks vs float64 oracle / unsharded HIP fit" % name)
    _run_split(split, refs, table, "split/" + name)
    table.close(capsys)


@pytest.mark.parametrize("variant", sorted(sc.VARIANTS))
def test_variants_on_four_cuts(variant, capsys):
    refs = _refs(variant)
    table = ShardTable("variant %s: HIP ranks vs float64 oracle / unsharded HIP fit" % variant)
    for sizes in sc.VARIANT_SPLITS[refs.total]:
        split = sc.split_of(sizes)
        _run_split(split, refs, table, "%s/%s" % (variant, sc.split_name(split)))
    if variant == "per_frame_scales":
        assert refs.hip["log_beta_scales"].shape == (refs.total, 6)
        assert (refs.hip["log_beta_scales"] != refs.cur["log_beta_scales"]).all()        # the scales were trained
    if variant == "no_limb_scaling":
        assert _same_bits(refs.hip["log_beta_scales"], refs.cur["log_beta_scales"])      # 20 of the 26 shared floats are stepped
    if variant == "joint_limits":
        assert refs.trace64[-1]["terms"][8] > 0                                          # the hinge is in the objective
    table.close(capsys)


# ------------------------------------------------------------------------------------------------
# D. the simulator is the real thing
# ------------------------------------------------------------------------------------------------
def test_rank_sim_gives_the_bits_of_a_two_process_world(clip8):
    """tests/test_gpu_sharded.py's two-rank case (8 frames, window 4, its SCHEDULE, gloo; each rank's step is one smalfit_shard_run
    of one iteration) against RankSim on the same problem: the same launches on the same bytes, so the same bits on both ranks --
    which extends "the C loop equals the Python loop" from a world of one to a world of two.  The only test here that starts
    further processes (two)."""
    from smalify_amd import distributed
    from tests import test_gpu_sharded as tgs
    cur, tg = clip8
    n_frames, window, world = 8, 4, 2
    torch.cuda.synchronize()
    got = tgs._spawn("gloo", world, n_frames, window, cur, tg)
    fitters = [tgs._factory(pc, cur, tg, *distributed.shard_range(n_frames, r, world, window=window), n_frames, window) for r in range(world)]
    sim = sc.RankSim(fitters)
    for stage_id, its in tgs.SCHEDULE:
        sim.begin_stage(stage_id)
        w, w_temp, lr = _weights(stage_id)
        for _ in range(its):
            sim.step(w, w_temp, lr, stage_id)
    for r, f in enumerate(fitters):
        assert f.e.status() == 0
        for k in vf.PARAMS:
            assert _same_bits(f32(f.p[k]), got[r][k]), "rank %d %s: RankSim and the two-process world differ" % (r, k)
