"""smalfit_fit_run folds gradient assembly + Adam of every iteration but the last into the next iteration's head launch
(lbs_head_step_kernel) and skips the loss sums nobody can see (-m gpu).

The arithmetic is the same operations in the same order, so the bar is bit-identity: one call of K iterations against K calls
of one iteration (a single-iteration call has nothing pending and runs assemble_kernel + adam_segments_kernel as ever) must
leave the same parameters, moments, gradients and losses."""
import numpy as np
import pytest
import torch

from . import parity_cases as pc

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 7)


def _weights():
    from smalify_amd import config as cfg
    return np.array(cfg.OPT_WEIGHTS).T


def _state(f):
    torch.cuda.synchronize()
    return {k: getattr(f, k).cpu().numpy().copy() for k in ("flat", "grad", "exp_avg", "exp_avg_sq", "losses")}


def _assert_same(a, b, what):
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), \
            "%s: %s differs in %d of %d floats" % (what, k, int((a[k].view(np.uint32) != b[k].view(np.uint32)).sum()), a[k].size)


# (stage, begin_stage first?): stage 0 trains global_rotation and trans only; the second silhouette call goes on from the
# first one's moments and step count, the first one starts from fresh moments
CALLS = ((0, True), (2, True), (2, False))


def _run_calls(f, K, whole, calls=CALLS):
    """-> the state after every call; whole: each call is ONE run of K iterations, else K runs of one"""
    W = _weights()
    out = []
    for stage, begin in calls:
        if begin:
            f.begin_stage(stage)
        w = (W[stage][:6], float(W[stage][6]), float(W[stage][8]), stage)
        if whole:
            f.run_iterations(*w, K)
        else:
            for _ in range(K):
                f.run_iterations(*w, 1)
        out.append(_state(f))
    return out


def _small_fitter(shared_scales, seed):
    """8 frames at 64^2 (the split skinning kernel); shared limb scales with the 26-dim unity prior, or per-frame limb scales
    with a 20-dim shape prior"""
    from smalify_amd import engine as eng, fitter as fit, synthetic
    _, cur, tg = pc.make_problem_cpu(8, 64, 4, seed)
    if shared_scales:
        e, _, _ = pc.get_engine(8, 64)
    else:
        _, _, dm = pc.get_model()
        e = eng.Engine(dm, 8, 64)
        e.set_pose_prior(*synthetic.synthetic_pose_prior())
        prec, mean = synthetic.synthetic_shape_prior()
        e.set_shape_prior(np.ascontiguousarray(prec[:20, :20]), np.ascontiguousarray(mean[:20]))

    def new_fitter():
        e.reset_raster_cache()
        f = fit.FusedFitter(e, tg["tj"], tg["vis"], tg["tsil"], 4, shared_scales, cur["betas"],
                            cur["log_beta_scales"] if shared_scales else None)
        for k in ("global_rotation", "joint_rotations", "trans"):
            f.p[k].copy_(pc.dev(cur[k]))
        return f
    return e, new_fitter


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("shared_scales", [True, False], ids=["shared_scales", "per_frame_scales"])
def test_one_call_of_k_iterations_equals_k_calls_of_one(shared_scales, K):
    e, new_fitter = _small_fitter(shared_scales, 41)
    ref = _run_calls(new_fitter(), K, whole=False)
    got = _run_calls(new_fitter(), K, whole=True)
    assert e.status() == 0
    for (stage, begin), a, b in zip(CALLS, ref, got):
        _assert_same(a, b, "stage %d%s, K=%d" % (stage, "" if begin else " continued", K))
    # the optimiser moved every trainable tensor (the comparison is not one of two idle fits)
    assert np.count_nonzero(got[-1]["exp_avg"]) > got[-1]["exp_avg"].size // 2


@pytest.mark.parametrize("K", KS)
def test_fold_at_64_frames(K):
    """the benchmark's size (64 frames, 256^2: the wide skinning kernel reads the translations the head launch stepped)"""
    import bench
    from smalify_amd import engine as eng, fitter as fit, synthetic
    _, _, dm = pc.get_model()
    e = eng.Engine(dm, bench.NUM_FRAMES, bench.IMAGE_SIZE)
    e.set_pose_prior(*synthetic.synthetic_pose_prior())
    gt, tj, vis, tsil, sp = bench.build_problem(e, torch, "survey")
    e.set_shape_prior(*sp)
    out = []
    for whole in (False, True):
        e.reset_raster_cache()
        f = fit.FusedFitter(e, tj, vis, tsil, bench.WINDOW, True, sp[1][:20], sp[1][20:26])
        out.append(_run_calls(f, K, whole, calls=((0, True), (2, True))))
    assert e.status() == 0
    for stage, a, b in zip((0, 2), out[0], out[1]):
        _assert_same(a, b, "64 frames, stage %d, K=%d" % (stage, K))


@pytest.mark.parametrize("K", (3, 7))
def test_graph_switch_and_profiled_run_give_the_same_state(K):
    """the captured-graph path and a profiled run keep the plain chain: the same bits as the folded loop"""
    e, new_fitter = _small_fitter(True, 43)
    ref = _run_calls(new_fitter(), K, whole=False)
    side = torch.cuda.Stream()
    for graph in (True, False):
        e.set_graph(graph)
        try:
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                got = _run_calls(new_fitter(), K, whole=True)
                side.synchronize()
        finally:
            e.set_graph(False)
        for (stage, begin), a, b in zip(CALLS, ref, got):
            _assert_same(a, b, "graph %s, stage %d%s, K=%d" % (graph, stage, "" if begin else " continued", K))
    f = new_fitter()
    e.profile_begin(3 * K)
    got = _run_calls(f, K, whole=True)
    sections = e.profile_end()
    assert sections["lbs_fwd"][1] == 3 * K
    for (stage, begin), a, b in zip(CALLS, ref, got):
        _assert_same(a, b, "profiled, stage %d%s, K=%d" % (stage, "" if begin else " continued", K))
    assert e.status() == 0


# ======================================================================================================================
# Every trainable set, layout, mask, shard and frame count the folded loop accepts or must refuse (tests/fold_forms.py names
# them; tests/test_fold_forms_cpu.py checks that the lists reach every branch).  The yardstick stays the plain chain: K calls
# of one iteration.  Targets are rendered by the engine itself (a bit comparison needs no oracle), every tensor holds distinct
# values per frame and element, and the moments, the gradients and every float between the tensors start from recognisable
# patterns, so that a float nobody may touch shows when it is touched.
# ======================================================================================================================
from . import fold_forms as ff  # noqa: E402

S_IMG = 64
SHAPES = dict(betas=lambda M, mode: (20,), log_beta_scales=lambda M, mode: (6,) if mode == 1 else (M, 6),
              joint_rotations=lambda M, mode: (M, 34, 3), global_rotation=lambda M, mode: (M, 3), trans=lambda M, mode: (M, 3))
_ENGINES, _PROBLEMS = {}, {}


def _engine(max_frames, prior_dim, tag=""):
    """an engine of this file's own (the joint-limit table and the graph switch are engine state): the 26-dim unity prior over
    betas and shared limb scales, or its 20-dim block for the fits without shared scales"""
    from smalify_amd import engine as eng, synthetic
    key = (max_frames, prior_dim, tag)
    if key not in _ENGINES:
        e = eng.Engine(pc.get_model()[2], max_frames, S_IMG)
        e.set_pose_prior(*synthetic.synthetic_pose_prior())
        prec, mean = synthetic.synthetic_shape_prior()
        e.set_shape_prior(np.ascontiguousarray(prec[:prior_dim, :prior_dim]), np.ascontiguousarray(mean[:prior_dim]))
        _ENGINES[key] = e
    return _ENGINES[key]


def _problem(M, seed=51):
    """start parameters (distinct per frame and element; limb scales shared and per frame) and targets rendered on the GPU from
    a ground-truth pose nearby"""
    from smalify_amd import fitter as fit
    if (M, seed) in _PROBLEMS:
        return _PROBLEMS[(M, seed)]
    gt, cur = pc.random_pose(M, seed), pc.random_pose(M, seed)
    rs = np.random.RandomState(seed + 7)
    cur["global_rotation"] += (0.05 * rs.randn(M, 3)).astype(np.float32)
    cur["joint_rotations"] += (0.08 * rs.randn(M, 34, 3)).astype(np.float32)
    cur["trans"] += (0.02 * rs.randn(M, 3)).astype(np.float32)
    cur["betas"] += (0.1 * rs.randn(20)).astype(np.float32)
    cur["log_beta_scales_per_frame"] = (cur["log_beta_scales"][None] + 0.1 * rs.randn(M, 6)).astype(np.float32)
    e = _engine(max(M, 8), 26)
    f = fit.FusedFitter(e, np.zeros((M, 25, 2), np.float32), np.ones((M, 25), np.float32), np.zeros((M, S_IMG, S_IMG), np.float32),
                        4, True, gt["betas"], gt["log_beta_scales"])
    for k in ("global_rotation", "joint_rotations", "trans"):
        f.p[k].copy_(pc.dev(gt[k]))
    _, sil, proj = f.snapshot()
    vis = (rs.rand(M, 25) < 0.85).astype(np.float32)
    vis[:, [2, 5, 8]] = 1.0
    tg = dict(tj=(proj.cpu().numpy() + rs.randn(M, 25, 2)).astype(np.float32), vis=vis, tsil=(sil > 0.5).float().cpu().numpy())
    assert 0.02 < tg["tsil"].mean() < 0.9
    halos = [np.concatenate([cur["global_rotation"][i] + 0.03, cur["joint_rotations"][i].reshape(-1) - 0.02, cur["trans"][i] + 0.01])
             for i in (0, M - 1)]
    tg["halo_prev"], tg["halo_next"] = (h.astype(np.float32) for h in halos)
    _PROBLEMS[(M, seed)] = (cur, tg)
    return cur, tg


def _pattern(n, which):
    """n floats no kernel writes by accident: distinct, non-zero, of a gradient's size (which = 3: positive, a second moment)"""
    i = np.arange(n, dtype=np.float64)
    x = 1e-3 * (1.0 + which) * (1.5 + np.sin(0.37 * i + which))
    return torch.from_numpy((x if which == 3 else x * np.where(i % 2, -1.0, 1.0)).astype(np.float32)).cuda()


class EngineCase:
    """One fit through Engine.build_fit_args + make_adam_args + Engine.fit_run on this test's own flat buffers.
    mode: logscale_mode; train / want: trained tensors / tensors whose gradient is asked for; order, pad: the buffer's layout;
    ranges: the optimiser's (default: the trained tensors, adjacent ones merged); outside: tensors in a buffer of their own;
    separate_grad: tensors whose gradient goes to a buffer of its own"""

    def __init__(self, M=8, mode=1, train=ff.TENSORS, want=None, order=None, pad=0, ranges=None, outside=(), separate_grad=(),
                 stage=2, w_betas=None, masks=None, limits=False, halos=False, frame_offset=0, total_frames=0, window=4,
                 graph=False, seed=51):
        self.M, self.mode = M, mode
        every = [k for k in ff.TENSORS if not (k == "log_beta_scales" and mode == 0)]
        self.train = tuple(k for k in every if k in train)
        self.want = self.train if want is None else tuple(k for k in every if k in want)
        self.offs, self.size = ff.layout(M, mode, order, pad)
        self.ranges = ff.merged_ranges(self.offs, self.train) if ranges is None else list(ranges)
        self.outside, self.separate_grad = tuple(outside), tuple(separate_grad)
        W = _weights()[stage]
        self.weights, self.w_temp, self.lr = W[:6].copy(), float(W[6]), float(W[8])
        if w_betas is not None:
            self.weights[2] = w_betas
        self.limits = limits
        if not limits:
            self.weights[4] = 0.0
        self.masks, self.halos, self.graph, self.window = masks, halos, graph, window
        self.frame_offset, self.total_frames, self.seed = frame_offset, total_frames, seed
        self.e = _engine(max(M, 8), 26 if mode == 1 else 20, "limits" if limits else "")

    def run(self, K, whole, calls=2):
        """-> (the buffers before the first call, the state after each call: fresh moments, then continued)"""
        from smalify_amd import engine as eng, model_io
        M, mode, e = self.M, self.mode, self.e
        cur, tg = _problem(M, self.seed)
        e.reset_raster_cache()
        flat, grad, m, v = (_pattern(self.size, w) for w in range(4))
        values = dict(cur, log_beta_scales=cur["log_beta_scales"] if mode == 1 else cur["log_beta_scales_per_frame"])
        p, g, extra = {}, {}, {}
        for k, (o, c) in self.offs.items():
            shape = SHAPES[k](M, mode)
            if k in self.outside:
                p[k] = extra["param_" + k] = pc.dev(values[k]).reshape(shape).clone()
            else:
                p[k] = flat[o:o + c].view(shape)
                p[k].copy_(pc.dev(values[k]).reshape(shape))
            if k in self.separate_grad:
                g[k] = extra["grad_" + k] = _pattern(c, 1).view(shape).clone()
            else:
                g[k] = grad[o:o + c].view(shape)
        gm, rm = (None, None) if self.masks is None else (pc.dev(self.masks[0]), pc.dev(self.masks[1]))
        hp, hn = (pc.dev(tg["halo_prev"]), pc.dev(tg["halo_next"])) if self.halos else (None, None)
        if self.limits:
            e.set_joint_limits(*model_io.joint_limit_table())
        losses = torch.zeros(eng.NUM_LOSS_TERMS, device="cuda")
        a, _, _, keep = e.build_fit_args(
            betas=p["betas"], log_beta_scales=p.get("log_beta_scales"), global_rotation=p["global_rotation"],
            joint_rotations=p["joint_rotations"], trans=p["trans"], target_joints=pc.dev(tg["tj"]),
            target_visibility=pc.dev(tg["vis"]), target_sil=pc.dev(tg["tsil"]), weights=self.weights, w_temp=self.w_temp,
            window=self.window, temporal=True, global_mask=gm, rotation_mask=rm, halo_prev=hp, halo_next=hn, losses=losses,
            grads=g, want=self.want, frame_offset=self.frame_offset, total_frames=self.total_frames)
        aa = eng.make_adam_args(flat, grad, m, v, self.ranges, self.lr)
        # what plan_fold sees: every tensor's place relative to the flat buffer, and where its gradient goes
        self.offsets = {k: (p[k].data_ptr() - flat.data_ptr()) // 4 for k in p}
        self.grad_at_offset = {k: k in self.want and g[k].data_ptr() == grad.data_ptr() + 4 * self.offsets[k] for k in p}

        def state():
            torch.cuda.synchronize()
            st = dict(flat=flat, grad=grad, exp_avg=m, exp_avg_sq=v, losses=losses, **extra)
            return {k: t.detach().cpu().numpy().reshape(-1).copy() for k, t in st.items()}

        before, out = state(), []
        e.set_graph(self.graph)
        try:
            for _ in range(calls):
                if whole:
                    e.fit_run(a, aa, K)
                else:
                    for _ in range(K):
                        e.fit_run(a, aa, 1)
                out.append(state())
        finally:
            e.set_graph(False)
        assert aa.step == calls * K and e.status() == 0
        del keep
        return before, out

    def plan(self):
        return ff.plan_fold(self.M, self.mode, self.offsets, self.ranges, self.grad_at_offset)

    def in_ranges(self):
        sel = np.zeros(self.size, bool)
        for b, en in self.ranges:
            sel[b:en] = True
        return sel

    def check(self, K, expect, what):
        """the folded (or refused) call against K calls of one iteration, bit for bit, after a fresh and a continued call;
        expect: 'folded', or the reason plan_fold must refuse the layout with"""
        before, ref = self.run(K, whole=False)
        _, got = self.run(K, whole=True)
        ok, train, why = self.plan()
        if expect == "folded":
            assert ok and {k for k in train if train[k]} == set(self.train), (what, why, train)
        else:
            assert not ok and why == expect, (what, why)
        assert ff.path(K, self.graph, False, True, ok) == ("folded" if expect == "folded" else "plain"), what
        for i, (a, b) in enumerate(zip(ref, got)):
            _assert_same(a, b, "%s, K=%d%s" % (what, K, " continued" if i else ""))
        # nobody touched a float outside the optimiser's ranges, or a gradient nobody asked for
        sel = self.in_ranges()
        for k in ("flat", "exp_avg", "exp_avg_sq"):
            assert np.array_equal(got[-1][k][~sel].view(np.uint32), before[k][~sel].view(np.uint32)), (what, k, "outside the ranges")
        wanted = np.zeros(self.size, bool)
        for k in self.want:
            if k not in self.separate_grad:
                wanted[self.offs[k][0]:self.offs[k][0] + self.offs[k][1]] = True
        assert np.array_equal(got[-1]["grad"][~(wanted | sel)].view(np.uint32), before["grad"][~(wanted | sel)].view(np.uint32)), (what, "grad")
        for k in self.outside:
            assert np.array_equal(got[-1]["param_" + k].view(np.uint32), before["param_" + k].view(np.uint32)), (what, k, "outside")
        # the optimiser moved what it trains
        for k in self.train:
            if k in self.outside:
                continue
            o, c = self.offs[k]
            assert np.count_nonzero(got[-1]["exp_avg"][o:o + c]) > c // 2, (what, k, "did not move")
            assert not np.array_equal(got[-1]["flat"][o:o + c], before["flat"][o:o + c]), (what, k)
        return before, got


# ---- a. trainable sets through FusedFitter ----------------------------------------------------------------------------
def _fitter_case(shared_scales, allow_limb_scaling, seed=53):
    from smalify_amd import fitter as fit
    M = 8
    cur, tg = _problem(M, seed)
    e = _engine(8, 26 if shared_scales else 20)

    def new_fitter():
        e.reset_raster_cache()
        f = fit.FusedFitter(e, tg["tj"], tg["vis"], tg["tsil"], 4, shared_scales, cur["betas"],
                            cur["log_beta_scales"] if shared_scales else None, allow_limb_scaling=allow_limb_scaling)
        for k in ("global_rotation", "joint_rotations", "trans"):
            f.p[k].copy_(pc.dev(cur[k]))
        if not shared_scales:
            f.p["log_beta_scales"].copy_(pc.dev(cur["log_beta_scales_per_frame"]))
        for w, t in enumerate((f.grad, f.exp_avg, f.exp_avg_sq)):
            t.copy_(_pattern(t.numel(), w + 1))
        return f
    return e, new_fitter


def _check_fitter(e, new_fitter, stage, K, what):
    calls = ((stage, True), (stage, False))
    f0 = new_fitter()
    before = _state(f0)
    ref = _run_calls(f0, K, whole=False, calls=calls)
    f1 = new_fitter()
    got = _run_calls(f1, K, whole=True, calls=calls)
    assert e.status() == 0
    names = f1.trainable(stage)
    offs = {k: o for k, (o, _) in f1.offsets.items()}
    ranges = [tuple(s) for s in f1._segments(names)]
    mode = 1 if f1.ls_shared else 2
    ok, train, why = ff.plan_fold(f1.N, mode, offs, ranges, {k: k in names for k in offs})
    assert ok and {k for k in train if train[k]} == set(names), (what, why)
    assert ff.path(K, False, False, True, ok) == "folded"
    for i, (a, b) in enumerate(zip(ref, got)):
        _assert_same(a, b, "%s, stage %d%s, K=%d" % (what, stage, " continued" if i else "", K))
    sel = np.zeros(f1.flat.numel(), bool)
    for b, en in ranges:
        sel[b:en] = True
    for k in ("flat", "exp_avg", "exp_avg_sq", "grad"):
        assert np.array_equal(got[-1][k][~sel].view(np.uint32), before[k][~sel].view(np.uint32)), (what, stage, k, "outside the ranges")
    for k in names:
        o, c = f1.offsets[k]
        assert np.count_nonzero(got[-1]["exp_avg"][o:o + c]) > c // 2, (what, stage, k, "did not move")


@pytest.mark.parametrize("K", ff.KS)
@pytest.mark.parametrize("stage", (0, 1, 3))
@pytest.mark.parametrize("shared_scales", [True, False], ids=["shared_scales", "per_frame_scales"])
def test_fitter_without_limb_scaling(shared_scales, stage, K):
    """allow_limb_scaling=False: the limb scales -- shared with the unity prior, else per frame and different in every frame --
    are read by every pending step and trained by none; in stage 0 the betas too"""
    e, new_fitter = _fitter_case(shared_scales, False)
    assert "log_beta_scales" not in new_fitter().trainable(stage)
    _check_fitter(e, new_fitter, stage, K, "no limb scaling, " + ("shared" if shared_scales else "per frame"))


@pytest.mark.parametrize("K", ff.KS)
@pytest.mark.parametrize("stage", (1, 3))
@pytest.mark.parametrize("shared_scales", [True, False], ids=["shared_scales", "per_frame_scales"])
def test_default_fitter_stages_1_and_3(shared_scales, stage, K):
    e, new_fitter = _fitter_case(shared_scales, True)
    _check_fitter(e, new_fitter, stage, K, "default fitter")


# ---- b. trainable sets through the engine -------------------------------------------------------------------------------
_SETS = [(mode, name) for mode in (0, 1, 2) for name in ff.trainable_sets(mode)]


@pytest.mark.parametrize("K", (2, 3, 6))
@pytest.mark.parametrize("mode,name", _SETS, ids=["mode%d-%s" % s for s in _SETS])
def test_engine_trainable_sets(mode, name, K):
    """every tensor alone, the shared pair, all but the limb scales (two ranges with a gap), all, and gradients asked of tensors
    nobody trains -- without limb scales (logscale_mode 0), with shared (1) and with per-frame ones (2).  The same tensors in
    another order in the flat buffer are accepted too and give the same bits."""
    train, want = ff.trainable_sets(mode)[name]
    case = EngineCase(mode=mode, train=train, want=want)
    _, got = case.check(K, "folded", "mode %d, %s" % (mode, name))
    other = EngineCase(mode=mode, train=train, want=want, order=ff.TENSORS[::-1])
    assert other.offs != case.offs
    _, got2 = other.check(K, "folded", "mode %d, %s, reversed buffer" % (mode, name))
    for k, (o, c) in case.offs.items():
        o2 = other.offs[k][0]
        for buf in ("flat", "exp_avg", "exp_avg_sq") if k in train else ("flat",):
            assert np.array_equal(got[-1][buf][o:o + c].view(np.uint32), got2[-1][buf][o2:o2 + c].view(np.uint32)), (mode, name, k, buf)
        if k in want:
            assert np.array_equal(got[-1]["grad"][o:o + c].view(np.uint32), got2[-1]["grad"][o2:o2 + c].view(np.uint32)), (mode, name, k)
    assert np.array_equal(got[-1]["losses"].view(np.uint32), got2[-1]["losses"].view(np.uint32))


@pytest.mark.parametrize("K", (2, 3, 4))
@pytest.mark.parametrize("mode", (0, 1, 2))
def test_betas_trained_without_a_shape_prior(mode, K):
    """w_betas == 0: the launch has no prior block and the pending step no prior share to add"""
    for train in (("betas",), ff.TENSORS):
        case = EngineCase(mode=mode, train=train, w_betas=0.0)
        _, got = case.check(K, "folded", "mode %d, w_betas = 0, %s" % (mode, "+".join(case.train)))
        assert got[-1]["losses"][3] == 0.0


# ---- c. refused layouts ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (2, 3, 4))
@pytest.mark.parametrize("name,why", ff.REFUSED, ids=[n for n, _ in ff.REFUSED])
@pytest.mark.parametrize("mode", (1, 2))
def test_refused_layouts_run_the_plain_chain(mode, name, why, K):
    """layouts plan_fold must refuse: one call of K iterations still equals K calls of one (the plain chain runs), and the
    floats outside the ranges stay as they were.  With the gradient of `trans` written to a buffer of its own, Adam steps
    `trans` by what adam.grad holds there -- the pattern it was filled with: stale, but the same in both chains."""
    r = ff.refused_layout(name, 8, mode)
    case = EngineCase(mode=mode, pad=5 if name == "padding_in_ranges" else 0, ranges=r["ranges"], outside=r["outside"],
                      separate_grad=r["separate_grad"])
    assert case.offs == r["offs"] and case.size == r["size"]
    before, got = case.check(K, why, "refused: %s, mode %d" % (name, mode))
    sel = case.in_ranges()
    # every float of the ranges was stepped, the padding and the vacated floats included (a plan that trained whole tensors only
    # would leave them behind)
    assert not np.any(got[-1]["flat"][sel] == before["flat"][sel])
    if name == "gradient_elsewhere":
        o, c = case.offs["trans"]
        assert np.array_equal(got[-1]["grad"][o:o + c], before["grad"][o:o + c]) and np.count_nonzero(got[-1]["grad_trans"]) == c
        assert not np.array_equal(got[-1]["grad_trans"], before["grad_trans"])


# ---- d. masks, limits, halos, shards ------------------------------------------------------------------------------------
def _masks():
    gm = np.array([1.0, 0.0, 0.5], np.float32)
    rm = np.ones((34, 3), np.float32)
    rm[::3] = 0.0                        # whole joints switched off
    rm[1::3, 1] = 0.25                   # fractions
    rm[5, 2] = 0.0
    return gm, rm


@pytest.mark.parametrize("K", (2, 3, 4))
@pytest.mark.parametrize("mode", (1, 2))
def test_masked_pose(mode, K):
    """global_mask / rotation_mask with zeros, ones and fractions: the pending step multiplies the adjoint by the mask and the
    pose block the stepped value.  A masked-out component has no gradient: it keeps its bits and its moments stay zero."""
    gm, rm = _masks()
    case = EngineCase(mode=mode, masks=(gm, rm))
    before, got = case.check(K, "folded", "masked pose, mode %d" % mode)
    for k, mask in (("global_rotation", gm), ("joint_rotations", rm.reshape(-1))):
        o, c = case.offs[k]
        off = np.tile(mask == 0.0, 8)
        assert off.any() and not off.all()
        for st in got:
            assert np.array_equal(st["flat"][o:o + c][off].view(np.uint32), before["flat"][o:o + c][off].view(np.uint32)), k
            assert not np.any(st["exp_avg"][o:o + c][off]) and not np.any(st["exp_avg_sq"][o:o + c][off]) and not np.any(st["grad"][o:o + c][off])
            assert np.all(st["exp_avg"][o:o + c][~off] != 0.0) and np.all(st["flat"][o:o + c][~off] != before["flat"][o:o + c][~off]), k


@pytest.mark.parametrize("K", (2, 3, 4))
def test_joint_limits_in_a_folded_run(K):
    from smalify_amd import model_io
    case = EngineCase(limits=True, stage=1)
    cur, _ = _problem(8, case.seed)
    lo, hi = model_io.joint_limit_table()
    jr = cur["joint_rotations"]
    assert np.count_nonzero((jr > hi) | (jr < lo)) > 50          # the pose violates the table
    _, got = case.check(K, "folded", "joint limits")
    assert got[-1]["losses"][8] > 0.0
    # (the same fit without the table has no such term: the switch is what this case adds)
    _, plain = EngineCase(stage=1).check(K, "folded", "no joint limits")
    assert plain[-1]["losses"][8] == 0.0 and not np.array_equal(plain[-1]["flat"], got[-1]["flat"])


# (frames, frame_offset, total_frames): windows of 4 frames; the second shard starts no window of its sequence
SHARDS = ((8, 3, 16), (2, 5, 16), (5, 4, 9))


@pytest.mark.parametrize("K", (2, 3, 4))
@pytest.mark.parametrize("M,offset,total", SHARDS)
@pytest.mark.parametrize("mode", (1, 2))
def test_halos_and_shards(mode, M, offset, total, K):
    """temporal halos on both sides and a shard in the middle of its sequence: the per-window normalisers follow the sequence's
    windows and the shape prior counts the windows that start among the shard's frames -- none at all for frames [5, 7)"""
    nwin = ff.prior_windows(4, offset, M)
    assert nwin == {(8, 3, 16): 2, (2, 5, 16): 0, (5, 4, 9): 2}[(M, offset, total)]
    case = EngineCase(M=M, mode=mode, halos=True, frame_offset=offset, total_frames=total)
    assert case.weights[2] > 0
    _, got = case.check(K, "folded", "shard [%d, %d) of %d, mode %d" % (offset, offset + M, total, mode))
    assert (got[-1]["losses"][3] > 0.0) == (nwin > 0)
    _, whole_seq = EngineCase(M=M, mode=mode).check(K, "folded", "no halos, whole sequence")
    assert not np.array_equal(whole_seq[-1]["flat"], got[-1]["flat"])


# ---- e. frame counts --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", ff.FRAME_KS)
@pytest.mark.parametrize("mode", (1, 2))
@pytest.mark.parametrize("M", ff.FRAMES)
def test_frame_counts(M, mode, K):
    """the step kernel's sums over frames at one frame, with slices that hold no frame (M < 12, M < 32) and with a second batch
    (M > 96, M > 128), and each skinning form as the first reader of the stepped translations"""
    case = EngineCase(M=M, mode=mode, window=4)
    case.check(K, "folded", "%d frames (%s), mode %d" % (M, "/".join(str(x) for x in ff.step_kernel_forms(M)), mode))


# ---- f. graph replay switched on, default stream ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", (2, 3, 7))
def test_graph_switch_on_the_default_stream_runs_the_folded_loop(K):
    assert torch.cuda.current_stream().cuda_stream == 0
    assert ff.path(K, True, False, True, True) == "folded"
    case = EngineCase(graph=True)
    _, got = case.check(K, "folded", "graph switch on, default stream")
    _, ref = EngineCase().run(K, whole=False)
    for a, b in zip(ref, got):
        _assert_same(a, b, "graph switch on against off, K=%d" % K)


# ---- g. what runs next on the same engine -------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (2, 3, 4))
@pytest.mark.parametrize("shared_scales", [True, False], ids=["shared_scales", "per_frame_scales"])
def test_evaluate_after_a_folded_run(shared_scales, K):
    """the last pending step of a call ends in a staging slot (K = 2) or in the caller's buffers, and the prior's gradient was
    last written to slot 1 (even K) or 0: an evaluation behind the call must see none of that"""
    e, new_fitter = _fitter_case(shared_scales, True, seed=55)
    W = _weights()
    out = []
    for whole in (False, True):
        f = new_fitter()
        _run_calls(f, K, whole, calls=((2, True),))
        f.evaluate(W[2][:6], float(W[2][6]), 2)
        out.append(_state(f))
        f.evaluate(W[0][:6], float(W[0][6]), 0)            # stage 0: no shape prior, other gradients
        out.append(_state(f))
    assert e.status() == 0
    _assert_same(out[0], out[2], "evaluate() after K=%d" % K)
    _assert_same(out[1], out[3], "stage-0 evaluate() after K=%d" % K)
    assert ff.prior_slot(K - 1) == (K - 1) & 1


@pytest.mark.parametrize("K", (2, 3, 4))
@pytest.mark.parametrize("mode", (1, 2))
def test_shorter_fit_after_a_longer_one_on_the_same_engine(mode, K):
    """16 frames folded, then 8 frames folded on the same engine: the staging slots, the prior's slots and the partials of
    frames 8 .. 15 the first run left must not reach the second"""
    fresh = _engine(16, 26 if mode == 1 else 20, "fresh-%d" % K)
    used = _engine(16, 26 if mode == 1 else 20, "used-%d" % K)
    long_case = EngineCase(M=16, mode=mode, seed=57)
    long_case.e = used
    long_case.run(K + 1, whole=True, calls=1)
    short_used, short_fresh = EngineCase(mode=mode), EngineCase(mode=mode)
    short_used.e, short_fresh.e = used, fresh
    _, a = short_fresh.run(K, whole=True)
    _, b = short_used.run(K, whole=True)
    assert short_used.plan()[0]
    for x, y in zip(a, b):
        _assert_same(x, y, "8 frames after 16, K=%d" % K)
