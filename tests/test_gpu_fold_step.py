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
