"""Which argument blocks the host refuses, and in which order (smalify_amd/csrc/smalfit_plan.h: fit_args_refusal, called
through tests/host_plan_shim.cpp): every refusal of smalfit_fit_eval from a ctypes block with dummy pointers, no GPU needed.
The GPU tests match the same texts behind the entry point's name."""
import ctypes as C

import pytest

from smalify_amd import _lib
from tests import host_plan
from tests.host_plan import valid_fit_args

MAX_FRAMES = 8
INDEP = dict(subject_frames=1, window=1, temporal=0, logscale_mode=2)        # a batch of independent images that is accepted

# (fields bent on the accepted block, engine facts bent, the refusal), in the order the host checks them
REFUSALS = (
    (dict(struct_size=C.sizeof(_lib.FitArgs) - 8), {}, "smalfit_fit_args.struct_size does not match this library (built against another smalfit.h?)"),
    (dict(num_frames=0), {}, "num_frames exceeds the engine's max_frames"),
    (dict(num_frames=MAX_FRAMES + 1), {}, "num_frames exceeds the engine's max_frames"),
    (dict(window=0), {}, "window must be positive"),
    (dict(frame_offset=-1), {}, "frame_offset must be >= 0"),
    (dict(frame_offset=2, total_frames=5), {}, "total_frames is smaller than frame_offset + num_frames"),
    (dict(betas=None), {}, "missing parameter / losses pointer"),
    (dict(global_rotation=None), {}, "missing parameter / losses pointer"),
    (dict(joint_rotations=None), {}, "missing parameter / losses pointer"),
    (dict(trans=None), {}, "missing parameter / losses pointer"),
    (dict(losses=None), {}, "missing parameter / losses pointer"),
    (dict(target_joints=None), {}, "keypoint targets missing"),
    (dict(target_visibility=None), {}, "keypoint targets missing"),
    (dict(target_sil=None), {}, "target_sil missing with w_sil > 0"),
    ({}, dict(has_pose_prior=False), "pose prior not set"),
    ({}, dict(shape_dim=0), "shape prior not set"),
    (dict(log_beta_scales=None), {}, "log_beta_scales missing"),
    (dict(subject_frames=2), {}, "subject_frames must be 0 (one subject) or 1 (independent images); clips of K > 1 frames per subject in one batch are not implemented"),
    (dict(subject_frames=-1), {}, "subject_frames must be 0 (one subject) or 1 (independent images); clips of K > 1 frames per subject in one batch are not implemented"),
    (dict(INDEP, window=2), {}, "subject_frames = 1 needs window = 1 (an image is its own window)"),
    (dict(INDEP, temporal=1), {}, "subject_frames = 1 needs temporal = 0 (unrelated images have no neighbours)"),
    (dict(INDEP, logscale_mode=1), {}, "subject_frames = 1 takes logscale_mode 0 or 2 (nothing is shared between images)"),
    (dict(INDEP, halo_prev=0x9000), {}, "subject_frames = 1 needs halo_prev = halo_next = NULL"),
    (dict(INDEP, halo_next=0x9000), {}, "subject_frames = 1 needs halo_prev = halo_next = NULL"),
    (dict(INDEP, frame_offset=1), {}, "subject_frames = 1 needs frame_offset = total_frames = 0"),
    (dict(INDEP, total_frames=4), {}, "subject_frames = 1 needs frame_offset = total_frames = 0"),
    (dict(INDEP, logscale_mode=0), {}, "a 26-dim shape prior of independent images needs per-frame log_beta_scales (logscale_mode 2)"),
    (dict(logscale_mode=2), {}, "a 26-dim shape prior needs shared log_beta_scales"),
    (dict(logscale_mode=0), {}, "a 26-dim shape prior needs shared log_beta_scales"),
)
ORDER = list(dict.fromkeys(msg for _, _, msg in REFUSALS))


@pytest.fixture(scope="module")
def plan():
    return host_plan.load()


def _refusal(plan, fields, facts=None):
    f = dict(max_frames=MAX_FRAMES, has_pose_prior=True, shape_dim=26)
    f.update(facts or {})
    return plan.fit_args_refusal(valid_fit_args(**fields), f["max_frames"], f["has_pose_prior"], f["shape_dim"])


def test_accepted_blocks(plan):
    assert plan.SIZEOF_FIT_ARGS == C.sizeof(_lib.FitArgs)
    assert _refusal(plan, {}) is None and _refusal(plan, INDEP) is None
    assert _refusal(plan, dict(num_frames=MAX_FRAMES)) is None and _refusal(plan, dict(num_frames=1)) is None
    assert _refusal(plan, dict(frame_offset=2, total_frames=6)) is None and _refusal(plan, dict(frame_offset=2)) is None
    # a term that is off needs nothing
    assert _refusal(plan, dict(w_j2d=0.0, target_joints=None, target_visibility=None)) is None
    assert _refusal(plan, dict(w_sil=0.0, target_sil=None)) is None
    assert _refusal(plan, dict(target_sil=None, target_sil_u8=0x9000)) is None
    assert _refusal(plan, dict(w_pose=0.0), dict(has_pose_prior=False)) is None
    assert _refusal(plan, dict(w_betas=0.0, logscale_mode=2), dict(shape_dim=0)) is None
    assert _refusal(plan, dict(logscale_mode=0, log_beta_scales=None), dict(shape_dim=20)) is None
    # the prior's dimension: the block's own wins over the engine's
    assert _refusal(plan, dict(logscale_mode=2, shape_prior_dim=20)) is None
    assert _refusal(plan, dict(logscale_mode=2), dict(shape_dim=20)) is None
    assert _refusal(plan, dict(logscale_mode=2, shape_prior_dim=21), dict(shape_dim=20)) == "a 26-dim shape prior needs shared log_beta_scales"
    assert _refusal(plan, dict(INDEP, logscale_mode=0, log_beta_scales=None), dict(shape_dim=20)) is None


@pytest.mark.parametrize("i", range(len(REFUSALS)))
def test_every_refusal(plan, i):
    fields, facts, msg = REFUSALS[i]
    assert _refusal(plan, fields, facts) == msg


def test_the_first_fault_is_reported(plan):
    """two faults in one block: the one the host checks first"""
    one = {}
    for fields, facts, msg in REFUSALS:
        one.setdefault(msg, (fields, facts))
    for i, first in enumerate(ORDER):
        for second in ORDER[i + 1:]:
            (f1, e1), (f2, e2) = one[first], one[second]
            if set(f1) & set(f2) or set(e1) & set(e2) or ("subject_frames" in f1) != ("subject_frames" in f2):
                continue                                   # the two need different values of one field
            got = _refusal(plan, dict(f2, **f1), dict(e2, **e1))
            assert got == first, (first, second, got)


def test_struct_size_alone(plan):
    """the rule smalfit_fit_run and the shard entry points ask on its own, before they read subject_frames at the block's tail"""
    a = valid_fit_args()
    assert plan.fit_args_size_refusal(a) is None
    for size in (0, C.sizeof(_lib.FitArgs) - 16, C.sizeof(_lib.FitArgs) + 8):
        a.struct_size = size
        assert plan.fit_args_size_refusal(a) == REFUSALS[0][2] == plan.fit_args_refusal(a, MAX_FRAMES, True, 26)


def test_sequence_frames_and_parents(plan):
    assert plan.sequence_frames(valid_fit_args()) == 4 and plan.sequence_frames(valid_fit_args(frame_offset=3)) == 7
    assert plan.sequence_frames(valid_fit_args(frame_offset=3, total_frames=16)) == 16
    ok = [-1] + [max(i - 3, 0) for i in range(1, 35)]
    assert plan.parents_ordered(ok) and plan.parents_ordered([7] + ok[1:])        # (the root's entry is not read)
    for i, bad in ((1, 1), (5, 5), (34, 40), (12, -1)):
        assert not plan.parents_ordered(ok[:i] + [bad] + ok[i + 1:])


def test_model_refusals(plan):
    """smalfit_model_create refuses what chain_bwd_kernel cannot reduce (more than 64 shape directions: one lane of one wave
    each), the fitter a model with fewer than the 20 directions it optimises; the texts name the limits"""
    assert plan.model_dims_refusal(3889, 7774, 41) is None and plan.model_dims_refusal(3056, 1, 1) is None
    assert plan.model_dims_refusal(3889, 7774, 64) is None
    for dims in ((0, 7774, 41), (3889, 0, 41), (3889, 7774, 0), (-1, 7774, 41)):
        assert plan.model_dims_refusal(*dims) == "bad dimensions"
    for nb in (65, 66, 128, 300):
        assert plan.model_dims_refusal(3889, 7774, nb) == "num_betas above 64 is not supported (the rest-joint path of d/d betas reduces 64 shape directions)"
    assert plan.model_dims_refusal(0, 0, 65) == "bad dimensions"                       # the first fault is reported
    for nb in (20, 21, 41, 64):
        assert plan.fit_model_refusal(nb) is None
    for nb in (1, 12, 19):
        assert plan.fit_model_refusal(nb) == "the model has fewer than the 20 shape directions the fitter optimises"


# ------------------------------------------------------------------------------------------------
# plan_eval: what one evaluation launches, with which switches
# ------------------------------------------------------------------------------------------------
P = 0x9000                                            # a dummy pointer
# the plan of valid_fit_args() -- 4 frames, windows of 2, shared limb scales, every term on, no gradient wanted -- on an engine
# with both priors (26-dim shape prior) and no joint limits; written from fit_eval_impl as it was before plan_eval existed
DEFAULT_PLAN = dict(
    M=4, window=2, frame_offset=0, sequence_frames=4, independent=0, nb=20, betas_stride=0, ls_stride=0, limb_scales=1,
    shape_prior=1, prior_dim=26, prior_uses_ls=1, prior_windows=2, prior_weight=2.0, prior_per_frame=0, head_prior="shared", head="plain",
    sil_on=1, rasterise=1, sil_target="f32", frame_loss=0, queue_loss=1, raster_backward=1, loss_launch="in_resolve", joints_in_head=0,
    w_temp=0.0, w_limit=0.0, halos=1, verts_out=0, need_pose=0, need_beta=0, need_ls=0, bwd_betas_shared=1, j_stride=0,
    asm_betas_shared=1, asm_ls_shared=1, ngrp_beta=8, asm_shape_sets=1, rows=0, W=0, ls_rows=0, clear_qloss=0,
    assembly_leaves_betas=0, assembly_leaves_scales=0)
NO_SIL = dict(sil_on=0, sil_target="none", queue_loss=0, raster_backward=0)
NO_PRIOR = dict(shape_prior=0, prior_dim=0, prior_uses_ls=0, prior_windows=0, prior_weight=0.0, head_prior="none")
ALL_GRADS = dict(g_betas=P, g_log_beta_scales=P, g_global_rotation=P, g_joint_rotations=P, g_trans=P)
IMAGES = dict(INDEP, num_frames=3)
# the plan of three independent images with the 26-dim prior, as differences from DEFAULT_PLAN
IMAGES_PLAN = dict(M=3, window=1, sequence_frames=3, independent=1, betas_stride=20, ls_stride=6, prior_windows=3, prior_weight=1.0,
                   prior_per_frame=1, head_prior="per_frame", head="images", halos=0, bwd_betas_shared=0, j_stride=105,
                   asm_betas_shared=0, asm_ls_shared=0, ngrp_beta=1, asm_shape_sets=3)
# window rows over the default block (smalfit_fit_eval_windows): two windows; the shared gradients are left to window_rows_kernel.
# ngrp_beta stays 8 although the backward pass then writes one group of per-frame partials: kept as the host always had it
WINDOWS_PLAN = dict(W=2, need_beta=1, bwd_betas_shared=0, frame_loss=1, clear_qloss=1, assembly_leaves_betas=1, assembly_leaves_scales=1,
                    ngrp_beta=8)
WR = dict(window_rows=True, want_betas=True)

# name: (fields bent on valid_fit_args, engine facts / mode bent, the fields of the plan that differ from DEFAULT_PLAN)
EVAL_PLANS = {
    "default": ({}, {}, {}),
    "w_sil 0": (dict(w_sil=0.0), {}, dict(NO_SIL, rasterise=0, loss_launch="own_kernel", joints_in_head=1)),
    "w_sil 0, sil_out": (dict(w_sil=0.0, sil_out=P), {}, dict(NO_SIL, rasterise=1, loss_launch="in_resolve", joints_in_head=0)),
    "u8 target": (dict(target_sil=None, target_sil_u8=P), {}, dict(sil_target="u8")),
    "both targets: bytes win": (dict(target_sil_u8=P), {}, dict(sil_target="u8")),
    "w_betas 0": (dict(w_betas=0.0), {}, NO_PRIOR),
    "shape_prior_dim 20": (dict(shape_prior_dim=20), {}, dict(prior_dim=20, prior_uses_ls=0)),
    "engine's prior of 20": ({}, dict(shape_dim=20), dict(prior_dim=20, prior_uses_ls=0)),
    "logscale_mode 0": (dict(logscale_mode=0, shape_prior_dim=20, log_beta_scales=None, g_log_beta_scales=P), {},
                        dict(limb_scales=0, asm_ls_shared=0, prior_dim=20, prior_uses_ls=0, need_ls=0)),
    "logscale_mode 2": (dict(logscale_mode=2, shape_prior_dim=20, g_log_beta_scales=P), {},
                        dict(ls_stride=6, asm_ls_shared=0, prior_dim=20, prior_uses_ls=0, need_ls=1)),
    "shard": (dict(frame_offset=3, total_frames=16), {}, dict(frame_offset=3, sequence_frames=16, prior_windows=2, prior_weight=2.0)),
    "shard inside one window": (dict(num_frames=1, window=8, frame_offset=3, total_frames=16), {},
                                dict(M=1, window=8, frame_offset=3, sequence_frames=16, prior_windows=0, prior_weight=0.0)),
    "temporal": (dict(w_temp=0.5, halo_prev=P, halo_next=P), {}, dict(w_temp=0.5)),
    "temporal 0, halos given": (dict(temporal=0, w_temp=0.5, halo_prev=P, halo_next=P), {}, dict(w_temp=0.0, halos=0)),
    "joint limits on": (dict(w_limit=100.0), dict(has_joint_limits=True), dict(w_limit=100.0)),
    "joint limits off": (dict(w_limit=100.0), {}, dict(w_limit=0.0)),
    "every gradient": (ALL_GRADS, {}, dict(need_pose=1, need_beta=1, need_ls=1)),
    "g_joint_rotations alone missing": (dict(ALL_GRADS, g_joint_rotations=None), {}, dict(need_pose=0, need_beta=1, need_ls=1)),
    "verts_out": (dict(verts_out=P), {}, dict(verts_out=1)),
    "pending step": (ALL_GRADS, dict(pending=True), dict(head="step", need_pose=1, need_beta=1, need_ls=1)),
    "losses_per_frame": (dict(losses_per_frame=P), {}, dict(rows=1, frame_loss=1)),
    "assemble off, losses_per_frame": (dict(losses_per_frame=P), dict(assemble=False), dict(rows=0, frame_loss=0)),
    "images": (IMAGES, {}, IMAGES_PLAN),
    "images, prior off": (dict(IMAGES, w_betas=0.0), {}, dict(IMAGES_PLAN, **dict(NO_PRIOR, prior_per_frame=0, head="plain"))),
    "images, rows": (dict(IMAGES, losses_per_frame=P), {}, dict(IMAGES_PLAN, rows=1, frame_loss=1)),
    "images, every gradient": (dict(IMAGES, **ALL_GRADS), {}, dict(IMAGES_PLAN, need_pose=1, need_beta=1, need_ls=1)),
    "windows: g_betas": ({}, WR, WINDOWS_PLAN),
    "windows: both gradients": ({}, dict(WR, want_scales=True), dict(WINDOWS_PLAN, need_ls=1, ls_rows=1)),
    "windows: totals too": (dict(g_betas=P, g_log_beta_scales=P), dict(WR, want_scales=True), dict(WINDOWS_PLAN, need_ls=1, ls_rows=1)),
    "windows: losses only": ({}, dict(window_rows=True), dict(WINDOWS_PLAN, need_beta=0)),
    "windows, rows": (dict(losses_per_frame=P), WR, dict(WINDOWS_PLAN, rows=1, clear_qloss=0)),
    "windows, logscale_mode 2": (dict(logscale_mode=2, shape_prior_dim=20, g_log_beta_scales=P), WR,
                                 dict(WINDOWS_PLAN, ls_stride=6, asm_ls_shared=0, prior_dim=20, prior_uses_ls=0, need_ls=1, ls_rows=0,
                                      assembly_leaves_scales=0)),
    "windows, w_sil 0": (dict(w_sil=0.0), WR, dict(WINDOWS_PLAN, **dict(NO_SIL, rasterise=0, loss_launch="own_kernel", joints_in_head=1,
                                                                         frame_loss=0))),
    "windows of a shard": (dict(frame_offset=3, total_frames=16), WR, dict(WINDOWS_PLAN, frame_offset=3, sequence_frames=16, W=3)),
}
FACTS = ("max_frames", "has_pose_prior", "shape_dim", "has_joint_limits")


def _plan_of(plan, fields, bent):
    args = valid_fit_args(**fields)
    facts = {k: v for k, v in bent.items() if k in FACTS}
    assert plan.fit_args_refusal(args, facts.get("max_frames", MAX_FRAMES), facts.get("has_pose_prior", True), facts.get("shape_dim", 26)) is None
    if bent.get("window_rows"):
        rows = _lib.WindowRows()
        rows.num_windows, rows.losses = plan.window_rows_count(args.window, args.frame_offset, args.num_frames), P
        rows.g_betas = P if bent.get("want_betas") else None
        rows.g_log_beta_scales = P if bent.get("want_scales") else None
        assert plan.refusal("window_rows", args, rows) is None
    return plan.plan_eval(args, **bent)


@pytest.mark.parametrize("name", list(EVAL_PLANS))
def test_eval_plan(plan, name):
    fields, bent, differs = EVAL_PLANS[name]
    want = dict(DEFAULT_PLAN, **differs)
    assert set(want) == set(host_plan.EVAL_INTS) | set(host_plan.EVAL_FLOATS)
    got = _plan_of(plan, fields, bent)
    assert got == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}


def test_eval_plan_crossings(plan):
    # per-frame rows x window rows x silhouette term -> who counts the queue kernels' loss per frame, who clears the counters
    #   (rows, windows, w_sil): (frame_loss, rows, clear_qloss, W)
    table = {(0, 0, 1.0): (0, 0, 0, 0), (1, 0, 1.0): (1, 1, 0, 0), (0, 1, 1.0): (1, 0, 1, 2), (1, 1, 1.0): (1, 1, 0, 2),
             (0, 0, 0.0): (0, 0, 0, 0), (1, 0, 0.0): (0, 1, 0, 0), (0, 1, 0.0): (0, 0, 1, 2), (1, 1, 0.0): (0, 1, 0, 2)}
    for (rows, windows, w_sil), want in table.items():
        got = _plan_of(plan, dict(w_sil=w_sil, losses_per_frame=P if rows else None), dict(WR) if windows else {})
        assert (got["frame_loss"], got["rows"], got["clear_qloss"], got["W"]) == want, (rows, windows, w_sil)
        assert got["queue_loss"] == got["raster_backward"] == got["sil_on"] == int(w_sil > 0)
    # independent images x the prior's dimension x the scale mode (26 dimensions need the per-frame scales: refused otherwise)
    #   (dim, mode): (prior_uses_ls, limb_scales, ls_stride, head, asm_ls_shared, asm_shape_sets)
    table = {(26, 2): (1, 1, 6, "images", 0, 3), (20, 2): (0, 1, 6, "images", 0, 3), (20, 0): (0, 0, 0, "images", 0, 3)}
    for (dim, mode), want in table.items():
        got = _plan_of(plan, dict(IMAGES, shape_prior_dim=dim, logscale_mode=mode), {})
        assert tuple(got[k] for k in ("prior_uses_ls", "limb_scales", "ls_stride", "head", "asm_ls_shared", "asm_shape_sets")) == want, (dim, mode)
        assert got["prior_dim"] == dim and got["prior_weight"] == 1.0 and got["prior_windows"] == 3
    # one subject x the same: the shared scales are the only mode 26 dimensions take
    table = {(26, 1): (1, 1, 0, 1), (20, 1): (0, 1, 0, 1), (20, 2): (0, 1, 6, 0), (20, 0): (0, 0, 0, 0)}
    for (dim, mode), want in table.items():
        got = _plan_of(plan, dict(shape_prior_dim=dim, logscale_mode=mode), {})
        assert tuple(got[k] for k in ("prior_uses_ls", "limb_scales", "ls_stride", "asm_ls_shared")) == want, (dim, mode)


# ------------------------------------------------------------------------------------------------
# grids of the fit path
# ------------------------------------------------------------------------------------------------
def test_grid_constants(plan):
    assert (plan.SWEEP_FACES, plan.BWD_FACES, plan.BWD_LANES, plan.RES_EDGE, plan.RECT_FACES) == (32, 4, 16, 32, 8)
    assert (plan.ASM_ELEM, plan.ASM_LOSS, plan.ASM_ROWS, plan.BAND_BLOCKS, plan.SELECT_BLOCKS, plan.SEL_WAVES, plan.SEL_GROUPS) == (4, 16, 4, 1536, 1792, 2, 16)
    assert (plan.PBM_SPLITS, plan.PBM_TILES, plan.FRAME_LOSS_STRIDE, plan.JOINT_BLOCKS, plan.SKIN_VERTS, plan.SKIN_THREADS) == (24, 4, 32, 41, 32, 512)
    assert plan.QUEUE_LOSS_BLOCKS == 3328


def test_grids_by_frames(plan):
    """M = 1, 8, 9: one frame, a full round of eight frames (one per XCD), the first overflow into a second round"""
    assert [plan.xcd_grid(1, M) for M in (1, 8, 9, 16, 17)] == [8, 8, 16, 16, 24]
    assert [plan.xcd_grid(31, M) for M in (1, 8, 9)] == [248, 248, 496]
    # box kernel: frame blocks | face blocks | joint riders | launch
    assert plan.box_grid(7774, 1, True) == (8, 248, 41, 297) and plan.box_grid(7774, 1, False) == (8, 248, 0, 256)
    assert plan.box_grid(7774, 8, True) == (8, 248, 328, 584) and plan.box_grid(7774, 9, True) == (16, 496, 369, 881)
    assert plan.box_grid(7774, 9, False) == (16, 496, 0, 512)
    assert [plan.sweep_grid(7774, M) for M in (1, 8, 9)] == [1944, 1944, 3888]
    assert [plan.raster_bwd_grid(7774, M) for M in (1, 8, 9)] == [15552, 15552, 31104]
    assert [plan.vertex_bwd_grid(4096, M) for M in (1, 8, 9)] == [128, 128, 256]
    assert [plan.vertex_bwd_grid(256, M) for M in (1, 8, 9)] == [8, 8, 16]
    # resolve: tiles per frame | loss riders | launch
    assert plan.resolve_grid(64, 1, 1) == (4, 8, 40) and plan.resolve_grid(64, 8, 8) == (4, 8, 40) and plan.resolve_grid(64, 9, 9) == (4, 16, 80)
    assert plan.resolve_grid(64, 9, 0) == (4, 0, 64)
    # mid kernel: pose-blend ids (chunks of four tiles of 16 frames) | dA ids | launch
    assert plan.mid_grid(1, True) == (240, 280, 520) and plan.mid_grid(8, True) == (240, 280, 520) and plan.mid_grid(9, True) == (240, 560, 800)
    assert plan.mid_grid(9, False) == (240, 560, 560)
    assert plan.mid_grid(64, True)[0] == 240 and plan.mid_grid(65, True)[0] == 480
    # chain: M frame blocks + the dbeta riders (48 column blocks at 4096 vertices, 3 at 256)
    assert [plan.chain_grid(M, True, 4096, True) for M in (1, 8, 9)] == [385, 392, 393]
    assert [plan.chain_grid(M, True, 4096, False) for M in (1, 8, 9)] == [49, 392, 441]
    assert [plan.chain_grid(M, False, 4096, True) for M in (1, 8, 9)] == [1, 8, 9]
    assert plan.chain_grid(4, True, 256, True) == 28 and plan.chain_grid(4, True, 256, False) == 16
    # assembly: shape sets | limb scales | 4 element blocks | 16 loss partials
    assert [plan.assemble_grid(True, M) for M in (1, 8, 9)] == [22, 22, 22]
    assert [plan.assemble_grid(False, M) for M in (1, 8, 9)] == [22, 29, 30]
    assert [plan.window_rows_grid(W) for W in (1, 2, 9)] == [1, 2, 9] and plan.frame_loss_rows_grid() == 4
    # skinning: (vertex blocks, frame tiles) of the form skin_form chose -- plain to 4 frames, wide from 49 at 4096 vertices
    assert plan.skin_grid(1, 4096) == (64, 1) and plan.skin_grid(4, 4096) == (64, 1)
    assert plan.skin_grid(8, 4096) == (128, 1) and plan.skin_grid(9, 4096) == (128, 1) and plan.skin_grid(17, 4096) == (128, 2)
    assert plan.skin_grid(48, 4096) == (128, 3) and plan.skin_grid(49, 4096) == (64, 4)


def test_grids_by_faces_vertices_and_image_size(plan):
    faces = (1, 255, 256, 257, 7774)
    assert [plan.box_grid(F, 1, False)[1] for F in faces] == [8, 8, 8, 16, 248]               # 256 faces per block
    assert [plan.sweep_grid(F, 1) for F in faces] == [8, 64, 64, 72, 1944]                    # 32
    assert [plan.raster_bwd_grid(F, 1) for F in faces] == [8, 512, 512, 520, 15552]           # 4
    assert [plan.rect_count(F) for F in faces] == [1, 32, 32, 33, 972]                        # 8 faces per union box
    # image sizes whose tile count is / is not a multiple of the resolve edge (32)
    assert [plan.resolve_grid(S, 1, 0)[0] for S in (1, 32, 33, 64, 100, 512, 1000, 1024)] == [1, 1, 4, 4, 16, 256, 1024, 1024]
    assert plan.resolve_grid(100, 9, 9) == (16, 16, 272)
    assert [plan.elem_blocks(n) for n in (0, 1, 256, 257, 3889 * 3, 2 ** 31 + 1)] == [0, 1, 1, 2, 46, 8388609]


# ------------------------------------------------------------------------------------------------
# the other entry points: every refusal, its order, the accepted edge next to the refused one
# ------------------------------------------------------------------------------------------------
def _lbs(**fields):
    a = _lib.LbsArgs()
    a.num_frames, a.num_betas, a.beta, a.theta, a.verts, a.joints = 2, 20, P, P, P, P
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def _adam(**fields):
    o = _lib.AdamArgs()
    o.param = o.grad = o.exp_avg = o.exp_avg_sq = P
    for k, v in fields.items():
        setattr(o, k, v)
    return o


def _shard(**fields):
    sh = _lib.ShardArgs()
    sh.world_size, sh.rank, sh.num_shared, sh.num_trainable_shared = 2, 1, 26, 20
    sh.shared_grad = sh.record = sh.gathered = sh.allgather = P
    for k, v in fields.items():
        setattr(sh, k, v)
    return sh


def _table(plan, name, good, table):
    """`good` is accepted; each row of `table` bends it and names the refusal; two faults at once: the first in the table's order"""
    assert plan.refusal(name, *good) is None
    for bent, msg in table:
        assert plan.refusal(name, *bent) == msg, (name, msg)


def test_null_count_step_refusals(plan):
    assert plan.refusal("null_argument", 1) is None and plan.refusal("null_argument", 0) == "null argument"
    _table(plan, "operator_args", (1, 1), (((0, 1), "bad argument"), ((-1, 1), "bad argument"), ((1, 0), "bad argument")))
    assert plan.refusal("step", 0) is None and plan.refusal("step", -1) == "step must be >= 0"
    assert plan.refusal("iterations", 1) is None and plan.refusal("iterations", 0) == "iterations must be positive"
    _table(plan, "adam_step", (1, 1, 1), (((0, 1, 1), "bad argument"), ((1, 0, 1), "bad argument"), ((1, 1, 0), "bad argument")))
    _table(plan, "profile_begin", (1, 1, 1), (((0, 1, 1), "bad argument"), ((1, 0, 1), "bad argument"), ((1, 1, 0), "bad argument")))


def test_engine_refusals(plan):
    big = "image_size above 1024 is not supported (float32 pixel walk, see kernels_raster.inc)"
    _table(plan, "engine_create", (1, 1, 1024), (((0, 1, 64), "bad argument"), ((1, 0, 64), "bad argument"), ((1, 1, 0), "bad argument"),
                                                 ((1, 1, 1025), big), ((0, 1, 1025), "bad argument"), ((1, 0, 4096), "bad argument")))
    assert plan.refusal("engine_create", 1, 1, 1) is None and plan.MAX_IMAGE_SIZE == 1024
    dims = "bad argument (dim must be 1..26)"
    _table(plan, "shape_prior", (1, 26), (((1, 27), dims), ((1, 0), dims), ((1, -1), dims), ((0, 20), dims)))
    assert plan.refusal("shape_prior", 1, 1) is None
    lo, hi = (C.c_float * 102)(*([-1.0] * 102)), (C.c_float * 102)(*([1.0] * 102))
    assert plan.refusal("joint_limits", lo, hi) is None and plan.refusal("joint_limits", lo, lo) is None       # min == max
    assert plan.refusal("joint_limits", None, hi) == "null argument" == plan.refusal("joint_limits", lo, None)
    assert plan.refusal("joint_limits", hi, lo) == "min must not exceed max"
    for i in (0, 57, 101):
        bad = (C.c_float * 102)(*([-1.0] * 102))
        bad[i] = 1.5
        assert plan.refusal("joint_limits", bad, hi) == "min must not exceed max"
        bad[i] = float("nan")
        assert plan.refusal("joint_limits", bad, hi) == "min must not exceed max"
        bad[i] = 1.0
        assert plan.refusal("joint_limits", bad, hi) is None
    edge = "SMALFIT_OPT_UNCLAMPED_EDGE_T takes 0 or 1"
    _table(plan, "option", (1, 1), (((1, 2), edge), ((1, -1), edge), ((0, 0), "unknown option"), ((2, 1), "unknown option")))
    assert plan.refusal("option", 1, 0) is None


def test_lbs_refusals(plan):
    frames, one = "num_frames exceeds the engine's max_frames", "give exactly one of theta (axis-angle) and Rs (rotation matrices)"
    table = ((dict(num_frames=0), frames), (dict(num_frames=MAX_FRAMES + 1), frames), (dict(num_betas=0), "num_betas out of range"),
             (dict(num_betas=42), "num_betas out of range"), (dict(beta=None), "beta missing"), (dict(Rs=P), one), (dict(theta=None), one))
    assert plan.refusal("lbs_args", _lbs(), MAX_FRAMES, 41) is None
    assert plan.refusal("lbs_args", _lbs(num_frames=MAX_FRAMES, num_betas=41), MAX_FRAMES, 41) is None
    assert plan.refusal("lbs_args", _lbs(theta=None, Rs=P), MAX_FRAMES, 41) is None
    for i, (bent, msg) in enumerate(table):
        assert plan.refusal("lbs_args", _lbs(**bent), MAX_FRAMES, 41) == msg
        for later, other in table[i + 1:]:                                                    # the first fault is reported
            if not set(later) & set(bent) and other != msg:
                assert plan.refusal("lbs_args", _lbs(**dict(later, **bent)), MAX_FRAMES, 41) == msg
    assert plan.refusal("lbs_outputs", _lbs()) is None
    assert plan.refusal("lbs_outputs", _lbs(verts=None)) == "verts / joints outputs missing" == plan.refusal("lbs_outputs", _lbs(joints=None))


def test_render_temporal_pose_prior_refusals(plan):
    m, n = "M exceeds the engine's max_frames", "N exceeds the engine's max_frames"
    _table(plan, "render_frames", (MAX_FRAMES, MAX_FRAMES), (((MAX_FRAMES + 1, MAX_FRAMES), m), ((0, MAX_FRAMES), m), ((-1, MAX_FRAMES), m)))
    _table(plan, "temporal_frames", (MAX_FRAMES, MAX_FRAMES), (((MAX_FRAMES + 1, MAX_FRAMES), n), ((0, MAX_FRAMES), n)))
    assert plan.refusal("render_frames", 1, MAX_FRAMES) is None and plan.refusal("temporal_frames", 1, MAX_FRAMES) is None
    _table(plan, "pose_prior", (1, 1, 1), (((0, 1, 1), "bad argument"), ((1, 0, 1), "bad argument"), ((1, 1, 0), "pose prior not set"),
                                           ((0, 1, 0), "bad argument"), ((1, 0, 0), "bad argument")))


def test_fit_run_and_shard_refusals(plan):
    graph = "subject_frames != 0 is not supported by the graph replay (smalfit_engine_set_graph)"
    shard = "subject_frames != 0 cannot be sharded (independent images need no collective: give each rank its own batch)"
    assert plan.refusal("graph_subject", 1, valid_fit_args()) is None and plan.refusal("graph_subject", 0, valid_fit_args(**INDEP)) is None
    assert plan.refusal("graph_subject", 1, valid_fit_args(**INDEP)) == graph
    assert plan.refusal("shard_subject", valid_fit_args()) is None and plan.refusal("shard_subject", valid_fit_args(**INDEP)) == shard
    # a block of another header: its tail is not read here, the evaluation refuses it
    assert plan.refusal("shard_subject", valid_fit_args(struct_size=C.sizeof(_lib.FitArgs) - 8, **INDEP)) is None
    _table(plan, "shard_record", (0, 1, 1), (((-1, 1, 1), "bad argument"), ((0, 0, 1), "bad argument"), ((0, 1, 0), "bad argument")))
    good = (2, 26, 1, 26, 26, _adam())
    state = "bad optimiser state"
    _table(plan, "shard_reduce", good, (((0, 26, 1, 26, 26, _adam()), "bad argument"), ((2, 25, 1, 26, 26, _adam()), "bad argument"),
                                        ((2, 26, 0, 26, 26, _adam()), "bad argument"), ((2, 26, 1, 0, 0, _adam()), "bad argument"),
                                        ((2, 26, 1, 26, -1, _adam()), "bad argument"), ((2, 26, 1, 26, 27, _adam()), "bad argument"),
                                        ((2, 26, 1, 26, 26, None), "bad argument"), ((2, 26, 1, 26, 26, _adam(param=None)), state),
                                        ((2, 26, 1, 26, 26, _adam(exp_avg_sq=None)), state), ((2, 26, 1, 26, 26, _adam(step=-1)), state),
                                        ((0, 26, 1, 26, 26, _adam(step=-1)), "bad argument")))
    assert plan.refusal("shard_reduce", 1, 26, 1, 26, 0, _adam()) is None
    # smalfit_shard_run, in the order it checks
    a, o = valid_fit_args(), _adam(step=3)
    table = ((dict(sh=_shard(struct_size=8)), "smalfit_shard_args.struct_size does not match this library (built against another smalfit.h?)"),
             (dict(iterations=0), "iterations must be positive"),
             (dict(sh=_shard(world_size=0)), "bad rank / world_size"), (dict(sh=_shard(rank=-1)), "bad rank / world_size"),
             (dict(sh=_shard(rank=2)), "bad rank / world_size"),
             (dict(sh=_shard(num_shared=0)), "bad num_shared / num_trainable_shared"), (dict(sh=_shard(num_trainable_shared=27)), "bad num_shared / num_trainable_shared"),
             (dict(sh=_shard(num_trainable_shared=-1)), "bad num_shared / num_trainable_shared"),
             (dict(sh=_shard(shared_grad=None)), "missing buffer / collective"), (dict(sh=_shard(allgather=None)), "missing buffer / collective"),
             (dict(ol=_adam(step=-1), os=_adam(step=-1)), "adam_local and adam_shared must carry the same step >= 0"),
             (dict(os=_adam(step=4)), "adam_local and adam_shared must carry the same step >= 0"),
             (dict(a=valid_fit_args(**INDEP)), shard))

    def run(**bent):
        k = dict(dict(a=a, ol=o, os=_adam(step=3), sh=_shard(), iterations=1), **bent)
        return plan.refusal("shard_run", k["a"], k["ol"], k["os"], k["sh"], k["iterations"])
    assert run() is None and run(sh=_shard(rank=0, world_size=1, num_trainable_shared=26)) is None and run(sh=_shard(num_trainable_shared=0)) is None
    for i, (bent, msg) in enumerate(table):
        assert run(**bent) == msg, msg
        for later, _ in table[i + 1:]:
            if not set(later) & set(bent):
                assert run(**dict(later, **bent)) == msg, (msg, list(later))


def test_window_rows_refusals(plan):
    def rows(**fields):
        r = _lib.WindowRows()
        r.num_windows, r.losses, r.g_betas, r.g_log_beta_scales = 2, P, P, P
        for k, v in fields.items():
            setattr(r, k, v)
        return r
    count = "smalfit_window_rows.num_windows is not the number of windows these frames belong to"
    assert plan.refusal("window_rows", valid_fit_args(), rows()) is None
    assert plan.refusal("window_rows", valid_fit_args(frame_offset=3), rows(num_windows=3)) is None
    assert plan.refusal("window_rows", valid_fit_args(), rows(struct_size=8)) == "smalfit_window_rows.struct_size does not match this library (built against another smalfit.h?)"
    assert plan.refusal("window_rows", valid_fit_args(), rows(losses=None)) == "smalfit_window_rows.losses missing"
    assert plan.refusal("window_rows", valid_fit_args(**INDEP), rows(num_windows=4)) == "window rows need subject_frames = 0 (independent images already have one row per image)"
    assert plan.refusal("window_rows", valid_fit_args(), rows(num_windows=3)) == count == plan.refusal("window_rows", valid_fit_args(frame_offset=3), rows())
    assert plan.refusal("window_rows", valid_fit_args(logscale_mode=2), rows()) == "smalfit_window_rows.g_log_beta_scales needs shared log_beta_scales (logscale_mode 1)"
    assert plan.refusal("window_rows", valid_fit_args(logscale_mode=2), rows(g_log_beta_scales=None)) is None
    assert [plan.window_rows_count(2, off, 4) for off in (0, 1, 2, 3)] == [2, 3, 2, 3] and plan.window_rows_count(8, 3, 1) == 1


# ------------------------------------------------------------------------------------------------
# the mesh objective's entry points and smalfit_fit3d_step
# ------------------------------------------------------------------------------------------------
def test_mesh_entry_refusals(plan):
    positive = "max_meshes and max_points must be positive"
    _table(plan, "mesh_objective_create", (1, 1, 1), (((0, 1, 1), "null argument"), ((1, 0, 1), positive), ((1, 1, 0), positive),
                                                      ((1, -1, 8), positive), ((0, 0, 0), "null argument")))
    assert plan.refusal("null_handle", 1) is None and plan.refusal("null_handle", 0) == "null handle"
    meshes, points = "num_meshes out of range", "the chamfer term needs 1 <= num_points <= max_points target points"
    # (num_meshes, max_meshes, w_chamfer, points given, num_points, max_points)
    _table(plan, "mesh_eval", (2, 2, 1.0, 1, 8, 8), (((0, 2, 1.0, 1, 8, 8), meshes), ((3, 2, 1.0, 1, 8, 8), meshes), ((-1, 2, 0.0, 0, 0, 8), meshes),
                                                     ((2, 2, 1.0, 0, 8, 8), points), ((2, 2, 1.0, 1, 0, 8), points), ((2, 2, 1.0, 1, 9, 8), points),
                                                     ((2, 2, 0.5, 1, -1, 8), points), ((3, 2, 1.0, 0, 0, 8), meshes)))
    for w in (0.0, -1.0):                                       # chamfer off: the points are not looked at
        assert plan.refusal("mesh_eval", 1, 2, w, 0, 0, 8) is None and plan.refusal("mesh_eval", 1, 2, w, 1, 9, 8) is None
    assert plan.refusal("mesh_eval", 1, 2, 1.0, 1, 1, 8) is None

    def counts(*values):
        return (C.c_int * len(values))(*values) if values else None      # (the array itself: it must outlive the call)
    good = (1, 2, counts(4, 3), counts(4, 1))
    _table(plan, "mesh_targets_create", good, (((0, 2, counts(4, 3), counts(4, 1)), "null argument"), ((1, 0, counts(4), counts(4)), "no meshes"),
                                               ((1, -1, counts(4), counts(4)), "no meshes"), ((1, 2, counts(4, 0), counts(4, 1)), "empty target mesh"),
                                               ((1, 2, counts(4, 3), counts(0, 1)), "empty target mesh"), ((1, 2, counts(-1, 3), counts(4, 1)), "empty target mesh"),
                                               ((0, 0, None, None), "null argument"), ((1, 0, counts(0), counts(0)), "no meshes")))
    _table(plan, "mesh_sample", (1, 1), (((0, 1), "null argument"), ((1, 0), "num_points must be positive"), ((1, -5), "num_points must be positive"),
                                         ((0, 0), "null argument")))


FIT3D_TRAINED = "%s is trained (lr > 0) but its parameter or Adam state is missing"
# (fields bent on the accepted block, facts bent, the refusal), in the order the host checks them
FIT3D_REFUSALS = (
    (dict(num_meshes=0), {}, "num_meshes exceeds the engine's max_frames or the objective's max_meshes"),
    (dict(num_meshes=3), dict(max_frames=2), "num_meshes exceeds the engine's max_frames or the objective's max_meshes"),
    (dict(num_meshes=3), dict(max_meshes=2, target_meshes=3), "num_meshes exceeds the engine's max_frames or the objective's max_meshes"),
    ({}, dict(objective_verts=4), "engine and objective were built for different meshes"),
    (dict(num_betas=0), {}, "num_betas out of range"),
    (dict(num_betas=42), {}, "num_betas out of range"),
    (dict(num_betas=65), dict(model_betas=80), "num_betas out of range"),
    (dict(betas=None), {}, "missing parameter / losses pointer"),
    (dict(global_rot=None), {}, "missing parameter / losses pointer"),
    (dict(joint_rot=None), {}, "missing parameter / losses pointer"),
    (dict(trans=None), {}, "missing parameter / losses pointer"),
    (dict(losses=None), {}, "missing parameter / losses pointer"),
    (dict(num_points=0), {}, "the chamfer term needs 1 <= num_points <= max_points"),
    (dict(num_points=65), {}, "the chamfer term needs 1 <= num_points <= max_points"),
    ({}, dict(targets=False), "neither target points nor target meshes given"),
    ({}, dict(target_meshes=3), "number of target meshes differs from num_meshes"),
    (dict(m_betas=None), {}, "betas is trained (lr > 0) but its parameter or Adam state is missing"),
    (dict(v_betas=None), {}, "betas is trained (lr > 0) but its parameter or Adam state is missing"),
    (dict(m_global_rot=None), {}, "global_rot is trained (lr > 0) but its parameter or Adam state is missing"),
    (dict(v_global_rot=None), {}, "global_rot is trained (lr > 0) but its parameter or Adam state is missing"),
    (dict(m_joint_rot=None), {}, "joint_rot is trained (lr > 0) but its parameter or Adam state is missing"),
    (dict(v_joint_rot=None), {}, "joint_rot is trained (lr > 0) but its parameter or Adam state is missing"),
    (dict(m_trans=None), {}, "trans is trained (lr > 0) but its parameter or Adam state is missing"),
    (dict(v_trans=None), {}, "trans is trained (lr > 0) but its parameter or Adam state is missing"),
    (dict(deform_verts=None), {}, "deform_verts is trained (lr > 0) but its parameter or Adam state is missing"),
    (dict(m_deform_verts=None), {}, "deform_verts is trained (lr > 0) but its parameter or Adam state is missing"),
    (dict(v_deform_verts=None), {}, "deform_verts is trained (lr > 0) but its parameter or Adam state is missing"),
    (dict(adam_t=0), {}, "adam_t must be the 1-based step count"),
    (dict(adam_t=-1), {}, "adam_t must be the 1-based step count"),
)


def test_fit3d_refusals_whole_and_in_order(plan):
    assert plan.fit3d_args_refusal(host_plan.valid_fit3d_args()) is None
    for name in host_plan.FIT3D_TENSORS:
        assert FIT3D_TRAINED % name in [msg for _, _, msg in FIT3D_REFUSALS]
    order = list(dict.fromkeys(msg for _, _, msg in FIT3D_REFUSALS))
    for i, (fields, facts, msg) in enumerate(FIT3D_REFUSALS):
        assert plan.fit3d_args_refusal(host_plan.valid_fit3d_args(**fields), **facts) == msg, (fields, facts)
        # two faults at once: the one that comes first in the host's order
        for later, later_facts, other in FIT3D_REFUSALS[i + 1:]:
            if order.index(other) > order.index(msg) and not set(later) & set(fields) and not set(later_facts) & set(facts):
                got = plan.fit3d_args_refusal(host_plan.valid_fit3d_args(**dict(later, **fields)), **dict(later_facts, **facts))
                assert got == msg, (fields, facts, later, later_facts)


def test_fit3d_accepts_what_the_rules_leave_open(plan):
    ok = lambda facts=None, **fields: plan.fit3d_args_refusal(host_plan.valid_fit3d_args(**fields), **(facts or {})) is None  # noqa: E731
    assert ok(dict(max_frames=2, max_meshes=2), num_meshes=2) and ok(num_points=64) and ok(num_points=1)
    assert ok(num_betas=41) and ok(dict(model_betas=80), num_betas=64) and ok(num_betas=1)
    # chamfer off: neither the points nor the targets are looked at
    off = (C.c_float * 4)(0.0, 1.0, 0.01, 0.1)
    assert ok(dict(targets=False), weights=off, num_points=0) and ok(dict(target_meshes=7), weights=off, num_points=1000)
    # the caller's points: no targets needed, and their number is not compared
    assert ok(dict(targets=False), points=0x777000) and ok(dict(target_meshes=3), points=0x777000)
    # a frozen tensor needs no state, deform_verts not even the parameter; nothing trained: no step count
    for name in host_plan.FIT3D_TENSORS:
        assert ok(**{"lr_" + name: 0.0, "m_" + name: None, "v_" + name: None})
        assert ok(**{"lr_" + name: -1.0, "m_" + name: None})
    assert ok(lr_deform_verts=0.0, deform_verts=None)
    assert ok(adam_t=0, **{"lr_" + name: 0.0 for name in host_plan.FIT3D_TENSORS})
    assert not ok(adam_t=0, lr_betas=0.0)


V_STANDIN = 3889
# fitter_3d's schemes (SMALParamGroup.param_map without log_beta_scales, which no scheme trains through the step) and the step
# that trains nothing
SCHEMES = {"init": ("global_rot", "trans"), "default": ("betas", "global_rot", "joint_rot", "trans"), "shape": ("betas", "global_rot", "trans"),
           "pose": ("global_rot", "joint_rot", "trans"), "deform": ("deform_verts",), "none": ()}


def _seg(tensor, count, row_len, g_stride, g_offset, block0):
    return dict(tensor=tensor, count=count, row_len=row_len, g_stride=g_stride, g_offset=g_offset, block0=block0)


# 3 meshes, 20 betas, the stand-in's 3889 vertices: (need_pose, need_beta, segments, blocks of the Adam launch)
PLANS_N3 = {
    "init": (True, False, [_seg("global_rot", 9, 3, 105, 0, 0), _seg("trans", 9, 3, 3, 0, 1)], 2),
    "default": (True, True, [_seg("betas", 60, 20, 20, 0, 0), _seg("global_rot", 9, 3, 105, 0, 1), _seg("joint_rot", 306, 102, 105, 3, 2),
                             _seg("trans", 9, 3, 3, 0, 4)], 5),
    "shape": (True, True, [_seg("betas", 60, 20, 20, 0, 0), _seg("global_rot", 9, 3, 105, 0, 1), _seg("trans", 9, 3, 3, 0, 2)], 3),
    "pose": (True, False, [_seg("global_rot", 9, 3, 105, 0, 0), _seg("joint_rot", 306, 102, 105, 3, 1), _seg("trans", 9, 3, 3, 0, 3)], 4),
    "deform": (False, False, [_seg("deform_verts", 35001, 11667, 11667, 0, 0)], 137),
    "none": (False, False, [], 0),
}
# the other sizes: per tensor (count, row_len, g_stride, g_offset, blocks)
GEOMETRY = {
    (1, 20): dict(betas=(20, 20, 20, 0, 1), global_rot=(3, 3, 105, 0, 1), joint_rot=(102, 102, 105, 3, 1), trans=(3, 3, 3, 0, 1),
                  deform_verts=(11667, 11667, 11667, 0, 46)),
    (1, 41): dict(betas=(41, 41, 41, 0, 1), global_rot=(3, 3, 105, 0, 1), joint_rot=(102, 102, 105, 3, 1), trans=(3, 3, 3, 0, 1),
                  deform_verts=(11667, 11667, 11667, 0, 46)),
    (3, 20): dict(betas=(60, 20, 20, 0, 1), global_rot=(9, 3, 105, 0, 1), joint_rot=(306, 102, 105, 3, 2), trans=(9, 3, 3, 0, 1),
                  deform_verts=(35001, 11667, 11667, 0, 137)),
    (3, 41): dict(betas=(123, 41, 41, 0, 1), global_rot=(9, 3, 105, 0, 1), joint_rot=(306, 102, 105, 3, 2), trans=(9, 3, 3, 0, 1),
                  deform_verts=(35001, 11667, 11667, 0, 137)),
}
POINTS = (  # (chamfer on, the caller's points, points_out) -> Fit3dPlan::points
    ((True, None, None), "sample_to_objective"), ((True, None, 0x888000), "sample_to_caller"), ((True, 0x777000, None), "callers"),
    ((True, 0x777000, 0x888000), "callers_copied"), ((True, 0x777000, 0x777000), "callers"),
    ((False, None, None), "none"), ((False, 0x777000, 0x888000), "none"), ((False, None, 0x888000), "none"),
)


def _scheme_args(scheme, **fields):
    lrs = {"lr_" + t: (0.01 if t in SCHEMES[scheme] else 0.0) for t in host_plan.FIT3D_TENSORS}
    return host_plan.valid_fit3d_args(**dict(lrs, **fields))


@pytest.mark.parametrize("scheme", list(SCHEMES))
def test_plan_fit3d_of_every_scheme(plan, scheme):
    need_pose, need_beta, seg, blocks = PLANS_N3[scheme]
    for (chamfer, points, points_out), where in POINTS:
        w = (C.c_float * 4)(1.0 if chamfer else 0.0, 1.0, 0.01, 0.1)
        a = _scheme_args(scheme, num_meshes=3, weights=w, points=points, points_out=points_out)
        assert plan.fit3d_args_refusal(a, target_meshes=3) is None
        assert plan.plan_fit3d(a, V_STANDIN) == dict(chamfer=chamfer, points=where, need_pose=need_pose, need_beta=need_beta,
                                                     planar_vertex_grad=need_pose or need_beta, any_trained=bool(seg), seg=seg,
                                                     adam_blocks=blocks)


@pytest.mark.parametrize("N,nb", list(GEOMETRY))
@pytest.mark.parametrize("scheme", list(SCHEMES))
def test_plan_fit3d_adam_geometry(plan, scheme, N, nb):
    got = plan.plan_fit3d(_scheme_args(scheme, num_meshes=N, num_betas=nb), V_STANDIN)
    want, block0 = [], 0
    for t in host_plan.FIT3D_TENSORS:
        if t in SCHEMES[scheme]:
            count, row_len, g_stride, g_offset, blocks = GEOMETRY[(N, nb)][t]
            want.append(_seg(t, count, row_len, g_stride, g_offset, block0))
            block0 += blocks
    assert got["seg"] == want and got["adam_blocks"] == block0
    if (N, nb) == (3, 20):
        assert want == PLANS_N3[scheme][2]


def test_plan_fit3d_negative_and_nan_rates_train_nothing(plan):
    a = _scheme_args("none", lr_betas=-0.5, lr_trans=float("nan"))
    got = plan.plan_fit3d(a, V_STANDIN)
    assert not got["any_trained"] and got["seg"] == [] and got["adam_blocks"] == 0 and not got["need_beta"]


def test_fit3d_adam_argument_layout(plan):
    """the kernel argument moved to smalfit_plan.h whole: four pointers, six 4-byte fields per segment; five segments and five
    4-byte fields, padded to the pointers' alignment"""
    params, seg, args, block = plan.fit3d_constants()
    assert params == len(host_plan.FIT3D_TENSORS) == 5
    assert seg == 4 * 8 + 6 * 4 == 56 and args == 5 * 56 + 5 * 4 + 4 == 304
    assert block == C.sizeof(_lib.Fit3dArgs)


def test_mesh_launch_grids_on_both_sides_of_256(plan):
    # compose: N V 3 coordinates, one thread each
    assert [plan.mesh_compose_blocks(1, v) for v in (1, 85, 86, 170, 171)] == [1, 1, 2, 2, 3]      # 3, 255, 258, 510, 513
    assert plan.mesh_compose_blocks(2, 128) == 3 and plan.mesh_compose_blocks(256, 1) == 3 and plan.mesh_compose_blocks(3, V_STANDIN) == 137
    assert plan.mesh_compose_blocks(1024, 1 << 20) == 1024 * (1 << 20) * 3 // 256                  # past 2^31 coordinates
    # the sampler: S points x N meshes
    assert [plan.mesh_sample_grid(s, 3) for s in (1, 255, 256, 257, 512, 513, 3000)] == [(1, 3), (1, 3), (1, 3), (2, 3), (2, 3), (3, 3), (12, 3)]
    assert [plan.fit3d_adam_blocks(c) for c in (1, 255, 256, 257, 511, 512, 513)] == [1, 1, 1, 2, 2, 2, 3]
    assert [plan.frame_betas_grid(m) for m in (1, 3, 256, 257)] == [1, 3, 256, 257]


def test_plan_fit3d_riders_every_switch(plan):
    """what the opt-in blocks of a step share, over every combination of: each surface direction, min_cos_point / min_cos_vert of
    both gate blocks, the chamfer boundary rule, the chamfer term itself, a vert_normals output, the caller's points against
    sampled ones.  The rule beside it is written from the step's description: normals and boundary bytes are drawn with the
    points only in a step that samples them, when a compatibility test that reads them (each chamfer test reads both sets) or the
    boundary rule is on in a term that runs; the vertex normals go to the surface gate block's output when its own vertex test
    is on and asks for them; the surface term reuses them when the chamfer gates gathered them"""
    import itertools
    checked = 0
    for wp, wv, scp, scv, ccp, ccv, bound, wc, out, points in itertools.product(
            (0.0, 0.5), (0.0, 0.25), (False, True), (False, True), (False, True), (False, True), (False, True), (0.0, 1.0),
            (False, True), ("callers", "callers_copied", "sample_to_caller", "sample_to_objective")):
        sf = _lib.SurfaceTermArgs()
        sf.w_point_surface, sf.w_vert_surface = wp, wv
        sg = _lib.SurfaceGateArgs()
        sg.min_cos_point, sg.min_cos_vert = (0.3 if scp else -1.0), (0.3 if scv else -1.0)
        if out and scv and wv > 0:                       # (refused otherwise: vert_normals given without min_cos_vert)
            sg.vert_normals = 1 << 20
        cg = _lib.ChamferGateArgs()
        cg.min_cos_point, cg.min_cos_vert, cg.reject_boundary = (0.3 if ccp else -1.0), (0.3 if ccv else -1.0), int(bound)
        sampled = points.startswith("sample")
        s_cos_point, s_cos_vert = wp > 0 and scp, wv > 0 and scv
        c_cos, c_bound = wc > 0 and (ccp or ccv), wc > 0 and bound
        src = lambda on: "drawn" if sampled and on else "callers"
        want = dict(draw_normals=bool(sampled and (s_cos_point or c_cos)), draw_boundary=bool(sampled and c_bound),
                    surface_normals=src(s_cos_point), chamfer_normals=src(c_cos), chamfer_boundary=src(c_bound),
                    vert_normals="surface_gate_block" if s_cos_vert and out else "objective",
                    surface_reuses_vert_normals=bool(c_cos and s_cos_vert))
        assert plan.plan_fit3d_riders(sf, sg, cg, wc, points) == want, (wp, wv, scp, scv, ccp, ccv, bound, wc, out, points)
        checked += 1
    assert checked == 2 ** 9 * 4
    # absent blocks are blocks with everything off; a gate block without its surface block's weights gates nothing
    off = dict(draw_normals=False, draw_boundary=False, surface_normals="callers", chamfer_normals="callers", chamfer_boundary="callers",
               vert_normals="objective", surface_reuses_vert_normals=False)
    assert plan.plan_fit3d_riders(None, None, None, 1.0, "sample_to_caller") == off
    sf, sg = _lib.SurfaceTermArgs(), _lib.SurfaceGateArgs()
    sg.min_cos_point = sg.min_cos_vert = 0.5
    assert plan.plan_fit3d_riders(sf, sg, None, 1.0, "sample_to_caller") == off
    sf.w_point_surface = 1.0
    assert plan.plan_fit3d_riders(sf, None, None, 1.0, "sample_to_caller") == off
    assert plan.plan_fit3d_riders(sf, sg, None, 0.0, "sample_to_objective") == dict(off, draw_normals=True, surface_normals="drawn")
