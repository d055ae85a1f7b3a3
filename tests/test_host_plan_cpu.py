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
