"""GPU: the refusals smalfit_plan.h words for the entry points beside smalfit_fit_eval (tests/test_host_plan_cpu.py holds the
texts and their order on the CPU) reach smalfit_last_error() behind the name of the entry point that met them.  An engine of 2
frames at 32 x 32 without priors; every call is refused before anything is launched, so the pointers are dummies of the smallest
valid shapes and a case takes no time."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from smalify_amd import _lib, engine as eng  # noqa: E402
from tests import parity_cases as pc  # noqa: E402

M, S = 2, 32
_CTX = {}


def _ctx():
    if not _CTX:
        _, _, dm = pc.get_model()
        _CTX["dm"], _CTX["e"] = dm, eng.Engine(dm, M, S)
        _CTX["buf"] = torch.zeros(M * 4096, device="cuda")
        _CTX["lo"], _CTX["hi"] = np.full(102, -1.0, np.float32), np.full(102, 1.0, np.float32)
    return _CTX


def _fit(**fields):
    a = _lib.FitArgs()
    a.num_frames, a.window, a.logscale_mode = M, 1, 0
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def _adam(D, **fields):
    o = _lib.AdamArgs()
    o.param = o.grad = o.exp_avg = o.exp_avg_sq = D
    for k, v in fields.items():
        setattr(o, k, v)
    return o


def _lbs(D, **fields):
    a = _lib.LbsArgs()
    a.num_frames, a.num_betas, a.beta, a.theta, a.verts, a.joints = M, 20, D, D, D, D
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def _shard(D, **fields):
    sh = _lib.ShardArgs()
    sh.world_size, sh.rank, sh.num_shared, sh.num_trainable_shared = 2, 1, 26, 20
    sh.shared_grad = sh.record = sh.gathered = sh.allgather = D       # (the collective is never called: refused before the loop)
    for k, v in fields.items():
        setattr(sh, k, v)
    return sh


SHARD_TEXT = "subject_frames != 0 cannot be sharded (independent images need no collective: give each rank its own batch)"
FRAMES_TEXT = "num_frames exceeds the engine's max_frames"
ONE_OF_TEXT = "give exactly one of theta (axis-angle) and Rs (rotation matrices)"
# name: (entry point, arguments given the engine handle E, the model handle MODEL, a device pointer D, host limit tables LO / HI
#        and the stream ST, the text)
CASES = {
    "engine_create frames": ("smalfit_engine_create", lambda k: (k.MODEL, 0, S, C.byref(C.c_void_p())), "bad argument"),
    "engine_create size 0": ("smalfit_engine_create", lambda k: (k.MODEL, M, 0, C.byref(C.c_void_p())), "bad argument"),
    "engine_create size": ("smalfit_engine_create", lambda k: (k.MODEL, M, 1025, C.byref(C.c_void_p())),
                           "image_size above 1024 is not supported (float32 pixel walk, see kernels_raster.inc)"),
    "set_shape_prior 27": ("smalfit_engine_set_shape_prior", lambda k: (k.E, k.LO, k.LO, 27), "bad argument (dim must be 1..26)"),
    "set_shape_prior 0": ("smalfit_engine_set_shape_prior", lambda k: (k.E, k.LO, k.LO, 0), "bad argument (dim must be 1..26)"),
    "set_joint_limits null": ("smalfit_engine_set_joint_limits", lambda k: (k.E, k.LO, None), "null argument"),
    "set_joint_limits order": ("smalfit_engine_set_joint_limits", lambda k: (k.E, k.HI, k.LO), "min must not exceed max"),
    "set_option value": ("smalfit_engine_set_option", lambda k: (k.E, 1, 2), "SMALFIT_OPT_UNCLAMPED_EDGE_T takes 0 or 1"),
    "set_option unknown": ("smalfit_engine_set_option", lambda k: (k.E, 99, 0), "unknown option"),
    "profile_begin": ("smalfit_engine_profile_begin", lambda k: (k.E, 0, 1), "bad argument"),
    "lbs_forward_ex null": ("smalfit_lbs_forward_ex", lambda k: (k.E, k.ST, None), "null argument"),
    "lbs_forward_ex frames": ("smalfit_lbs_forward_ex", lambda k: (k.E, k.ST, C.byref(_lbs(k.D, num_frames=M + 1))), FRAMES_TEXT),
    "lbs_forward_ex betas": ("smalfit_lbs_forward_ex", lambda k: (k.E, k.ST, C.byref(_lbs(k.D, num_betas=0))), "num_betas out of range"),
    "lbs_forward_ex beta": ("smalfit_lbs_forward_ex", lambda k: (k.E, k.ST, C.byref(_lbs(k.D, beta=None))), "beta missing"),
    "lbs_forward_ex both": ("smalfit_lbs_forward_ex", lambda k: (k.E, k.ST, C.byref(_lbs(k.D, Rs=k.D))), ONE_OF_TEXT),
    "lbs_forward_ex outputs": ("smalfit_lbs_forward_ex", lambda k: (k.E, k.ST, C.byref(_lbs(k.D, verts=None))), "verts / joints outputs missing"),
    "lbs_backward_ex frames": ("smalfit_lbs_backward_ex", lambda k: (k.E, k.ST, C.byref(_lbs(k.D, num_frames=0))), FRAMES_TEXT),
    "lbs_backward_ex neither": ("smalfit_lbs_backward_ex", lambda k: (k.E, k.ST, C.byref(_lbs(k.D, theta=None))), ONE_OF_TEXT),
    "lbs_forward theta": ("smalfit_lbs_forward", lambda k: (k.E, k.ST, M, 20, k.D, None, None, k.D, k.D, None, None), "null argument"),
    "lbs_backward theta": ("smalfit_lbs_backward", lambda k: (k.E, k.ST, M, 20, k.D, None, None, k.D, k.D, k.D, k.D, None), "null argument"),
    "rodrigues": ("smalfit_rodrigues", lambda k: (k.ST, 0, k.D, k.D), "bad argument"),
    "rodrigues_backward": ("smalfit_rodrigues_backward", lambda k: (k.ST, 1, k.D, None, k.D), "bad argument"),
    "global_rigid_transformation": ("smalfit_global_rigid_transformation", lambda k: (k.ST, 0, k.D, k.D, k.D, None, k.D, k.D), "bad argument"),
    "global_rigid_transformation_backward": ("smalfit_global_rigid_transformation_backward",
                                             lambda k: (k.ST, 1, k.D, k.D, k.D, None, k.D, k.D, None, k.D, k.D, None), "bad argument"),
    "project_points_backward": ("smalfit_project_points_backward", lambda k: (k.ST, 0, S, k.D, k.D, k.D), "bad argument"),
    "render_forward null": ("smalfit_render_forward", lambda k: (k.E, k.ST, M, None, None, 0, k.D, None), "null argument"),
    "render_forward frames": ("smalfit_render_forward", lambda k: (k.E, k.ST, M + 1, k.D, None, 0, k.D, None), "M exceeds the engine's max_frames"),
    "render_color frames": ("smalfit_render_color", lambda k: (k.E, k.ST, 0, k.D, k.LO, k.D), "M exceeds the engine's max_frames"),
    "render_backward frames": ("smalfit_render_backward", lambda k: (k.E, k.ST, M + 1, k.D, k.D, k.D, k.D), "M exceeds the engine's max_frames"),
    "pose_prior count": ("smalfit_pose_prior", lambda k: (k.E, k.ST, 0, k.D, k.D), "bad argument"),
    "pose_prior unset": ("smalfit_pose_prior", lambda k: (k.E, k.ST, 1, k.D, k.D), "pose prior not set"),
    "pose_prior_backward unset": ("smalfit_pose_prior_backward", lambda k: (k.E, k.ST, 1, k.D, k.D, k.D), "pose prior not set"),
    "temporal null": ("smalfit_temporal", lambda k: (k.E, k.ST, M, 1.0, k.D, k.D, k.D, None, None, None, None, None, None), "null argument"),
    "temporal frames": ("smalfit_temporal", lambda k: (k.E, k.ST, M + 1, 1.0, k.D, k.D, k.D, None, None, k.D, None, None, None),
                        "N exceeds the engine's max_frames"),
    "adam_step": ("smalfit_adam_step", lambda k: (k.ST, 0, k.D, k.D, k.D, k.D, 0.1, 0.5, 0.999, 1e-8, 1), "bad argument"),
    "adam_step t": ("smalfit_adam_step", lambda k: (k.ST, 1, k.D, k.D, k.D, k.D, 0.1, 0.5, 0.999, 1e-8, 0), "bad argument"),
    "adam_segments step": ("smalfit_adam_segments", lambda k: (k.ST, C.byref(_adam(k.D, step=-1))), "step must be >= 0"),
    "fit_eval null": ("smalfit_fit_eval", lambda k: (k.E, k.ST, None), "null argument"),
    "fit_run iterations": ("smalfit_fit_run", lambda k: (k.E, k.ST, C.byref(_fit()), C.byref(_adam(k.D)), 0), "iterations must be positive"),
    "fit_run step": ("smalfit_fit_run", lambda k: (k.E, k.ST, C.byref(_fit()), C.byref(_adam(k.D, step=-1)), 1), "step must be >= 0"),
    "shard_record": ("smalfit_shard_record", lambda k: (k.ST, 26, k.D, 0, k.D, k.D, k.D, k.D, k.D, k.D), "bad argument"),
    "shard_local_step step": ("smalfit_shard_local_step", lambda k: (k.E, k.ST, C.byref(_fit()), C.byref(_adam(k.D, step=-1)), 26, k.D, k.D),
                              "step must be >= 0"),
    "shard_local_step subject": ("smalfit_shard_local_step",
                                 lambda k: (k.E, k.ST, C.byref(_fit(subject_frames=1)), C.byref(_adam(k.D)), 26, k.D, k.D), SHARD_TEXT),
    "shard_reduce_step": ("smalfit_shard_reduce_step", lambda k: (k.ST, 0, 242, k.D, 26, 20, C.byref(_adam(k.D))), "bad argument"),
    "shard_reduce_step state": ("smalfit_shard_reduce_step", lambda k: (k.ST, 2, 242, k.D, 26, 20, C.byref(_adam(k.D, grad=None))),
                                "bad optimiser state"),
    "shard_run size": ("smalfit_shard_run", lambda k: (k.E, k.ST, C.byref(_fit()), C.byref(_adam(k.D)), C.byref(_adam(k.D)),
                                                       C.byref(_shard(k.D, struct_size=8)), 1),
                       "smalfit_shard_args.struct_size does not match this library (built against another smalfit.h?)"),
    "shard_run iterations": ("smalfit_shard_run", lambda k: (k.E, k.ST, C.byref(_fit()), C.byref(_adam(k.D)), C.byref(_adam(k.D)),
                                                             C.byref(_shard(k.D)), 0), "iterations must be positive"),
    "shard_run rank": ("smalfit_shard_run", lambda k: (k.E, k.ST, C.byref(_fit()), C.byref(_adam(k.D)), C.byref(_adam(k.D)),
                                                       C.byref(_shard(k.D, rank=2)), 1), "bad rank / world_size"),
    "shard_run shared": ("smalfit_shard_run", lambda k: (k.E, k.ST, C.byref(_fit()), C.byref(_adam(k.D)), C.byref(_adam(k.D)),
                                                         C.byref(_shard(k.D, num_trainable_shared=27)), 1), "bad num_shared / num_trainable_shared"),
    "shard_run buffers": ("smalfit_shard_run", lambda k: (k.E, k.ST, C.byref(_fit()), C.byref(_adam(k.D)), C.byref(_adam(k.D)),
                                                          C.byref(_shard(k.D, record=None)), 1), "missing buffer / collective"),
    "shard_run steps": ("smalfit_shard_run", lambda k: (k.E, k.ST, C.byref(_fit()), C.byref(_adam(k.D, step=1)), C.byref(_adam(k.D, step=2)),
                                                        C.byref(_shard(k.D)), 1), "adam_local and adam_shared must carry the same step >= 0"),
    "shard_run subject": ("smalfit_shard_run", lambda k: (k.E, k.ST, C.byref(_fit(subject_frames=1)), C.byref(_adam(k.D)), C.byref(_adam(k.D)),
                                                          C.byref(_shard(k.D)), 1), SHARD_TEXT),
}


class _Handles:
    def __init__(self):
        c = _ctx()
        self.E, self.MODEL, self.ST = c["e"].handle, c["dm"].handle, eng._stream()
        self.D, self.LO, self.HI = c["buf"].data_ptr(), c["lo"].ctypes.data, c["hi"].ctypes.data


@pytest.mark.parametrize("name", list(CASES))
def test_refusal_reaches_last_error(name):
    entry, args, text = CASES[name]
    k = _Handles()
    e = _ctx()["e"]
    rc = getattr(e.lib, entry)(*args(k))
    assert rc != 0
    assert e.lib.smalfit_last_error().decode() == entry + ": " + text
    torch.cuda.synchronize()
    assert not _ctx()["buf"].any() and e.status() == 0          # nothing was launched on the dummies


def test_graph_replay_refuses_independent_images():
    """smalfit_fit_run under smalfit_engine_set_graph: refused before a capture could begin"""
    k = _Handles()
    e = _ctx()["e"]
    e.set_graph(True)
    try:
        rc = e.lib.smalfit_fit_run(k.E, k.ST, C.byref(_fit(subject_frames=1)), C.byref(_adam(k.D)), 2)
        assert rc != 0
        assert e.lib.smalfit_last_error().decode() == "smalfit_fit_run: subject_frames != 0 is not supported by the graph replay (smalfit_engine_set_graph)"
    finally:
        e.set_graph(False)
