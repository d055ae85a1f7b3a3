"""GPU: the refusals smalfit_plan.h words for the entry points beside smalfit_fit_eval (tests/test_host_plan_cpu.py holds the
texts and their order on the CPU) reach smalfit_last_error() behind the name of the entry point that met them.  An engine of 2
frames at 32 x 32 without priors; every call is refused before anything is launched, so the pointers are dummies of the smallest
valid shapes and a case takes no time.  The mesh entry points get two objectives of capacity 2 meshes x 8 points: a tetrahedron
(the create, eval and sample rules, and "different meshes" against the engine) and one over the model's own faces (the rules of
smalfit_fit3d_step behind that one), with target sets of one and of two tetrahedra."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from smalify_amd import _lib, engine as eng  # noqa: E402
from tests import parity_cases as pc  # noqa: E402

M, S = 2, 32
POINTS = 8
TET_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
TET_F = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int32)
_CTX = {}


def _ctx():
    if not _CTX:
        _, _, dm = pc.get_model()
        _CTX["dm"], _CTX["e"] = dm, eng.Engine(dm, M, S)
        _CTX["buf"] = torch.zeros(M * 4096, device="cuda")
        _CTX["lo"], _CTX["hi"] = np.full(102, -1.0, np.float32), np.full(102, 1.0, np.float32)
        _CTX["tet"] = eng.MeshObjective(4, TET_F, M, POINTS)
        _CTX["obj"] = eng.MeshObjective(dm.num_verts, np.asarray(dm.data.faces, np.int32), M, POINTS)
        _CTX["tgt1"], _CTX["tgt2"] = eng.MeshTargets([TET_V], [TET_F]), eng.MeshTargets([TET_V, TET_V], [TET_F, TET_F])
        # host arrays the mesh cases point at: faces (good, an index out of range, a repeated vertex), counts, vertices, weights
        far, twice = TET_F.copy(), TET_F.copy()
        far[2, 1], twice[1, 2] = 4, twice[1, 1]
        _CTX["host"] = dict(F=TET_F, F_FAR=far, F_TWICE=twice, V=TET_V, V_FLAT=np.zeros_like(TET_V), C4=np.array([4], np.int32),
                            C0=np.array([0], np.int32), W_ON=np.array([1.0, 1.0, 0.01, 0.1], np.float32),
                            W_OFF=np.array([0.0, 1.0, 0.01, 0.1], np.float32))
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


FIT3D_TENSORS = ("betas", "global_rot", "joint_rot", "trans", "deform_verts")


def _fit3d(D, **fields):
    """a block smalfit_fit3d_step accepts with the model-face objective and two target meshes: every tensor trained at step 1"""
    a = _lib.Fit3dArgs()
    a.num_meshes, a.num_betas, a.num_points, a.adam_t = M, 20, POINTS, 1
    a.beta1, a.beta2, a.eps = 0.9, 0.999, 1e-8
    a.weights = (C.c_float * 4)(1.0, 1.0, 0.01, 0.1)
    a.losses = D
    for t in FIT3D_TENSORS:
        for prefix in ("", "m_", "v_"):
            setattr(a, prefix + t, D)
        setattr(a, "lr_" + t, 0.01)
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def _eval(k, **bent):
    """arguments of smalfit_mesh_objective_eval the tetrahedron objective accepts, bent"""
    a = dict(m=k.TET, st=k.ST, N=M, lbs=k.D, trans=k.D, deform=None, points=k.D, S=POINTS, w=k.H["W_ON"], verts=None, losses=k.D, dverts=k.D,
             dtrans=k.D)
    a.update(bent)
    return tuple(a.values())


def _targets(k, **bent):
    a = dict(N=1, vc=k.H["C4"], fc=k.H["C4"], verts=k.H["V"], faces=k.H["F"], out=C.byref(C.c_void_p()))
    a.update(bent)
    return tuple(a.values())


def _step(k, m=None, t="TGT2", **fields):
    return (k.E, k.OBJ if m is None else m, getattr(k, t) if t else None, k.ST, C.byref(_fit3d(k.D, **fields)))


MESHES_TEXT = "num_meshes exceeds the engine's max_frames or the objective's max_meshes"
EVAL_POINTS_TEXT = "the chamfer term needs 1 <= num_points <= max_points target points"
POSITIVE_TEXT = "max_meshes and max_points must be positive"
TRAINED_TEXT = "%s is trained (lr > 0) but its parameter or Adam state is missing"
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
    # ---- the mesh objective
    "mesh_objective_create null": ("smalfit_mesh_objective_create", lambda k: (4, 4, None, M, POINTS, C.byref(C.c_void_p())), "null argument"),
    "mesh_objective_create out": ("smalfit_mesh_objective_create", lambda k: (4, 4, k.H["F"], M, POINTS, None), "null argument"),
    "mesh_objective_create meshes": ("smalfit_mesh_objective_create", lambda k: (4, 4, k.H["F"], 0, POINTS, C.byref(C.c_void_p())), POSITIVE_TEXT),
    "mesh_objective_create points": ("smalfit_mesh_objective_create", lambda k: (4, 4, k.H["F"], M, 0, C.byref(C.c_void_p())), POSITIVE_TEXT),
    "mesh_objective_create null first": ("smalfit_mesh_objective_create", lambda k: (4, 4, None, 0, 0, C.byref(C.c_void_p())), "null argument"),
    "mesh_objective_create empty": ("smalfit_mesh_objective_create", lambda k: (0, 4, k.H["F"], M, POINTS, C.byref(C.c_void_p())),
                                    "mesh topology: empty mesh"),
    "mesh_objective_create index": ("smalfit_mesh_objective_create", lambda k: (4, 4, k.H["F_FAR"], M, POINTS, C.byref(C.c_void_p())),
                                    "mesh topology: face index out of range"),
    "mesh_objective_create repeated": ("smalfit_mesh_objective_create", lambda k: (4, 4, k.H["F_TWICE"], M, POINTS, C.byref(C.c_void_p())),
                                       "mesh topology: degenerate face (repeated vertex)"),
    "mesh_objective_create capacity first": ("smalfit_mesh_objective_create", lambda k: (4, 4, k.H["F_FAR"], M, 0, C.byref(C.c_void_p())), POSITIVE_TEXT),
    "mesh_objective_counts": ("smalfit_mesh_objective_counts", lambda k: (None, None, None), "null handle"),
    "mesh_objective_eval null": ("smalfit_mesh_objective_eval", lambda k: _eval(k, lbs=None), "null argument"),
    "mesh_objective_eval handle": ("smalfit_mesh_objective_eval", lambda k: _eval(k, m=None), "null argument"),
    "mesh_objective_eval weights": ("smalfit_mesh_objective_eval", lambda k: _eval(k, w=None), "null argument"),
    "mesh_objective_eval losses": ("smalfit_mesh_objective_eval", lambda k: _eval(k, losses=None, N=0), "null argument"),
    "mesh_objective_eval meshes 0": ("smalfit_mesh_objective_eval", lambda k: _eval(k, N=0), "num_meshes out of range"),
    "mesh_objective_eval meshes": ("smalfit_mesh_objective_eval", lambda k: _eval(k, N=M + 1, S=POINTS + 1), "num_meshes out of range"),
    "mesh_objective_eval no points": ("smalfit_mesh_objective_eval", lambda k: _eval(k, points=None), EVAL_POINTS_TEXT),
    "mesh_objective_eval points 0": ("smalfit_mesh_objective_eval", lambda k: _eval(k, S=0), EVAL_POINTS_TEXT),
    "mesh_objective_eval points": ("smalfit_mesh_objective_eval", lambda k: _eval(k, S=POINTS + 1), EVAL_POINTS_TEXT),
    "mesh_targets_create null": ("smalfit_mesh_targets_create", lambda k: _targets(k, verts=None), "null argument"),
    "mesh_targets_create out": ("smalfit_mesh_targets_create", lambda k: _targets(k, out=None, N=0), "null argument"),
    "mesh_targets_create none": ("smalfit_mesh_targets_create", lambda k: _targets(k, N=0), "no meshes"),
    "mesh_targets_create empty": ("smalfit_mesh_targets_create", lambda k: _targets(k, vc=k.H["C0"]), "empty target mesh"),
    "mesh_targets_create faceless": ("smalfit_mesh_targets_create", lambda k: _targets(k, fc=k.H["C0"], faces=k.H["F_FAR"]), "empty target mesh"),
    "mesh_targets_create index": ("smalfit_mesh_targets_create", lambda k: _targets(k, faces=k.H["F_FAR"]), "target mesh: face index out of range"),
    "mesh_targets_create flat": ("smalfit_mesh_targets_create", lambda k: _targets(k, verts=k.H["V_FLAT"]), "target mesh: zero surface area"),
    "mesh_targets_sample null": ("smalfit_mesh_targets_sample", lambda k: (None, k.ST, POINTS, 1, 0, k.D), "null argument"),
    "mesh_targets_sample out": ("smalfit_mesh_targets_sample", lambda k: (k.TGT2, k.ST, 0, 1, 0, None), "null argument"),
    "mesh_targets_sample points": ("smalfit_mesh_targets_sample", lambda k: (k.TGT2, k.ST, 0, 1, 0, k.D), "num_points must be positive"),
    # ---- smalfit_fit3d_step
    "fit3d_step null": ("smalfit_fit3d_step", lambda k: (k.E, k.OBJ, k.TGT2, k.ST, None), "null argument"),
    "fit3d_step objective": ("smalfit_fit3d_step", lambda k: (k.E, None, k.TGT2, k.ST, C.byref(_fit3d(k.D))), "null argument"),
    "fit3d_step meshes 0": ("smalfit_fit3d_step", lambda k: _step(k, num_meshes=0), MESHES_TEXT),
    "fit3d_step meshes": ("smalfit_fit3d_step", lambda k: _step(k, m=k.TET, num_meshes=M + 1), MESHES_TEXT),
    "fit3d_step different meshes": ("smalfit_fit3d_step", lambda k: _step(k, m=k.TET), "engine and objective were built for different meshes"),
    "fit3d_step different meshes first": ("smalfit_fit3d_step", lambda k: _step(k, m=k.TET, num_betas=0, betas=None),
                                          "engine and objective were built for different meshes"),
    "fit3d_step betas 0": ("smalfit_fit3d_step", lambda k: _step(k, num_betas=0), "num_betas out of range"),
    "fit3d_step betas": ("smalfit_fit3d_step", lambda k: _step(k, num_betas=42, trans=None), "num_betas out of range"),
    "fit3d_step parameter": ("smalfit_fit3d_step", lambda k: _step(k, joint_rot=None, num_points=0), "missing parameter / losses pointer"),
    "fit3d_step losses": ("smalfit_fit3d_step", lambda k: _step(k, losses=None), "missing parameter / losses pointer"),
    "fit3d_step points 0": ("smalfit_fit3d_step", lambda k: _step(k, num_points=0), "the chamfer term needs 1 <= num_points <= max_points"),
    "fit3d_step points": ("smalfit_fit3d_step", lambda k: _step(k, t=None, num_points=POINTS + 1), "the chamfer term needs 1 <= num_points <= max_points"),
    "fit3d_step no targets": ("smalfit_fit3d_step", lambda k: _step(k, t=None, m_betas=None), "neither target points nor target meshes given"),
    "fit3d_step target count": ("smalfit_fit3d_step", lambda k: _step(k, t="TGT1", adam_t=0), "number of target meshes differs from num_meshes"),
    "fit3d_step betas state": ("smalfit_fit3d_step", lambda k: _step(k, m_betas=None, v_trans=None), TRAINED_TEXT % "betas"),
    "fit3d_step global_rot state": ("smalfit_fit3d_step", lambda k: _step(k, v_global_rot=None, m_joint_rot=None), TRAINED_TEXT % "global_rot"),
    "fit3d_step joint_rot state": ("smalfit_fit3d_step", lambda k: _step(k, m_joint_rot=None, deform_verts=None), TRAINED_TEXT % "joint_rot"),
    "fit3d_step trans state": ("smalfit_fit3d_step", lambda k: _step(k, v_trans=None, adam_t=0), TRAINED_TEXT % "trans"),
    "fit3d_step deform_verts": ("smalfit_fit3d_step", lambda k: _step(k, deform_verts=None), TRAINED_TEXT % "deform_verts"),
    "fit3d_step deform_verts state": ("smalfit_fit3d_step", lambda k: _step(k, points=k.D, t=None, m_deform_verts=None, adam_t=0),
                                      TRAINED_TEXT % "deform_verts"),
    "fit3d_step adam_t": ("smalfit_fit3d_step", lambda k: _step(k, adam_t=0), "adam_t must be the 1-based step count"),
}


class _Handles:
    def __init__(self):
        c = _ctx()
        self.E, self.MODEL, self.ST = c["e"].handle, c["dm"].handle, eng._stream()
        self.D, self.LO, self.HI = c["buf"].data_ptr(), c["lo"].ctypes.data, c["hi"].ctypes.data
        self.TET, self.OBJ, self.TGT1, self.TGT2 = c["tet"].handle, c["obj"].handle, c["tgt1"].handle, c["tgt2"].handle
        self.H = {name: a.ctypes.data for name, a in c["host"].items()}


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
