"""The host's launch decisions (smalify_amd/csrc/smalfit_plan.h) and the model packer (smal_model_pack.h) as Python calls:
tests/host_plan_shim.cpp built and loaded by tests/host_shim.py, each function returning what the restatements of
tests/fold_forms.py, lbs_forms.py and mesh3d_forms.py return, so that a test compares the two with `==`.  The CPU tests call
load() from a module fixture; nothing here needs a GPU, and nothing the GPU tests import needs this file."""
from __future__ import annotations

import ctypes as C

import numpy as np

from smalify_amd import _lib
from tests import fold_forms as ff
from tests import host_shim


LOOPS = ("graph", "folded", "plain")                                  # RunLoop
SKIN_FORMS = ("plain", "split", "wide")                               # SkinForm
REASONS = (None, "cut", "gradient", "alias", "nothing", "extra")      # FoldRefusal
HEAD_PRIORS = {"none": 0, "shared": 1, "per_frame": 2}                # HeadPrior
HEAD_KERNELS = ("plain", "images", "step")                            # HeadKernel
SIL_TARGETS = ("none", "f32", "u8")                                   # SilTargetKind
LOSS_LAUNCHES = ("own_kernel", "in_resolve")                          # LossLaunch
# EvalPlan as hp_plan_eval lays it out
EVAL_INTS = ("M", "window", "frame_offset", "sequence_frames", "independent", "nb", "betas_stride", "ls_stride", "limb_scales",
             "shape_prior", "prior_dim", "prior_uses_ls", "prior_windows", "prior_per_frame", "head_prior", "head",
             "sil_on", "rasterise", "sil_target", "frame_loss", "queue_loss", "raster_backward", "loss_launch",
             "joints_in_head", "halos", "verts_out", "need_pose", "need_beta", "need_ls", "bwd_betas_shared", "j_stride",
             "asm_betas_shared", "asm_ls_shared", "ngrp_beta", "asm_shape_sets", "rows", "W", "ls_rows", "clear_qloss",
             "assembly_leaves_betas", "assembly_leaves_scales")
EVAL_FLOATS = ("prior_weight", "w_temp", "w_limit")
EVAL_NAMED = {"head_prior": ("none", "shared", "per_frame"), "head": HEAD_KERNELS, "sil_target": SIL_TARGETS, "loss_launch": LOSS_LAUNCHES}
GRID_CONSTANTS = ("SWEEP_FACES", "BWD_FACES", "BWD_LANES", "RES_EDGE", "RECT_FACES", "ASM_ELEM", "ASM_LOSS", "ASM_ROWS", "BAND_BLOCKS",
                  "SELECT_BLOCKS", "SEL_WAVES", "SEL_GROUPS", "PBM_SPLITS", "PBM_TILES", "FRAME_LOSS_STRIDE", "JOINT_BLOCKS", "SKIN_VERTS",
                  "SKIN_THREADS", "QUEUE_LOSS_BLOCKS")
# model_tables of smal_model_pack.h: the order of the model's device blob
MODEL_TABLES = ("vt", "sd", "pd", "w_j", "w_val", "wc_off", "wc_v", "wc_val", "jr_off", "jr_v", "jr_val", "jrv_j", "jrv_val", "Jt", "JS",
                "parents", "faces_int", "vf_off", "vf_idx", "sidx")
FIT3D_TENSORS = ("betas", "global_rot", "joint_rot", "trans", "deform_verts")           # the order of kFit3dParams
FIT3D_POINTS = ("none", "sample_to_objective", "sample_to_caller", "callers", "callers_copied")   # Fit3dPoints
RIDER_SOURCES = ("callers", "drawn")                                  # RiderSource
VERT_NORMALS_DESTS = ("objective", "surface_gate_block")              # VertNormalsDest
# Fit3dFacts: an engine of 4 frames on the stand-in's dimensions, an objective over the same mesh, two target meshes
FIT3D_FACT_NAMES = ("max_frames", "model_verts", "model_betas", "max_meshes", "max_points", "objective_verts", "targets", "target_meshes")
FIT3D_FACTS = dict(max_frames=4, model_verts=3889, model_betas=41, max_meshes=4, max_points=64, objective_verts=3889, targets=True,
                   target_meshes=2)


class Plan:
    def __init__(self, lib):
        self.lib = lib
        for name in ("hp_fit_args_refusal", "hp_fit_args_size_refusal", "hp_pack_adam_segments", "hp_model_dims_refusal",
                     "hp_fit_model_refusal", "hp_null_argument_refusal", "hp_operator_args_refusal", "hp_step_refusal",
                     "hp_iterations_refusal", "hp_engine_create_refusal", "hp_shape_prior_refusal", "hp_joint_limits_refusal",
                     "hp_option_refusal", "hp_profile_begin_refusal", "hp_lbs_args_refusal", "hp_lbs_outputs_refusal",
                     "hp_render_frames_refusal", "hp_temporal_frames_refusal", "hp_pose_prior_refusal", "hp_graph_subject_refusal",
                     "hp_shard_subject_refusal", "hp_shard_record_refusal", "hp_shard_reduce_refusal", "hp_shard_run_refusal",
                     "hp_adam_step_refusal", "hp_window_rows_refusal", "hp_model_desc_refusal", "hp_null_handle_refusal",
                     "hp_mesh_objective_create_refusal", "hp_mesh_eval_refusal", "hp_mesh_targets_create_refusal",
                     "hp_mesh_sample_refusal", "hp_fit3d_args_refusal"):
            getattr(lib, name).restype = C.c_char_p
        lib.hp_mesh_eval_refusal.argtypes = [C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int]
        lib.hp_mesh_targets_create_refusal.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        lib.hp_pack_model.restype = C.c_void_p
        lib.hp_pack_model.argtypes = [C.c_void_p]
        lib.hp_pack_free.argtypes = [C.c_void_p]
        lib.hp_pack_dims.argtypes = [C.c_void_p, C.c_void_p]
        lib.hp_pack_table.restype = lib.hp_pack_blob.restype = C.c_void_p
        lib.hp_pack_table.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        lib.hp_pack_blob.argtypes = [C.c_void_p, C.c_void_p]
        lib.hp_elem_blocks.argtypes = [C.c_longlong]
        lib.hp_joint_limits_refusal.argtypes = [C.c_void_p, C.c_void_p]
        out = (C.c_int * len(GRID_CONSTANTS))()
        lib.hp_grid_constants(out)
        for name, value in zip(GRID_CONSTANTS, out):
            setattr(self, name, value)
        lib.hp_mesh_weight.restype = C.c_float
        lib.hp_mesh_weight.argtypes = [C.c_float]
        lib.hp_mesh_points.argtypes = [C.c_float, C.c_int]
        lib.hp_plan_fit3d_riders.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_void_p]
        out = (C.c_int * 8)()
        lib.hp_constants(out)
        (self.BETA_GROUPS, self.MAX_IMAGE_SIZE, self.MESH_QUERIES, self.MESH_THREADS, self.HEAD_PRIOR_FRAMES, self.CALLER,
         self.SHARED_SLOT_FLOATS, self.SIZEOF_FIT_ARGS) = list(out)

    # ---- smalfit_fit_run ----
    def path(self, iterations, graph, profiled, default_stream, accepted):
        return LOOPS[self.lib.hp_run_loop(int(graph), int(profiled), iterations, int(not default_stream), int(accepted))]

    def plan_fold(self, M, logscale_mode, offsets, ranges, grad_at_offset, subject_frames=0):
        """fold_forms.plan_fold's arguments and result; a tensor missing from `offsets` is a null pointer"""
        off = (C.c_longlong * 5)(*[offsets.get(k, 0) for k in ff.TENSORS])
        present = (C.c_int * 5)(*[int(k in offsets) for k in ff.TENSORS])
        gao = (C.c_int * 5)(*[int(bool(grad_at_offset.get(k, False))) for k in ff.TENSORS])
        beg = (C.c_int * 4)(*[b for b, _ in ranges])
        end = (C.c_int * 4)(*[e for _, e in ranges])
        train, at = (C.c_int * 5)(), (C.c_int * 5)()
        why = self.lib.hp_plan_fold(M, logscale_mode, subject_frames, off, present, gao, len(ranges), beg, end, train, at)
        assert why >= 0, "the ranges themselves were refused"
        trained = {k: bool(train[i]) for i, k in enumerate(ff.TENSORS)}
        assert all(at[i] == offsets[k] for i, k in enumerate(ff.TENSORS) if trained[k])
        return why == 0, trained, REASONS[why]

    def _place(self, slot):
        return "caller" if slot == self.CALLER else slot

    def shared_travel(self, iterations):
        out, rw = [], (C.c_int * 2)()
        for it in range(iterations - 1):
            self.lib.hp_shared_route(it, iterations, rw)
            out.append((self._place(rw[0]), self._place(rw[1])))
        return out

    def restore_slot(self, iterations, shared_trained=True):
        slot = self.lib.hp_restore_slot(iterations, int(shared_trained))
        return None if slot == self.CALLER else slot

    def prior_slot(self, it):
        return self.lib.hp_prior_slot(it)

    def prior_windows(self, window, frame_offset, M):
        return self.lib.hp_prior_windows(window, frame_offset, M)

    def tensor_is_shared(self, k, logscale_mode):
        return bool(self.lib.hp_tensor_is_shared(k, logscale_mode))

    def pack_adam_segments(self, adam):
        """-> (refusal text or None, (nseg, beg[4], off[5]))"""
        sg = (C.c_int * 10)()
        why = self.lib.hp_pack_adam_segments(C.byref(adam), sg)
        return (why.decode() if why else None), (sg[0], list(sg[1:5]), list(sg[5:10]))

    # ---- geometry ----
    def padded_verts(self, V):
        return self.lib.hp_padded_verts(V)

    def nblk_beta(self, Vp):
        return self.lib.hp_nblk_beta(Vp)

    def skin_form(self, M, V):
        return SKIN_FORMS[self.lib.hp_skin_form(M, self.padded_verts(V))]

    def head_blocks(self, M, Vp, shape_per_frame, prior):
        return self.lib.hp_head_blocks(M, Vp, int(shape_per_frame), HEAD_PRIORS[prior])

    def dbeta_grid(self, need_beta, Vp, betas_shared, M):
        out = (C.c_int * 3)()
        self.lib.hp_dbeta_grid(int(need_beta), Vp, int(betas_shared), M, out)
        return tuple(out)

    def parents_ordered(self, parents):
        return bool(self.lib.hp_parents_ordered((C.c_int * len(parents))(*parents), len(parents)))

    def tree_levels(self, parents, tables=False):
        """the walks' schedule of a tree of 35 joints (smalfit_plan.h: tree_levels): fast, npass, nlev, walk_passes (passes of
        the table-driven walk: npass without its cap), most_children (of a non-root joint), root_children, max_pass,
        max_children; with tables=True also the flat schedule, pass_joint / pass_parent / pass_nchild [max_pass][8] and
        pass_child [max_pass][8][max_children]"""
        assert len(parents) == 35
        facts, limits = (C.c_int * 6)(), (C.c_int * 2)()
        tab = (C.c_int * (16 * 8 * 8))() if tables else None
        self.lib.hp_tree_levels((C.c_int * 35)(*[int(p) for p in parents]), facts, limits, tab)
        out = dict(zip(("fast", "npass", "nlev", "walk_passes", "most_children", "root_children"), facts))
        out["fast"] = bool(out["fast"])
        out["max_pass"], out["max_children"] = limits
        if tables:
            P, K = out["max_pass"], out["max_children"]
            assert P * 8 * (3 + K) <= len(tab)
            flat = list(tab)
            grid = lambda o: [flat[o + k * 8:o + k * 8 + 8] for k in range(P)]  # noqa: E731
            out["pass_joint"], out["pass_parent"], out["pass_nchild"] = grid(0), grid(P * 8), grid(2 * P * 8)
            out["pass_child"] = [[flat[3 * P * 8 + (k * 8 + s) * K:3 * P * 8 + (k * 8 + s + 1) * K] for s in range(8)] for k in range(P)]
        return out

    def model_dims_refusal(self, V, F, NB):
        why = self.lib.hp_model_dims_refusal(V, F, NB)
        return why.decode() if why else None

    def fit_model_refusal(self, model_betas):
        why = self.lib.hp_fit_model_refusal(model_betas)
        return why.decode() if why else None

    def mesh_grids(self, V, S, P):
        """mesh3d_forms.grids's arguments and result"""
        out = (C.c_int * 4)()
        self.lib.hp_mesh_grids(S, V, P, out)
        return dict(zip(("bx", "by", "bv", "bp"), out))

    def mesh_query_blocks(self, queries):
        return self.lib.hp_mesh_query_blocks(queries)

    def mesh_weight(self, w):
        return self.lib.hp_mesh_weight(w)

    def mesh_points(self, w_chamfer, num_points):
        return self.lib.hp_mesh_points(w_chamfer, num_points)

    # ---- smalfit_model_create ----
    def _desc(self, md):
        """(smalfit_model_desc of a SMALModelData, the arrays it points into), laid out as engine.DeviceModel lays it out"""
        keep = [np.ascontiguousarray(np.asarray(getattr(md, k)), dtype=dt)
                for k, dt in (("v_template", np.float32), ("shapedirs", np.float32), ("posedirs", np.float32), ("J_regressor", np.float32),
                              ("weights", np.float32), ("parents", np.int32), ("faces", np.int32))]
        return _lib.ModelDesc(keep[0].shape[0], keep[6].shape[0], keep[1].shape[0], *[a.ctypes.data for a in keep]), keep

    def model_desc_refusal(self, md):
        desc, keep = self._desc(md)
        why = self.lib.hp_model_desc_refusal(C.byref(desc))
        return why.decode() if why else None

    def default_landmarks(self):
        return self._ints(self.lib.hp_default_landmarks, 6)

    def pack_model(self, md):
        """pack_smal_model of a SMALModelData -> (dims: V, Vp, F, NB, Kw, Kj; tables by MODEL_TABLES name as uint8 arrays; their
        offsets in the blob; the blob smalfit_model_create uploads, as bytes)"""
        desc, keep = self._desc(md)
        h = self.lib.hp_pack_model(C.addressof(desc))
        try:
            assert self.lib.hp_pack_num_tables() == len(MODEL_TABLES)
            dims = (C.c_int * 6)()
            self.lib.hp_pack_dims(h, dims)
            n, off = C.c_ulonglong(), C.c_ulonglong()
            tables, offsets = {}, {}
            for i, name in enumerate(MODEL_TABLES):
                ptr = self.lib.hp_pack_table(h, i, C.byref(n), C.byref(off))
                tables[name], offsets[name] = C.string_at(ptr, n.value), off.value
            ptr = self.lib.hp_pack_blob(h, C.byref(n))
            blob = C.string_at(ptr, n.value)
        finally:
            self.lib.hp_pack_free(h)
        return dict(zip(("V", "Vp", "F", "NB", "Kw", "Kj"), dims)), tables, offsets, blob

    # ---- the mesh objective and smalfit_fit3d_step ----
    def fit3d_args_refusal(self, args, **facts):
        f = dict(FIT3D_FACTS, **facts)
        why = self.lib.hp_fit3d_args_refusal(C.byref(args), (C.c_int * 8)(*[int(f[k]) for k in FIT3D_FACT_NAMES]))
        return why.decode() if why else None

    def plan_fit3d(self, args, model_verts):
        """Fit3dPlan as a dict; points by name, seg: a list of dicts (tensor by name)"""
        ints, segs = (C.c_int * 8)(), (C.c_int * 30)()
        self.lib.hp_plan_fit3d(C.byref(args), model_verts, ints, segs)
        out = dict(zip(("chamfer", "points", "need_pose", "need_beta", "planar_vertex_grad", "any_trained", "nseg", "adam_blocks"), ints))
        for k in ("chamfer", "need_pose", "need_beta", "planar_vertex_grad", "any_trained"):
            out[k] = bool(out[k])
        out["points"] = FIT3D_POINTS[out["points"]]
        out["seg"] = [dict(zip(("tensor", "count", "row_len", "g_stride", "g_offset", "block0"), segs[6 * s:6 * s + 6])) for s in range(out.pop("nseg"))]
        for sg in out["seg"]:
            sg["tensor"] = FIT3D_TENSORS[sg["tensor"]]
        return out

    def plan_fit3d_riders(self, surface, surface_gates, chamfer_gates, w_chamfer, points):
        """Fit3dRiders as a dict; the blocks are ctypes structs of smalify_amd._lib or None, points a name of FIT3D_POINTS;
        the sources by name (RIDER_SOURCES), vert_normals by name (VERT_NORMALS_DESTS)"""
        ref = lambda b: C.byref(b) if b is not None else None
        ints = (C.c_int * 7)()
        self.lib.hp_plan_fit3d_riders(ref(surface), ref(surface_gates), ref(chamfer_gates), float(w_chamfer),
                                      FIT3D_POINTS.index(points), ints)
        out = dict(zip(("draw_normals", "draw_boundary", "surface_normals", "chamfer_normals", "chamfer_boundary", "vert_normals",
                        "surface_reuses_vert_normals"), ints))
        for k in ("draw_normals", "draw_boundary", "surface_reuses_vert_normals"):
            out[k] = bool(out[k])
        for k in ("surface_normals", "chamfer_normals", "chamfer_boundary"):
            out[k] = RIDER_SOURCES[out[k]]
        out["vert_normals"] = VERT_NORMALS_DESTS[out["vert_normals"]]
        return out

    def fit3d_constants(self):
        """(kFit3dParams, sizeof Fit3dAdamSeg, sizeof Fit3dAdamArgs, sizeof smalfit_fit3d_args)"""
        return self._ints(self.lib.hp_fit3d_constants, 4)

    def mesh_compose_blocks(self, N, V):
        return self.lib.hp_mesh_compose_blocks(N, V)

    def mesh_sample_grid(self, S, N):
        return self._ints(self.lib.hp_mesh_sample_grid, 2, S, N)

    def fit3d_adam_blocks(self, count):
        return self.lib.hp_fit3d_adam_blocks(count)

    def frame_betas_grid(self, M):
        return self.lib.hp_frame_betas_grid(M)

    # ---- smalfit_fit_args ----
    def fit_args_refusal(self, args, max_frames, has_pose_prior, shape_dim):
        why = self.lib.hp_fit_args_refusal(C.byref(args), max_frames, int(has_pose_prior), shape_dim)
        return why.decode() if why else None

    def fit_args_size_refusal(self, args):
        why = self.lib.hp_fit_args_size_refusal(C.byref(args))
        return why.decode() if why else None

    def sequence_frames(self, args):
        return self.lib.hp_sequence_frames(C.byref(args))


    # ---- one evaluation ----
    def plan_eval(self, args, max_frames=8, has_pose_prior=True, shape_dim=26, has_joint_limits=False, pending=False, assemble=True,
                  window_rows=False, want_betas=False, want_scales=False):
        """EvalPlan of a block the refusals accept, as a dict over EVAL_INTS + EVAL_FLOATS; enumerations by name"""
        ints, floats = (C.c_int * 42)(), (C.c_float * 3)()
        self.lib.hp_plan_eval(C.byref(args), max_frames, int(has_pose_prior), shape_dim, int(has_joint_limits), int(pending),
                              int(assemble), int(window_rows), int(want_betas), int(want_scales), ints, floats)
        out = dict(zip(EVAL_INTS, ints))
        out.update(zip(EVAL_FLOATS, floats))
        for k, names in EVAL_NAMED.items():
            out[k] = names[out[k]]
        return out

    def window_rows_count(self, window, frame_offset, M):
        return self.lib.hp_window_rows_count(window, frame_offset, M)

    # ---- grids of the fit path ----
    def _ints(self, fn, n, *args):
        out = (C.c_int * n)()
        fn(*args, out)
        return tuple(out)

    def xcd_grid(self, blocks_per_frame, M):
        return self.lib.hp_xcd_grid(blocks_per_frame, M)

    def box_grid(self, F, M, joints):
        """(frame blocks, face blocks, joint riders, the launch)"""
        return self._ints(self.lib.hp_box_grid, 4, F, M, int(joints))

    def sweep_grid(self, F, M):
        return self.lib.hp_sweep_grid(F, M)

    def rect_count(self, F):
        return self.lib.hp_rect_count(F)

    def resolve_grid(self, S, M, loss_frames):
        """(tiles per frame, loss riders, the launch)"""
        return self._ints(self.lib.hp_resolve_grid, 3, S, M, loss_frames)

    def raster_bwd_grid(self, F, M):
        return self.lib.hp_raster_bwd_grid(F, M)

    def vertex_bwd_grid(self, Vp, M):
        return self.lib.hp_vertex_bwd_grid(Vp, M)

    def mid_grid(self, M, need_pose):
        """(pose-blend ids, dA ids, the launch)"""
        return self._ints(self.lib.hp_mid_grid, 3, M, int(need_pose))

    def chain_grid(self, M, need_beta, Vp, betas_shared):
        return self.lib.hp_chain_grid(M, int(need_beta), Vp, int(betas_shared))

    def assemble_grid(self, betas_shared, M):
        return self.lib.hp_assemble_grid(int(betas_shared), M)

    def window_rows_grid(self, W):
        return self.lib.hp_window_rows_grid(W)

    def frame_loss_rows_grid(self):
        return self.lib.hp_frame_loss_rows_grid()

    def skin_grid(self, M, Vp):
        return self._ints(self.lib.hp_skin_grid, 2, M, Vp)

    def elem_blocks(self, elements):
        return self.lib.hp_elem_blocks(elements)

    # ---- the other entry points' refusals: the text or None ----
    def refusal(self, name, *args):
        """hp_<name>_refusal(*args); ctypes structures go by reference"""
        why = getattr(self.lib, "hp_%s_refusal" % name)(*[C.byref(a) if isinstance(a, C.Structure) else a for a in args])
        return why.decode() if why else None


def load():
    return Plan(host_shim.build("host_plan_shim.cpp", "host_plan_shim"))


def valid_fit3d_args(**fields):
    """a block smalfit_fit3d_step accepts under FIT3D_FACTS (dummy non-null pointers: nothing dereferences them): two meshes, 20
    betas, chamfer on with points sampled from the targets, every tensor trained at step 1; with `fields` changed"""
    a = _lib.Fit3dArgs()
    a.num_meshes, a.num_betas, a.num_points, a.adam_t = 2, 20, 64, 1
    a.beta1, a.beta2, a.eps = 0.9, 0.999, 1e-8
    a.weights = (C.c_float * 4)(1.0, 1.0, 0.01, 0.1)
    names = [n + t for t in FIT3D_TENSORS for n in ("", "m_", "v_")] + ["losses"]
    for i, name in enumerate(names):
        setattr(a, name, 0x1000 * (i + 1))
    for t in FIT3D_TENSORS:
        setattr(a, "lr_" + t, 0.01)
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def valid_fit_args(**fields):
    """a block smalfit_fit_eval accepts on an engine with both priors set (dummy non-null pointers: nothing dereferences them),
    with `fields` changed"""
    a = _lib.FitArgs()
    a.num_frames, a.window, a.logscale_mode, a.temporal = 4, 2, 1, 1
    a.w_j2d = a.w_sil = a.w_betas = a.w_pose = 1.0
    for i, name in enumerate(("betas", "log_beta_scales", "global_rotation", "joint_rotations", "trans", "target_joints",
                              "target_visibility", "target_sil", "losses")):
        setattr(a, name, 0x1000 * (i + 1))
    for k, v in fields.items():
        setattr(a, k, v)
    return a
