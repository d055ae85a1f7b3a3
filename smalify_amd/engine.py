"""Thin object layer over the C-ABI: device model, workspace engine, typed calls on torch tensors.

PyTorch is plumbing here (HBM allocations, streams); every computation is a HIP kernel in
libsmalfit.so.  All tensors handed to these methods must be contiguous float32 CUDA(HIP) tensors.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import AdamArgs, FitArgs, LbsArgs, ModelDesc, ShardArgs, SmalfitError, check

LOSS_NAMES = ("joint", "pose", "splay", "betas", "sil_reproj", "temp_joint", "temp_global", "temp_trans", "limit")
NUM_LOSS_TERMS = len(LOSS_NAMES)


def _ptr(t):
    if t is None:
        return None
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise SmalfitError("expected a contiguous float32 device tensor, got %r" % (
            (t.dtype, t.device, t.is_contiguous()) if isinstance(t, torch.Tensor) else type(t),))
    return C.c_void_p(t.data_ptr())


def _ptr_u8(t):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()):
        raise SmalfitError("expected a contiguous uint8 device tensor")
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _host(a, dtype):
    return np.ascontiguousarray(np.asarray(a), dtype=dtype)


class DeviceModel:
    """SMAL constants resident in HBM (smalfit_model)."""

    def __init__(self, model_data):
        if not torch.cuda.is_available():
            raise SmalfitError("no HIP device available: smalify_amd has no CPU fallback")
        self.lib = _lib.load()
        md = model_data
        self.data = md
        self.num_verts = int(md.v_template.shape[0])
        self.num_faces = int(md.faces.shape[0])
        self.num_betas = int(md.shapedirs.shape[0])
        keep = dict(vt=_host(md.v_template, np.float32), sd=_host(md.shapedirs, np.float32),
                    pd=_host(md.posedirs, np.float32), jr=_host(md.J_regressor, np.float32),
                    w=_host(md.weights, np.float32), par=_host(md.parents, np.int32),
                    f=_host(md.faces, np.int32))
        desc = ModelDesc(self.num_verts, self.num_faces, self.num_betas,
                         keep["vt"].ctypes.data, keep["sd"].ctypes.data, keep["pd"].ctypes.data,
                         keep["jr"].ctypes.data, keep["w"].ctypes.data, keep["par"].ctypes.data,
                         keep["f"].ctypes.data)
        torch.cuda.init()
        torch.cuda.current_device()
        h = C.c_void_p()
        check(self.lib.smalfit_model_create(C.byref(desc), C.byref(h)), "smalfit_model_create")
        self.handle = h

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.smalfit_model_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class Engine:
    """Workspace for up to `max_frames` frames at `image_size`^2 (smalfit_engine)."""

    def __init__(self, model: DeviceModel, max_frames: int, image_size: int):
        self.lib = model.lib
        self.model = model
        self.max_frames = int(max_frames)
        self.image_size = int(image_size)
        h = C.c_void_p()
        check(self.lib.smalfit_engine_create(model.handle, self.max_frames, self.image_size, C.byref(h)),
              "smalfit_engine_create")
        self.handle = h
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.joint_limits_owner = None      # whoever set the engine's joint-limit table last (None: no table)

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.smalfit_engine_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    # ---- priors ------------------------------------------------------------------------------
    def set_pose_prior(self, prec, mean, mask):
        p, m, k = _host(prec, np.float32), _host(mean, np.float32), _host(mask, np.float32)
        assert p.shape == (105, 105) and m.shape == (105,) and k.shape == (105,)
        check(self.lib.smalfit_engine_set_pose_prior(self.handle, p.ctypes.data, m.ctypes.data, k.ctypes.data),
              "smalfit_engine_set_pose_prior")

    def set_shape_prior(self, prec, mean):
        p, m = _host(prec, np.float32), _host(mean, np.float32)
        assert p.shape == (m.shape[0], m.shape[0])
        check(self.lib.smalfit_engine_set_shape_prior(self.handle, p.ctypes.data, m.ctypes.data, int(m.shape[0])),
              "smalfit_engine_set_shape_prior")
        self.shape_prior_dim = int(m.shape[0])

    def set_graph(self, enable=True):
        """replay one captured iteration per fit_run step (HIP graph) instead of enqueueing its launches one by one"""
        check(self.lib.smalfit_engine_set_graph(self.handle, int(bool(enable))), "smalfit_engine_set_graph")

    OPT_UNCLAMPED_EDGE_T = 1      # SMALFIT_OPT_UNCLAMPED_EDGE_T of include/smalfit.h

    def set_option(self, option, value):
        """engine options (include/smalfit.h): OPT_UNCLAMPED_EDGE_T = 1 selects the silhouette adjoint with the edge parameter left
        unclamped (what some pytorch3d 0.2.x sources are recalled to do); the default 0 is the exact gradient"""
        check(self.lib.smalfit_engine_set_option(self.handle, int(option), int(value)), "smalfit_engine_set_option")

    def clear_joint_limits(self):
        """back to the reference's behaviour: the w_limit column is ignored (its term is commented out upstream)"""
        check(self.lib.smalfit_engine_clear_joint_limits(self.handle), "smalfit_engine_clear_joint_limits")
        self.joint_limits_owner = None

    def set_joint_limits(self, min_values, max_values, owner=None):
        """(34,3) lower / upper limits of the joint rotations for the w_limit term (reference smal_fitter.py:76-79,146-151).
        The table is engine state; `owner` records whose it is, so that a fitter sharing the engine can tell that its table
        was replaced or cleared behind its back and put it back (FusedFitter.assert_joint_limits)."""
        lo, hi = _host(min_values, np.float32).reshape(-1), _host(max_values, np.float32).reshape(-1)
        assert lo.shape == (102,) and hi.shape == (102,)
        check(self.lib.smalfit_engine_set_joint_limits(self.handle, lo.ctypes.data, hi.ctypes.data), "smalfit_engine_set_joint_limits")
        self.joint_limits_owner = owner

    SECTIONS = ("lbs_fwd", "raster_sweep", "raster_select", "raster_bwd", "lbs_bwd", "raster_resolve", "raster_bbox")

    def reset_raster_cache(self):
        """Forget the rasteriser's cached per-pixel depth bounds (affects time only, never results)."""
        check(self.lib.smalfit_engine_reset_raster_cache(self.handle, _stream()), "smalfit_engine_reset_raster_cache")

    def profile_begin(self, max_evals, stride=1):
        """Time the sections of every `stride`-th fit_eval with HIP events on the launch stream (up to max_evals)."""
        check(self.lib.smalfit_engine_profile_begin(self.handle, int(max_evals), int(stride)), "smalfit_engine_profile_begin")

    def profile_end(self):
        """-> {section: (total_ms, count)} measured with HIP events on the current stream."""
        ms = (C.c_float * len(self.SECTIONS))()
        cnt = (C.c_int * len(self.SECTIONS))()
        check(self.lib.smalfit_engine_profile_end(self.handle, _stream(), ms, cnt), "smalfit_engine_profile_end")
        return {n: (float(ms[i]), int(cnt[i])) for i, n in enumerate(self.SECTIONS)}

    def status(self):
        """Synchronises the current stream; returns and clears the sticky status bits."""
        bits = C.c_int(0)
        check(self.lib.smalfit_engine_status(self.handle, _stream(), C.byref(bits)), "smalfit_engine_status")
        return bits.value

    # ---- fused fitter evaluation ---------------------------------------------------------------
    def fit_eval(self, *, betas, log_beta_scales, global_rotation, joint_rotations, trans,
                 target_joints, target_visibility, target_sil, weights, w_temp, window,
                 temporal=True, global_mask=None, rotation_mask=None, halo_prev=None, halo_next=None,
                 losses=None, grads=None, want=("betas", "log_beta_scales", "global_rotation",
                                                "joint_rotations", "trans"),
                 sil_out=None, proj_out=None, verts_out=None, frame_offset=0, total_frames=0,
                 subject_frames=0, losses_per_frame=None):
        """One evaluation of sum_windows SMALFitter.forward + get_temporal and its gradient.

        weights = (w_j2d, w_sil, w_betas, w_pose, w_limit, w_splay) as in the reference's OPT_WEIGHTS columns
        (w_limit > 0 needs set_joint_limits).  target_sil: float32 (M,S,S), or uint8 bytes b = 255 t.
        Returns (losses (9,) device tensor in LOSS_NAMES order, grads dict)."""
        a, losses, grads, _keep = self.build_fit_args(
            betas=betas, log_beta_scales=log_beta_scales, global_rotation=global_rotation,
            joint_rotations=joint_rotations, trans=trans, target_joints=target_joints,
            target_visibility=target_visibility, target_sil=target_sil, weights=weights, w_temp=w_temp, window=window,
            temporal=temporal, global_mask=global_mask, rotation_mask=rotation_mask, halo_prev=halo_prev,
            halo_next=halo_next, losses=losses, grads=grads, want=want, sil_out=sil_out, proj_out=proj_out,
            verts_out=verts_out, frame_offset=frame_offset, total_frames=total_frames,
            subject_frames=subject_frames, losses_per_frame=losses_per_frame)
        check(self.lib.smalfit_fit_eval(self.handle, _stream(), C.byref(a)), "smalfit_fit_eval")
        return losses, grads

    @staticmethod
    def num_windows(num_frames, window, frame_offset=0):
        """windows of the sequence that hold at least one of the frames [frame_offset, frame_offset + num_frames)"""
        return (frame_offset + num_frames - 1) // window - frame_offset // window + 1

    def fit_eval_windows(self, *, window_losses=None, window_grads=None, **fit):
        """fit_eval (same arguments) that also hands out every window's share (smalfit_fit_eval_windows; reference
        smal_fitter.py:107-175 called per window, optimize_to_joints.py:119-122): row w of window_losses (W, 9) holds the nine
        terms of window w's frames, row w of window_grads["betas"] (W, 20) / ["log_beta_scales"] (W, 6) the gradient of that
        row's total with respect to the shared parameter.  Rows are formed for the shared tensors named in `want`
        (log_beta_scales only when it is shared, (6,)); the caller may pass the buffers.
        Returns (losses (9,), grads, window_losses, window_grads)."""
        fn = _lib.resolve(self.lib, "smalfit_fit_eval_windows")
        a, losses, grads, _keep = self.build_fit_args(**fit)
        if a.window <= 0 or a.frame_offset < 0:
            raise SmalfitError("window must be positive and frame_offset >= 0")
        W = self.num_windows(a.num_frames, a.window, a.frame_offset)
        dev = fit["global_rotation"].device

        def rows(t, cols, what):
            # the library cannot know the extent of a device pointer
            if t is None:
                return torch.empty(W, cols, device=dev, dtype=torch.float32)
            if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (W, cols)):
                raise SmalfitError("%s must be a contiguous float32 tensor of (%d, %d): one row per window" % (what, W, cols))
            return t

        window_losses = rows(window_losses, NUM_LOSS_TERMS, "window_losses")
        given = dict(window_grads) if window_grads is not None else {}
        unknown = set(given) - {"betas", "log_beta_scales"}
        if unknown:
            raise SmalfitError("window_grads takes 'betas' and 'log_beta_scales', not %s" % sorted(unknown))
        want = fit.get("want", ("betas", "log_beta_scales"))
        out = {}
        if "betas" in want or "betas" in given:
            out["betas"] = rows(given.get("betas"), 20, "window_grads['betas']")
        if a.logscale_mode == 1 and ("log_beta_scales" in want or "log_beta_scales" in given):
            out["log_beta_scales"] = rows(given.get("log_beta_scales"), 6, "window_grads['log_beta_scales']")
        elif "log_beta_scales" in given:
            raise SmalfitError("window_grads['log_beta_scales'] needs shared log_beta_scales of (6,)")
        r = _lib.WindowRows()
        r.num_windows = W
        r.losses, r.g_betas, r.g_log_beta_scales = _ptr(window_losses), _ptr(out.get("betas")), _ptr(out.get("log_beta_scales"))
        check(fn(self.handle, _stream(), C.byref(a), C.byref(r)), "smalfit_fit_eval_windows")
        return losses, grads, window_losses, out

    def build_fit_args(self, *, betas, log_beta_scales, global_rotation, joint_rotations, trans,
                       target_joints, target_visibility, target_sil, weights, w_temp, window,
                       temporal=True, global_mask=None, rotation_mask=None, halo_prev=None, halo_next=None,
                       losses=None, grads=None, want=("betas", "log_beta_scales", "global_rotation",
                                                      "joint_rotations", "trans"),
                       sil_out=None, proj_out=None, verts_out=None, frame_offset=0, total_frames=0,
                       subject_frames=0, losses_per_frame=None):
        """-> (smalfit_fit_args, losses, grads, keep-alive list): the argument block of smalfit_fit_eval / smalfit_fit_run.
        The block holds raw device pointers: the caller keeps the tensors alive for as long as it uses it.
        subject_frames=1: every frame is an unrelated image with its own betas (M,20) (and limb scales (M,6));
        losses_per_frame: an (M, 9) float32 tensor that receives each frame's share of the loss terms."""
        M = int(global_rotation.shape[0])
        w_j2d, w_sil, w_betas, w_pose, w_limit, w_splay = [float(w) for w in weights]
        dev = global_rotation.device
        if losses is None:
            losses = torch.empty(NUM_LOSS_TERMS, device=dev, dtype=torch.float32)
        elif losses.numel() < NUM_LOSS_TERMS:
            raise SmalfitError("losses must hold %d floats" % NUM_LOSS_TERMS)
        if grads is None:
            grads = {}
        params = dict(betas=betas, log_beta_scales=log_beta_scales, global_rotation=global_rotation,
                      joint_rotations=joint_rotations, trans=trans)
        for k in want:
            if k not in grads and params[k] is not None:
                grads[k] = torch.empty_like(params[k])
        if log_beta_scales is None:
            mode = 0
        elif log_beta_scales.dim() == 1:
            mode = 1
        else:
            mode = 2
        a = FitArgs()
        a.num_frames, a.window, a.logscale_mode, a.temporal = M, int(window), mode, int(bool(temporal))
        a.shape_prior_dim = 0
        # where these M frames sit in their sequence (shards; zeros = they are the whole sequence)
        a.frame_offset, a.total_frames = int(frame_offset), int(total_frames)
        a.subject_frames = int(subject_frames)
        if a.subject_frames == 1:
            # the library cannot know the extent of a device pointer: the usual (20,) betas here would be read M * 20 floats far
            if betas is None or betas.numel() != M * 20:
                raise SmalfitError("subject_frames=1 takes betas of (num_frames, 20): one shape per image")
            if log_beta_scales is not None and log_beta_scales.dim() != 1 and log_beta_scales.numel() != M * 6:
                raise SmalfitError("subject_frames=1 takes log_beta_scales of (num_frames, 6), or None")   # ((6,) = shared: the library refuses it)
            for k in ("betas", "log_beta_scales"):
                if k in want and grads.get(k) is not None and params[k] is not None and grads[k].numel() != params[k].numel():
                    raise SmalfitError("subject_frames=1: the gradient buffer of %s must have its shape" % k)
        if losses_per_frame is not None and (losses_per_frame.dtype != torch.float32 or not losses_per_frame.is_contiguous()
                                             or losses_per_frame.numel() < M * NUM_LOSS_TERMS):
            raise SmalfitError("losses_per_frame must be a contiguous float32 tensor of (num_frames, %d)" % NUM_LOSS_TERMS)
        a.losses_per_frame = _ptr(losses_per_frame)
        a.w_j2d, a.w_sil, a.w_betas, a.w_pose, a.w_splay, a.w_temp = w_j2d, w_sil, w_betas, w_pose, w_splay, float(w_temp)
        a.betas, a.log_beta_scales = _ptr(betas), _ptr(log_beta_scales)
        a.global_rotation, a.joint_rotations, a.trans = _ptr(global_rotation), _ptr(joint_rotations), _ptr(trans)
        a.global_mask, a.rotation_mask = _ptr(global_mask), _ptr(rotation_mask)
        a.target_joints, a.target_visibility = _ptr(target_joints), _ptr(target_visibility)
        if target_sil is not None and target_sil.dtype == torch.uint8:
            a.target_sil, a.target_sil_u8 = None, _ptr_u8(target_sil)
        else:
            a.target_sil, a.target_sil_u8 = _ptr(target_sil), None
        a.w_limit = w_limit
        a.halo_prev, a.halo_next = _ptr(halo_prev), _ptr(halo_next)
        a.losses = _ptr(losses)
        a.g_betas = _ptr(grads.get("betas")) if "betas" in want else None
        a.g_log_beta_scales = _ptr(grads.get("log_beta_scales")) if "log_beta_scales" in want else None
        a.g_global_rotation = _ptr(grads.get("global_rotation")) if "global_rotation" in want else None
        a.g_joint_rotations = _ptr(grads.get("joint_rotations")) if "joint_rotations" in want else None
        a.g_trans = _ptr(grads.get("trans")) if "trans" in want else None
        a.sil_out, a.proj_out, a.verts_out = _ptr(sil_out), _ptr(proj_out), _ptr(verts_out)
        keep = [betas, log_beta_scales, global_rotation, joint_rotations, trans, target_joints, target_visibility,
                target_sil, global_mask, rotation_mask, halo_prev, halo_next, losses, grads, sil_out, proj_out, verts_out,
                losses_per_frame]
        return a, losses, grads, keep

    def fit_run(self, fit_args, adam_args, iterations):
        """`iterations` x (evaluation + backward + Adam step) in one call (smalfit_fit_run; reference
        optimize_to_joints.py:113-137).  Advances adam_args.step."""
        check(self.lib.smalfit_fit_run(self.handle, _stream(), C.byref(fit_args), C.byref(adam_args), int(iterations)),
              "smalfit_fit_run")
        adam_args.step += int(iterations)

    # ---- SMAL.__call__ ---------------------------------------------------------------------------
    def lbs_forward(self, beta, theta, logscale=None, want_Rs=True, want_v_shaped=True, v_offset=None):
        """SMAL.__call__ (smalfit_lbs_forward_ex): theta (M,35,3) axis-angles or (M,35,3,3) rotation matrices; v_offset (M,V,3)
        is the reference's del_v (+ a per-call v_template's difference to the model's)"""
        M, nb = int(theta.shape[0]), int(beta.shape[1])
        V = self.model.num_verts
        dev = theta.device
        verts = torch.empty(M, V, 3, device=dev)
        joints = torch.empty(M, 41, 3, device=dev)
        Rs = torch.empty(M, 35, 3, 3, device=dev) if want_Rs else None
        vs = torch.empty(M, V, 3, device=dev) if want_v_shaped else None
        a = LbsArgs()
        a.num_frames, a.num_betas = M, nb
        a.beta, a.logscale, a.v_offset = _ptr(beta), _ptr(logscale), _ptr(v_offset)
        if theta.dim() == 4:
            a.Rs = _ptr(theta)
        else:
            a.theta = _ptr(theta)
        a.verts, a.joints, a.Rs_out, a.v_shaped = _ptr(verts), _ptr(joints), _ptr(Rs), _ptr(vs)
        check(self.lib.smalfit_lbs_forward_ex(self.handle, _stream(), C.byref(a)), "smalfit_lbs_forward_ex")
        return verts, joints, Rs, vs

    def lbs_backward(self, beta, theta, logscale, dverts, djoints, v_offset=None):
        """-> (dbeta, dtheta (or dRs for matrix input), dlogscale) and, when v_offset is given, dv_offset as a 4th value"""
        M, nb = int(theta.shape[0]), int(beta.shape[1])
        dev = theta.device
        dbeta = torch.empty(M, nb, device=dev)
        dth = torch.empty_like(theta)
        dls = torch.empty(M, 6, device=dev) if logscale is not None else None
        doff = torch.empty_like(v_offset) if v_offset is not None else None
        a = LbsArgs()
        a.num_frames, a.num_betas = M, nb
        a.beta, a.logscale, a.v_offset = _ptr(beta), _ptr(logscale), _ptr(v_offset)
        if theta.dim() == 4:
            a.Rs, a.dRs = _ptr(theta), _ptr(dth)
        else:
            a.theta, a.dtheta = _ptr(theta), _ptr(dth)
        a.dverts, a.djoints = _ptr(dverts), _ptr(djoints)
        a.dbeta, a.dlogscale, a.dv_offset = _ptr(dbeta), _ptr(dls), _ptr(doff)
        check(self.lib.smalfit_lbs_backward_ex(self.handle, _stream(), C.byref(a)), "smalfit_lbs_backward_ex")
        if v_offset is not None:
            return dbeta, dth, dls, doff
        return dbeta, dth, dls

    # ---- Renderer -----------------------------------------------------------------------------------
    def render_forward(self, verts, points=None, want_sil=True):
        M = int(verts.shape[0])
        S = self.image_size
        sil = torch.empty(M, S, S, device=verts.device) if want_sil else None
        proj = None
        P = 0
        if points is not None:
            P = int(points.shape[1])
            proj = torch.empty(M, P, 2, device=verts.device)
        check(self.lib.smalfit_render_forward(self.handle, _stream(), M, _ptr(verts), _ptr(points), P, _ptr(sil),
                                              _ptr(proj)), "smalfit_render_forward")
        return sil, proj

    def render_color(self, verts, rgb):
        """Hard-Phong colour render (visualisation, no gradient): verts (M,V,3) world incl. translation, rgb 3 floats in
        [0,1] -> (M,3,S,S)."""
        M = int(verts.shape[0])
        S = self.image_size
        image = torch.empty(M, 3, S, S, device=verts.device)
        col = np.ascontiguousarray(np.asarray(rgb, dtype=np.float32).reshape(3))
        check(self.lib.smalfit_render_color(self.handle, _stream(), M, _ptr(verts), col.ctypes.data, _ptr(image)),
              "smalfit_render_color")
        return image

    def fit_metrics(self, verts, target_sil, proj_joints=None, target_joints=None, target_visibility=None,
                    thresholds=(0.15,), want_mask=False):
        """How good a fit is, per frame (smalfit_fit_metrics; the definitions are this project's, include/smalfit.h).
        verts (M,V,3) with the translation applied and proj_joints (M,25,2): verts_out / proj_out of an evaluation;
        target_sil (M,S,S) float32 (on above 0.5) or uint8 (on from 128); keypoints: all three tensors or none.
        -> dict of device tensors: sil_counts (M,4) int32 = pixels in [rendered & target, rendered | target, rendered, target]
        (the hard render: covered exactly where render_color is not white); with keypoints keypoint_dist (M,25) = distance /
        sqrt(target pixels) of every keypoint (+inf where the target is empty) and pck_counts (M,1+T) int32 = visible
        keypoints, then those within thresholds[t]; with want_mask the hard coverage mask (M,S,S) uint8.  No quotient is
        formed on the device: smalify_amd.metrics.summarise turns the counts into IoU and PCK."""
        fn = _lib.resolve(self.lib, "smalfit_fit_metrics")
        M, S, V = int(verts.shape[0]), self.image_size, self.model.num_verts
        if tuple(verts.shape) != (M, V, 3):
            raise SmalfitError("verts must be (num_frames, %d, 3)" % V)
        # the library cannot know the extent, the element type or the device of a pointer
        if not (isinstance(target_sil, torch.Tensor) and tuple(target_sil.shape) == (M, S, S)
                and target_sil.dtype in (torch.float32, torch.uint8)):
            raise SmalfitError("target_sil must be a (num_frames, %d, %d) tensor of float32 or uint8" % (S, S))
        kp = (proj_joints, target_joints, target_visibility)
        for t, shape in zip(kp, ((M, 25, 2), (M, 25, 2), (M, 25))):
            if t is not None and not (isinstance(t, torch.Tensor) and tuple(t.shape) == shape):
                raise SmalfitError("keypoint tensors must be (num_frames,25,2), (num_frames,25,2) and (num_frames,25)")
        for t in (target_sil,) + kp:
            if t is not None and t.device != verts.device:
                raise SmalfitError("target_sil and the keypoint tensors must be on the device of verts (%s)" % verts.device)
        thr = [float(t) for t in thresholds]
        if len(thr) > _lib.MAX_PCK_THRESHOLDS:
            raise SmalfitError("at most %d thresholds" % _lib.MAX_PCK_THRESHOLDS)
        dev = verts.device
        have_kp = all(t is not None for t in kp)
        out = {"sil_counts": torch.empty(M, 4, dtype=torch.int32, device=dev)}
        if have_kp:
            out["keypoint_dist"] = torch.empty(M, 25, device=dev)
            out["pck_counts"] = torch.empty(M, 1 + len(thr), dtype=torch.int32, device=dev)
        if want_mask:
            out["mask"] = torch.empty(M, S, S, dtype=torch.uint8, device=dev)
        a = _lib.MetricsArgs()
        a.num_frames, a.verts = M, _ptr(verts)
        if target_sil.dtype == torch.uint8:
            a.target_sil_u8 = _ptr_u8(target_sil)
        else:
            a.target_sil = _ptr(target_sil)
        a.sil_counts = C.c_void_p(out["sil_counts"].data_ptr())
        a.mask_out = C.c_void_p(out["mask"].data_ptr()) if want_mask else None
        a.proj_joints, a.target_joints, a.target_visibility = _ptr(proj_joints), _ptr(target_joints), _ptr(target_visibility)
        a.num_thresholds = len(thr)
        for i, t in enumerate(thr):
            a.thresholds[i] = t
        if have_kp:
            a.keypoint_dist = _ptr(out["keypoint_dist"])
            a.pck_counts = C.c_void_p(out["pck_counts"].data_ptr())
        check(fn(self.handle, _stream(), C.byref(a)), "smalfit_fit_metrics")
        return out

    def render_backward(self, verts, sil, dsil):
        dverts = torch.empty_like(verts)
        check(self.lib.smalfit_render_backward(self.handle, _stream(), int(verts.shape[0]), _ptr(verts), _ptr(sil),
                                               _ptr(dsil), _ptr(dverts)), "smalfit_render_backward")
        return dverts

    def face_list_lengths(self, M):
        """(M, F) uint8: per face the length of the candidate list the last silhouette forward handed to the backward gather
        (0..128), 254 = candidate masks, 255 = the whole box is walked (diagnostics; results never depend on the form)"""
        out = torch.empty(int(M), self.model.num_faces, dtype=torch.uint8, device="cuda")
        check(self.lib.smalfit_engine_face_list_lengths(self.handle, _stream(), int(M), _ptr_u8(out)),
              "smalfit_engine_face_list_lengths")
        return out

    def project_points_backward(self, points, dproj):
        dpoints = torch.empty_like(points)
        count = int(points.numel() // 3)
        check(self.lib.smalfit_project_points_backward(_stream(), count, self.image_size, _ptr(points), _ptr(dproj),
                                                       _ptr(dpoints)), "smalfit_project_points_backward")
        return dpoints


def pose_prior(engine, x):
    N = int(x.shape[0])
    out = torch.empty(N, 105, device=x.device)
    check(engine.lib.smalfit_pose_prior(engine.handle, _stream(), N, _ptr(x), _ptr(out)), "smalfit_pose_prior")
    return out


def pose_prior_backward(engine, x, dout):
    N = int(x.shape[0])
    dx = torch.empty(N, 105, device=x.device)
    check(engine.lib.smalfit_pose_prior_backward(engine.handle, _stream(), N, _ptr(x), _ptr(dout), _ptr(dx)),
          "smalfit_pose_prior_backward")
    return dx


def temporal(engine, w_temp, global_rotation, joint_rotations, trans, global_mask=None, rotation_mask=None):
    """-> (losses (3,) joint/global/trans, g_global_rotation, g_joint_rotations, g_trans)"""
    N = int(global_rotation.shape[0])
    losses = torch.empty(3, device=trans.device)
    gg, gj, gt = torch.empty_like(global_rotation), torch.empty_like(joint_rotations), torch.empty_like(trans)
    check(engine.lib.smalfit_temporal(engine.handle, _stream(), N, float(w_temp), _ptr(global_rotation),
                                      _ptr(joint_rotations), _ptr(trans), _ptr(global_mask), _ptr(rotation_mask),
                                      _ptr(losses), _ptr(gg), _ptr(gj), _ptr(gt)), "smalfit_temporal")
    return losses, gg, gj, gt


def rodrigues(theta):
    lib = _lib.load()
    count = int(theta.shape[0])
    R = torch.empty(count, 3, 3, device=theta.device)
    check(lib.smalfit_rodrigues(_stream(), count, _ptr(theta), _ptr(R)), "smalfit_rodrigues")
    return R


def rodrigues_backward(theta, dR):
    lib = _lib.load()
    count = int(theta.shape[0])
    dth = torch.empty_like(theta)
    check(lib.smalfit_rodrigues_backward(_stream(), count, _ptr(theta), _ptr(dR), _ptr(dth)), "smalfit_rodrigues_backward")
    return dth


def global_rigid_transformation(Rs, Js, parents, logscale=None):
    """Rs (N,35,3,3), Js (N,35,3), parents (35,) host ints, logscale (N,6) or None -> new_J (N,35,3), A (N,35,4,4)
    (reference batch_lbs.py:75-170; adjoint: global_rigid_transformation_backward)"""
    lib = _lib.load()
    N = int(Rs.shape[0])
    if tuple(Rs.shape) != (N, 35, 3, 3) or tuple(Js.shape) != (N, 35, 3):
        raise SmalfitError("Rs must be (N,35,3,3) and Js (N,35,3)")
    if logscale is not None and tuple(logscale.shape) != (N, 6):
        raise SmalfitError("betas_logscale must be (N,6)")
    par = _host(parents, np.int32).reshape(-1)
    if par.shape[0] != 35:
        raise SmalfitError("parents must hold 35 entries")
    new_J = torch.empty(N, 35, 3, device=Rs.device)
    A = torch.empty(N, 35, 4, 4, device=Rs.device)
    check(lib.smalfit_global_rigid_transformation(_stream(), N, _ptr(Rs), _ptr(Js), par.ctypes.data, _ptr(logscale),
                                                  _ptr(new_J), _ptr(A)), "smalfit_global_rigid_transformation")
    return new_J, A


def global_rigid_transformation_backward(Rs, Js, parents, logscale, d_new_J, d_A):
    """adjoint of global_rigid_transformation -> (dRs (N,35,3,3), dJs (N,35,3), dlogscale (N,6) or None)"""
    lib = _lib.load()
    N = int(Rs.shape[0])
    par = _host(parents, np.int32).reshape(-1)
    dRs, dJs = torch.empty_like(Rs), torch.empty_like(Js)
    dls = torch.empty_like(logscale) if logscale is not None else None
    scratch = torch.empty(N * 840, device=Rs.device)
    check(lib.smalfit_global_rigid_transformation_backward(_stream(), N, _ptr(Rs), _ptr(Js), par.ctypes.data, _ptr(logscale),
                                                           _ptr(d_new_J), _ptr(d_A), _ptr(scratch), _ptr(dRs), _ptr(dJs),
                                                           _ptr(dls)), "smalfit_global_rigid_transformation_backward")
    return dRs, dJs, dls


def adam_step(param, grad, exp_avg, exp_avg_sq, lr, t, beta1=0.5, beta2=0.999, eps=1e-8):
    """In-place torch.optim.Adam step on a flat float32 device tensor (reference optimize_to_joints.py:96,137)."""
    lib = _lib.load()
    check(lib.smalfit_adam_step(_stream(), int(param.numel()), _ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq),
                                float(lr), float(beta1), float(beta2), float(eps), int(t)), "smalfit_adam_step")


def make_adam_args(param, grad, exp_avg, exp_avg_sq, segments, lr, step=0, beta1=0.5, beta2=0.999, eps=1e-8):
    """smalfit_adam_args over flat float32 device tensors; segments = [(begin, end), ...] (at most 4)"""
    if len(segments) > 4:
        raise SmalfitError("at most 4 trainable ranges")
    a = AdamArgs()
    a.param, a.grad, a.exp_avg, a.exp_avg_sq = _ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq)
    a.num_segments = len(segments)
    for k, (b, e) in enumerate(segments):
        a.seg_begin[k], a.seg_end[k] = int(b), int(e)
    a.lr, a.beta1, a.beta2, a.eps, a.step = float(lr), float(beta1), float(beta2), float(eps), int(step)
    return a


def adam_segments(adam_args):
    """one fused Adam launch over the ranges (t = step + 1); advances adam_args.step"""
    check(_lib.load().smalfit_adam_segments(_stream(), C.byref(adam_args)), "smalfit_adam_segments")
    adam_args.step += 1


def shard_record(num_shared, shared_grad, num_frames, global_rotation, joint_rotations, trans, global_mask, rotation_mask, record):
    check(_lib.load().smalfit_shard_record(_stream(), int(num_shared), _ptr(shared_grad), int(num_frames), _ptr(global_rotation),
                                           _ptr(joint_rotations), _ptr(trans), _ptr(global_mask), _ptr(rotation_mask),
                                           _ptr(record)), "smalfit_shard_record")


def shard_local_step(engine, fit_args, adam_args, num_shared, shared_grad, record):
    """evaluation + Adam on the per-frame ranges + this rank's record, one library call (smalfit_shard_local_step); does not
    advance adam_args.step (shard_reduce_step closes the iteration)"""
    check(engine.lib.smalfit_shard_local_step(engine.handle, _stream(), C.byref(fit_args), C.byref(adam_args), int(num_shared),
                                              _ptr(shared_grad), _ptr(record)), "smalfit_shard_local_step")


def shard_run(engine, fit_args, adam_local, adam_shared, shard_args, iterations):
    """`iterations` x [evaluation + per-frame Adam + record -> all-gather -> rank-ordered sum + shared Adam] in ONE library call
    (smalfit_shard_run); advances both step counts"""
    check(engine.lib.smalfit_shard_run(engine.handle, _stream(), C.byref(fit_args), C.byref(adam_local), C.byref(adam_shared),
                                       C.byref(shard_args), int(iterations)), "smalfit_shard_run")
    adam_local.step += int(iterations)
    adam_shared.step += int(iterations)


def shard_reduce_step(world_size, record_stride, gathered, num_shared, num_trainable, adam_args):
    """sum of the gathered partial shape gradients (rank order) + Adam on the first num_trainable shared parameters;
    does not advance adam_args.step (the caller does, once per iteration)"""
    check(_lib.load().smalfit_shard_reduce_step(_stream(), int(world_size), int(record_stride), _ptr(gathered), int(num_shared),
                                                int(num_trainable), C.byref(adam_args)), "smalfit_shard_reduce_step")


# ---- fitter_3d: SMAL-to-mesh objective ------------------------------------------------------
MESH_LOSS_NAMES = ("chamfer", "edge", "normal", "laplacian", "total")


class MeshObjective:
    """Chamfer + edge + normal-consistency + uniform-Laplacian objective of N deforming meshes of one topology and its
    gradient (smalfit_mesh_objective; reference fitter_3d/trainer.py:205-227 + the PyTorch3D v0.2.5 losses)."""

    def __init__(self, num_verts, faces, max_meshes, max_points):
        if not torch.cuda.is_available():
            raise SmalfitError("no HIP device available: smalify_amd has no CPU fallback")
        self.lib = _lib.load()
        f = _host(faces, np.int32).reshape(-1, 3)
        self.num_verts, self.num_faces = int(num_verts), int(f.shape[0])
        self.max_meshes, self.max_points = int(max_meshes), int(max_points)
        torch.cuda.init()
        torch.cuda.current_device()
        h = C.c_void_p()
        check(self.lib.smalfit_mesh_objective_create(self.num_verts, self.num_faces, f.ctypes.data, self.max_meshes,
                                                     self.max_points, C.byref(h)), "smalfit_mesh_objective_create")
        self.handle = h
        ne, npairs = C.c_int(), C.c_int()
        check(self.lib.smalfit_mesh_objective_counts(h, C.byref(ne), C.byref(npairs)), "smalfit_mesh_objective_counts")
        self.num_edges, self.num_face_pairs = ne.value, npairs.value

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.smalfit_mesh_objective_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def eval(self, lbs_verts, trans, deform_verts, points, weights, out=None, chamfer_gates=None, point_normals=None,
             point_boundary=None, targets=None, robust=None):
        """-> dict(losses (5,), verts (N,V,3), dverts (N,V,3), dtrans (N,3)); `weights` = (w_chamfer, w_edge, w_normal,
        w_laplacian) host floats; `out` may carry preallocated tensors under the same keys.
        chamfer_gates: None, or a dict of max_dist_point, max_dist_vert, min_cos_point, min_cos_vert, reject_boundary
        (chamfer_gates(); smalfit_mesh_objective_eval_gated, include/smalfit.h): which chamfer matches count on a partial scan.  A
        min_cos gate needs point_normals (N,S,3), reject_boundary point_boundary (N,S) uint8 (MeshTargets.sample_attrs).  Adds
        kept (N,2) int32 = kept points | kept vertices and, while w_chamfer > 0 and some gate is on, point_kept (N,S) / vert_kept (N,V) uint8 and
        point_nn (N,S) / vert_nn (N,V) int32 (-1: dropped point / no compatible point found).
        robust: None, or a dict of sigma_chamfer_point, sigma_chamfer_vert (robust(); smalfit_mesh_objective_eval_robust): the
        Geman-McClure kernel on the kept matches; the surface scales of the dict are not read here.  Adds chamfer_weight_sums
        (N,2) = sum of w over the kept points | kept vertices and, for a direction whose scale is on, point_weights (N,S) /
        vert_weights (N,V); losses[0] and losses[4] then carry the robust values.  With chamfer_gates None no gate block is passed."""
        N, V = int(lbs_verts.shape[0]), self.num_verts
        if tuple(lbs_verts.shape) != (N, V, 3) or tuple(trans.shape) != (N, 3):
            raise SmalfitError("lbs_verts must be (N,%d,3) and trans (N,3)" % V)
        if deform_verts is not None and tuple(deform_verts.shape) != (N, V, 3):
            raise SmalfitError("deform_verts must be (N,%d,3)" % V)
        S = 0
        if points is not None:
            if points.dim() != 3 or int(points.shape[0]) != N or int(points.shape[2]) != 3:
                raise SmalfitError("points must be (N,S,3)")
            S = int(points.shape[1])
        dev = lbs_verts.device
        o = out if out is not None else {}
        for k, shape in (("losses", (5,)), ("verts", (N, V, 3)), ("dverts", (N, V, 3)), ("dtrans", (N, 3))):
            _out_tensor(o, k, shape, torch.float32, dev)
        w = _host(weights, np.float32).reshape(4)
        on = float(w[0]) > 0 and S > 0
        # the blocks that are on, each with its outputs attached
        g = rb = None
        if robust is not None:
            rd = _robust_of(robust)
            rb = robust_block(rd)
            outs = (("chamfer_weight_sums", "chamfer_weight_sums", (N, 2)),)
            if on and _scale_on(rd["sigma_chamfer_point"]):
                outs += (("point_weights", "chamfer_point_weights", (N, S)),)
            if on and _scale_on(rd["sigma_chamfer_vert"]):
                outs += (("vert_weights", "chamfer_vert_weights", (N, V)),)
            for k, field, shape in outs:
                setattr(rb, field, _ptr(_out_tensor(o, k, shape, torch.float32, dev, zero=True)))
        if chamfer_gates is not None:
            chamfer_gates_dict = _chamfer_gates_of(chamfer_gates)
            g = chamfer_gate_block(chamfer_gates_dict)
            if point_normals is not None:
                if tuple(point_normals.shape) != (N, S, 3) or point_normals.device != dev or point_normals.dtype != torch.float32:
                    raise SmalfitError("point_normals must be float32 (N, S, 3) on the device of lbs_verts")
                g.point_normals = _ptr(point_normals)
            if point_boundary is not None:
                if tuple(point_boundary.shape) != (N, S) or point_boundary.device != dev or point_boundary.dtype != torch.uint8:
                    raise SmalfitError("point_boundary must be uint8 (N, S) on the device of lbs_verts")
                g.point_boundary = C.c_void_p(point_boundary.data_ptr())
            masks = (("point_kept", (N, S), torch.uint8), ("vert_kept", (N, V), torch.uint8), ("point_nn", (N, S), torch.int32),
                     ("vert_nn", (N, V), torch.int32)) if on and chamfer_gates_on(chamfer_gates_dict) else ()
            for k, shape, dt in (("kept", (N, 2), torch.int32),) + masks:
                setattr(g, k, C.c_void_p(_out_tensor(o, k, shape, dt, dev, zero=True).data_ptr()))
        # one call, through the narrowest entry point whose signature holds the last block that is on
        name, blocks = _narrowest(_EVAL_ENTRY_POINTS, g, rb)
        tail = ()
        if blocks:
            targets = getattr(targets, "_dev", targets)
            tail = (targets.handle if targets is not None else None,) + _refs(blocks)
        check(_lib.resolve(self.lib, name)(self.handle, _stream(), N, _ptr(lbs_verts), _ptr(trans), _ptr(deform_verts), _ptr(points), S,
                                           w.ctypes.data, _ptr(o["verts"]), _ptr(o["losses"]), _ptr(o["dverts"]), _ptr(o["dtrans"]),
                                           *tail), name)
        return o

    def score(self, verts, targets, points=None, thresholds=()):
        """How good a 3-D fit is, per mesh (smalfit_mesh_score; the definitions are this project's, include/smalfit.h).
        verts (N,V,3): the fitted vertices (verts of eval / a Stage's forward); targets: the MeshTargets (or a TargetMeshes)
        the meshes were fitted to, one per mesh; points (N,S,3), S <= max_points: points ON the target surfaces
        (MeshTargets.sample), or None for one direction only; thresholds: up to 8 distances in the model's units.
        -> dict of device tensors: vert_dist (N,V) = exact distance from every fitted vertex to the target's surface, with
        points point_dist (N,S) = from every point to the fitted surface, sums (N,2,3) = per direction sum d, sum d^2, max d
        (direction 1 zero without points), with thresholds within (N,2,T) int32 = queries with d <= thresholds[t].  No
        quotient is formed on the device: smalify_amd.metrics.summarise_mesh_score turns these into mean, RMS, Hausdorff,
        chamfer and F-score."""
        fn = _lib.resolve(self.lib, "smalfit_mesh_score")
        targets = getattr(targets, "_dev", targets)
        if not isinstance(targets, MeshTargets):
            raise SmalfitError("targets must be the MeshTargets the meshes were fitted to")
        N, V = int(verts.shape[0]), self.num_verts
        if tuple(verts.shape) != (N, V, 3):
            raise SmalfitError("verts must be (num_meshes, %d, 3)" % V)
        S = 0
        if points is not None:
            # the library cannot know the extent or the device of a pointer
            if not (isinstance(points, torch.Tensor) and points.dim() == 3 and int(points.shape[0]) == N and int(points.shape[2]) == 3):
                raise SmalfitError("points must be (num_meshes, S, 3)")
            if points.device != verts.device:
                raise SmalfitError("points must be on the device of verts (%s)" % verts.device)
            S = int(points.shape[1])
        thr = [float(t) for t in thresholds]
        if len(thr) > _lib.MAX_SCORE_THRESHOLDS:
            raise SmalfitError("at most %d thresholds" % _lib.MAX_SCORE_THRESHOLDS)
        a = _lib.MeshScoreArgs()
        a.num_meshes, a.verts, a.points, a.num_points = N, _ptr(verts), _ptr(points), S
        a.num_thresholds = len(thr)
        for i, t in enumerate(thr):
            a.thresholds[i] = t
        dev = verts.device
        out = {"vert_dist": torch.empty(N, V, device=dev), "sums": torch.empty(N, 2, 3, device=dev)}
        if points is not None:
            out["point_dist"] = torch.empty(N, S, device=dev)
        if thr:
            out["within"] = torch.empty(N, 2, len(thr), dtype=torch.int32, device=dev)
            a.within = C.c_void_p(out["within"].data_ptr())
        a.vert_dist, a.point_dist, a.sums = _ptr(out["vert_dist"]), _ptr(out.get("point_dist")), _ptr(out["sums"])
        check(fn(self.handle, targets.handle, _stream(), C.byref(a)), "smalfit_mesh_score")
        return out

    def surface(self, verts, targets, points, w_point_surface, w_vert_surface, correspondences=False, gates=None,
                point_normals=None, robust=None):
        """The point-to-surface term both ways and its gradient (smalfit_mesh_surface_eval; the definition is this project's,
        include/smalfit.h): L_ps = mean over the points of d^2(point, fitted surface), L_vs = mean over the fitted vertices of
        d^2(vertex, target surface), term = w_point_surface L_ps + w_vert_surface L_vs; a weight <= 0 skips its direction.
        verts (N,V,3); targets: the MeshTargets (or a TargetMeshes), may be None when w_vert_surface <= 0; points (N,S,3) on
        the target surfaces, may be None when w_point_surface <= 0.
        -> dict of device tensors: losses (3,) = L_ps, L_vs, term; rows (N,2) = per mesh sum d^2 of the points | the vertices;
        dverts (N,V,3), dtrans (N,3) = the term's gradient; with correspondences, for every direction that ran, point_face (N,S)
        int32 / point_bary (N,S,3) on the fitted topology and vert_face (N,V) / vert_bary (N,V,3) on target mesh n, each with its
        residual (point_residual, vert_residual: the query minus its closest point, as the gradient uses it).
        gates: None, or a dict of max_dist_point, max_dist_vert, min_cos_point, min_cos_vert, reject_boundary (surface_gates();
        smalfit_mesh_surface_eval_gated): which matches count on a partial scan.  min_cos_point needs point_normals (N,S,3), the
        unit normals of the points (MeshTargets.sample_normals).  Adds kept (N,2) int32 = kept points | kept vertices, and for
        every direction that ran point_kept (N,S) / vert_kept (N,V) uint8; vert_normals (N,V,3) when min_cos_vert is on.
        robust: None, or a dict of sigma_surface_point, sigma_surface_vert (robust(); smalfit_mesh_surface_eval_robust): the
        Geman-McClure kernel on the kept matches; the chamfer scales of the dict are not read here.  Adds surface_weight_sums
        (N,2) and, for a direction that ran with its scale on, point_weights (N,S) / vert_weights (N,V); losses, rows and the
        gradient then carry the robust values, the residuals stay geometric."""
        fn = _lib.resolve(self.lib, _narrowest(_SURFACE_ENTRY_POINTS, gates, robust)[0])
        targets = getattr(targets, "_dev", targets)
        if targets is not None and not isinstance(targets, MeshTargets):
            raise SmalfitError("targets must be the MeshTargets the meshes are fitted to")
        N, V = int(verts.shape[0]), self.num_verts
        if tuple(verts.shape) != (N, V, 3):
            raise SmalfitError("verts must be (num_meshes, %d, 3)" % V)
        S = 0
        if points is not None:
            if not (isinstance(points, torch.Tensor) and points.dim() == 3 and int(points.shape[0]) == N and int(points.shape[2]) == 3):
                raise SmalfitError("points must be (num_meshes, S, 3)")
            if points.device != verts.device:
                raise SmalfitError("points must be on the device of verts (%s)" % verts.device)
            S = int(points.shape[1])
        dev = verts.device
        a = _lib.SurfaceTermArgs()
        a.num_meshes, a.w_point_surface, a.w_vert_surface = N, float(w_point_surface), float(w_vert_surface)
        a.verts, a.points, a.num_points = _ptr(verts), _ptr(points), S
        out = {}
        new = lambda k, shape, dtype=torch.float32, zero=False: _out_tensor(out, k, shape, dtype, dev, zero=zero)
        a.losses, a.rows, a.dverts, a.dtrans = (_ptr(new(k, shape)) for k, shape in (("losses", (3,)), ("rows", (N, 2)), ("dverts", (N, V, 3)),
                                                                                    ("dtrans", (N, 3))))
        point_dir, vert_dir = w_point_surface > 0 and points is not None, w_vert_surface > 0
        if correspondences:
            if point_dir:
                a.point_face, a.point_bary = C.c_void_p(new("point_face", (N, S), torch.int32).data_ptr()), _ptr(new("point_bary", (N, S, 3)))
                a.point_residual = _ptr(new("point_residual", (N, S, 3)))
            if vert_dir:
                a.vert_face, a.vert_bary = C.c_void_p(new("vert_face", (N, V), torch.int32).data_ptr()), _ptr(new("vert_bary", (N, V, 3)))
                a.vert_residual = _ptr(new("vert_residual", (N, V, 3)))
        # the blocks that are on, each with its outputs attached
        g = rb = None
        if robust is not None:
            rd = _robust_of(robust)
            rb = robust_block(rd)
            rb.surface_weight_sums = _ptr(new("surface_weight_sums", (N, 2), zero=True))
            if point_dir and _scale_on(rd["sigma_surface_point"]):
                rb.surface_point_weights = _ptr(new("point_weights", (N, S), zero=True))
            if vert_dir and _scale_on(rd["sigma_surface_vert"]):
                rb.surface_vert_weights = _ptr(new("vert_weights", (N, V), zero=True))
        if gates is not None:
            g = surface_gate_block(gates)
            if point_normals is not None:
                if tuple(point_normals.shape) != (N, S, 3) or point_normals.device != dev:
                    raise SmalfitError("point_normals must be (num_meshes, S, 3) on the device of verts")
                g.point_normals = _ptr(point_normals)
            g.kept = C.c_void_p(new("kept", (N, 2), torch.int32, zero=True).data_ptr())
            if point_dir:
                g.point_kept = C.c_void_p(new("point_kept", (N, S), torch.uint8).data_ptr())
            if vert_dir:
                g.vert_kept = C.c_void_p(new("vert_kept", (N, V), torch.uint8).data_ptr())
                if g.min_cos_vert > -1.0:
                    g.vert_normals = _ptr(new("vert_normals", (N, V, 3)))
        # one call, through the narrowest entry point whose signature holds the last block that is on
        name, blocks = _narrowest(_SURFACE_ENTRY_POINTS, g, rb)
        check(fn(self.handle, targets.handle if targets is not None else None, _stream(), C.byref(a), *_refs(blocks)), name)
        return out


# the entry points of an evaluation by the number of opt-in blocks their signatures hold: none, the gate block, the robust block
_EVAL_ENTRY_POINTS = ("smalfit_mesh_objective_eval", "smalfit_mesh_objective_eval_gated", "smalfit_mesh_objective_eval_robust")
_SURFACE_ENTRY_POINTS = ("smalfit_mesh_surface_eval", "smalfit_mesh_surface_eval_gated", "smalfit_mesh_surface_eval_robust")


class RigidAligner:
    """Rigid pre-alignment of (N,V,3) vertices onto (N,S,3) points: iterative closest point from several starting orientations at
    once (smalfit_rigid_aligner; the definition is this project's, include/smalfit.h).  A handle of its own: it needs no engine,
    no objective and no targets."""

    def __init__(self, max_meshes, max_verts, max_points, max_starts=_lib.MAX_RIGID_STARTS):
        if not torch.cuda.is_available():
            raise SmalfitError("no HIP device available: smalify_amd has no CPU fallback")
        self.lib = _lib.load()
        self.max_meshes, self.max_verts, self.max_points = int(max_meshes), int(max_verts), int(max_points)
        self.max_starts = int(max_starts)
        create = _lib.resolve(self.lib, "smalfit_rigid_aligner_create")
        self._destroy = _lib.resolve(self.lib, "smalfit_rigid_aligner_destroy")
        self._align = _lib.resolve(self.lib, "smalfit_rigid_align")
        torch.cuda.init()
        torch.cuda.current_device()
        h = C.c_void_p()
        check(create(self.max_meshes, self.max_verts, self.max_points, self.max_starts, C.byref(h)), "smalfit_rigid_aligner_create")
        self.handle = h

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self._destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def align(self, verts, points, starts=None, start_transforms=None, iterations=30, w_point=1.0, w_vert=1.0, history=False,
              correspondences=False, out=None, trim_point=1.0, trim_vert=1.0, kept=False):
        """verts (N,V,3), points (N,S,3): float32 device tensors.  starts: None (the library's 24 rotations of the cube) or host
        (K,3,3) proper rotations; start_transforms: device (N,K,12) rows [R | t], used as they are (then starts must be None) -- the
        `transforms` of an earlier call continue it.  -> dict of device tensors: transforms (N,K,12), scores (N,K), best (N) int32,
        best_transform (N,12), kept_rotation (N,K) int32, with history=True history (N,K,iterations+1), with correspondences=True
        vert_nn (N,K,V) / point_nn (N,K,S) int32 of the score's scans (a direction of weight 0 is not scanned: its tensor keeps what
        it held).  `out` may carry preallocated tensors under the same keys.  Nothing synchronises.
        trim_point / trim_vert: the fraction in (0, 1] of the points / vertices every iteration keeps, those of smallest d^2
        (smalfit_trimmed_rigid_align; a partial or cluttered scan): keep = keep_count(fraction, count).  Both 1.0 and kept=False:
        smalfit_rigid_align itself.  kept=True adds point_kept (N,K,S) / vert_kept (N,K,V) uint8 and trim_d2 (N,K,2) of the score's
        round, and keep_point / keep_vert (ints).  The first trimmed call of an aligner allocates."""
        keep = {}
        for name, fraction in (("trim_point", trim_point), ("trim_vert", trim_vert)):
            fraction = float(fraction)
            if not (0.0 < fraction <= 1.0):
                raise SmalfitError("%s must be in (0, 1], got %r" % (name, fraction))
            keep[name] = fraction
        if not (isinstance(verts, torch.Tensor) and verts.dim() == 3 and int(verts.shape[2]) == 3):
            raise SmalfitError("verts must be (num_meshes, V, 3)")
        N, V = int(verts.shape[0]), int(verts.shape[1])
        # the library cannot know the extent or the device of a pointer
        if not (isinstance(points, torch.Tensor) and points.dim() == 3 and int(points.shape[0]) == N and int(points.shape[2]) == 3):
            raise SmalfitError("points must be (num_meshes, S, 3)")
        if points.device != verts.device:
            raise SmalfitError("points must be on the device of verts (%s)" % verts.device)
        S = int(points.shape[1])
        dev = verts.device
        a = _lib.RigidAlignArgs()
        host_starts = None
        if start_transforms is not None:
            if not (isinstance(start_transforms, torch.Tensor) and start_transforms.dim() == 3 and int(start_transforms.shape[0]) == N
                    and int(start_transforms.shape[2]) == 12):
                raise SmalfitError("start_transforms must be (num_meshes, K, 12)")
            if start_transforms.device != dev:
                raise SmalfitError("start_transforms must be on the device of verts (%s)" % dev)
            K = int(start_transforms.shape[1])
            a.start_transforms = _ptr(start_transforms)
            if starts is not None:       # the library words the refusal
                host_starts = _host(starts, np.float32).reshape(-1, 3, 3)
        elif starts is not None:
            host_starts = _host(starts, np.float32).reshape(-1, 3, 3)
            K = int(host_starts.shape[0])
        else:
            K = _lib.NUM_CUBE_ROTATIONS
        if host_starts is not None:
            a.starts = host_starts.ctypes.data
        iterations = int(iterations)
        a.num_meshes, a.num_verts, a.num_points, a.num_starts, a.iterations = N, V, S, K, iterations
        a.verts, a.points = _ptr(verts), _ptr(points)
        a.w_point, a.w_vert = float(w_point), float(w_vert)
        o = out if out is not None else {}
        fields = [("transforms", (N, K, 12), torch.float32), ("scores", (N, K), torch.float32), ("best", (N,), torch.int32),
                  ("best_transform", (N, 12), torch.float32), ("kept_rotation", (N, K), torch.int32)]
        if history:
            fields.append(("history", (N, K, max(iterations, 0) + 1), torch.float32))
        if correspondences:
            fields += [("vert_nn", (N, K, V), torch.int32), ("point_nn", (N, K, S), torch.int32)]
        for key, shape, dt in fields:
            t = _out_tensor(o, key, shape, dt, dev, zero=True)
            # a caller's tensor is written through its raw pointer: it must lie where and how the library expects it
            if t.device != dev or not t.is_contiguous():
                raise SmalfitError("out[%r] must be a contiguous tensor on the device of verts (%s)" % (key, dev))
            setattr(a, key, C.c_void_p(t.data_ptr()))
        if not kept and keep["trim_point"] == 1.0 and keep["trim_vert"] == 1.0:
            check(self._align(self.handle, _stream(), C.byref(a)), "smalfit_rigid_align")
            return o
        t = _lib.RigidTrimArgs()
        t.keep_point, t.keep_vert = keep_count(keep["trim_point"], S), keep_count(keep["trim_vert"], V)
        if kept:
            for key, shape, dt in (("vert_kept", (N, K, V), torch.uint8), ("point_kept", (N, K, S), torch.uint8),
                                   ("trim_d2", (N, K, 2), torch.float32)):
                buf = _out_tensor(o, key, shape, dt, dev, zero=True)
                if buf.device != dev or not buf.is_contiguous():
                    raise SmalfitError("out[%r] must be a contiguous tensor on the device of verts (%s)" % (key, dev))
                setattr(t, key, C.c_void_p(buf.data_ptr()))
            o["keep_point"], o["keep_vert"] = int(t.keep_point), int(t.keep_vert)
        check(_lib.resolve(self.lib, "smalfit_trimmed_rigid_align")(self.handle, _stream(), C.byref(a), C.byref(t)),
              "smalfit_trimmed_rigid_align")
        return o


def keep_count(fraction, count):
    """how many of `count` queries a trim fraction in (0, 1] keeps: min(count, max(1, ceil(fraction count))) in double -- the rule
    of rigid_keep_count (smalify_amd/csrc/rigid_align_math.h), restated for the binding"""
    return int(min(int(count), max(1, math.ceil(float(fraction) * int(count)))))


TEMPORAL_KEYS = ("w_temp_joint", "w_temp_global", "w_temp_trans")


def temporal_weights(weights=None):
    """the three temporal weights of a scan sequence with every one 0 (off), overridden by `weights`; an unknown key raises"""
    out = dict.fromkeys(TEMPORAL_KEYS, 0.0)
    for k, v in (weights or {}).items():
        if k not in out:
            raise KeyError("unknown temporal weight %r (have %s)" % (k, list(TEMPORAL_KEYS)))
        out[k] = float(v)
    return out


TEMPORAL_VERTEX_KEYS = ("w_temp_vert_vel", "w_temp_vert_acc")


def temporal_vertex_weights(weights=None):
    """the two weights of the temporal terms on the posed vertices of a scan sequence (velocity, acceleration) with both 0 (off),
    overridden by `weights`; an unknown key raises"""
    out = dict.fromkeys(TEMPORAL_VERTEX_KEYS, 0.0)
    for k, v in (weights or {}).items():
        if k not in out:
            raise KeyError("unknown temporal vertex weight %r (have %s)" % (k, list(TEMPORAL_VERTEX_KEYS)))
        out[k] = float(v)
    return out


def temporal_vertex_on(weights):
    """some weight of temporal_vertex_weights is positive (with none a stage calls what it called without the block)"""
    return any(weights[k] > 0 for k in TEMPORAL_VERTEX_KEYS)


def check_clip_lengths(clip_lengths, num_meshes):
    """-> the lengths as a list of ints; ValueError unless they are positive and sum to num_meshes"""
    lengths = [int(c) for c in clip_lengths]
    if not lengths or any(c <= 0 for c in lengths) or sum(lengths) != int(num_meshes):
        raise ValueError("clip_lengths %r: positive integers with sum %d expected" % (lengths, int(num_meshes)))
    return lengths


class ScanSequence:
    """The meshes of a batch as clips of one animal each (smalfit_scan_sequence; the definitions are this project's,
    include/smalfit.h): within a clip one shape -- the betas gradient rows of a clip replaced by their sum -- and the 2-D fitter's
    temporal terms between consecutive poses; and, on the posed vertices, a velocity and an acceleration term (vertex_term).  A
    handle of its own, for one N and one list of lengths."""

    def __init__(self, clip_lengths, num_meshes=None):
        if not torch.cuda.is_available():
            raise SmalfitError("no HIP device available: smalify_amd has no CPU fallback")
        lengths = [int(c) for c in clip_lengths]
        self.num_meshes = int(sum(lengths) if num_meshes is None else num_meshes)
        self.clip_lengths = tuple(lengths)
        self.lib = _lib.load()
        create = _lib.resolve(self.lib, "smalfit_scan_sequence_create")
        self._destroy = _lib.resolve(self.lib, "smalfit_scan_sequence_destroy")
        self._couple = _lib.resolve(self.lib, "smalfit_scan_sequence_couple")
        torch.cuda.init()
        torch.cuda.current_device()
        h = C.c_void_p()
        check(create(self.num_meshes, len(lengths), (C.c_int * max(len(lengths), 1))(*lengths), C.byref(h)), "smalfit_scan_sequence_create")
        self.handle = h

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self._destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def block(self, share_shape=True, temporal=None, losses=None, step_total=None):
        """-> (smalfit_sequence_args, its losses tensor (4,)): the block of couple() and of smalfit_scan_sequence_step"""
        w = temporal_weights(temporal)
        if losses is None:
            losses = torch.zeros(4, device="cuda")
        q = _lib.SequenceArgs()
        q.share_shape = int(bool(share_shape))
        q.w_temp_joint, q.w_temp_global, q.w_temp_trans = (w[k] for k in TEMPORAL_KEYS)
        q.losses = losses.data_ptr()
        q.step_total = step_total.data_ptr() if step_total is not None else None
        return q, losses

    def couple(self, global_rot=None, joint_rot=None, trans=None, g_betas=None, g_theta=None, g_trans=None, share_shape=True,
               temporal=None, losses=None):
        """the coupling alone on the caller's gradients, in place (smalfit_scan_sequence_couple): g_betas (N,nb) rows of a clip
        become their sum; g_theta (N,105) or (N,35,3) and g_trans (N,3) receive the temporal terms' gradients at global_rot (N,3),
        joint_rot (N,34,3), trans (N,3).  Any gradient may be None.  -> losses (4,) device: joint, global, trans, their sum"""
        q, losses = self.block(share_shape, temporal, losses)
        nb = int(g_betas.shape[1]) if g_betas is not None else 0
        check(self._couple(self.handle, _stream(), C.byref(q), nb, _ptr(global_rot), _ptr(joint_rot), _ptr(trans), _ptr(g_betas),
                           _ptr(g_theta), _ptr(g_trans)), "smalfit_scan_sequence_couple")
        return losses

    def vertex_block(self, temporal_verts=None, losses=None, step_total=None):
        """-> (smalfit_sequence_vertex_args, its losses tensor (3,)): the block of vertex_term() and of
        smalfit_scan_sequence_vertex_step"""
        w = temporal_vertex_weights(temporal_verts)
        if losses is None:
            losses = torch.zeros(3, device="cuda")
        q = _lib.SequenceVertexArgs()
        q.w_temp_vert_vel, q.w_temp_vert_acc = (w[k] for k in TEMPORAL_VERTEX_KEYS)
        q.losses = losses.data_ptr()
        q.step_total = step_total.data_ptr() if step_total is not None else None
        return q, losses

    def vertex_term(self, verts, temporal_verts=None, want_dverts=True, want_dtrans=True, losses=None, out=None):
        """the velocity and acceleration terms alone at verts (N,V,3) (smalfit_scan_sequence_vertex_term) -> dict(losses (3,):
        velocity, acceleration, their sum; dverts (N,V,3) and dtrans (N,3): the terms' gradient and its sum over every mesh's
        vertices, None where not wanted).  `out`: a dict of an earlier call whose tensors are written again"""
        N, V = int(verts.shape[0]), int(verts.shape[1])
        if N != self.num_meshes or verts.dim() != 3 or int(verts.shape[2]) != 3:
            raise ValueError("verts %r: (%d, V, 3) expected" % (tuple(verts.shape), self.num_meshes))
        out = {} if out is None else out
        q, losses = self.vertex_block(temporal_verts, losses if losses is not None else out.get("losses"))
        dverts = dtrans = None
        if want_dverts:
            dverts = out.get("dverts")
            if dverts is None or dverts.shape != verts.shape:
                dverts = torch.empty_like(verts, dtype=torch.float32)
        if want_dtrans:
            dtrans = out.get("dtrans")
            if dtrans is None:
                dtrans = torch.empty(N, 3, device=verts.device)
        check(_lib.resolve(self.lib, "smalfit_scan_sequence_vertex_term")(
            self.handle, _stream(), C.byref(q), V, _ptr(verts), _ptr(dverts), _ptr(dtrans)), "smalfit_scan_sequence_vertex_term")
        out.update(losses=losses, dverts=dverts, dtrans=dtrans)
        return out


def _narrowest(names, *blocks):
    """-> (the narrowest entry point of `names` whose signature holds the last block that is not None, the blocks it takes: a
    library built before the later symbols still serves the calls it could serve)"""
    while blocks and blocks[-1] is None:
        blocks = blocks[:-1]
    return names[len(blocks)], blocks


def _refs(blocks):
    return tuple(C.byref(b) if b is not None else None for b in blocks)


def _out_tensor(o, key, shape, dtype, dev, zero=False):
    """o[key] when it has this shape and dtype, else a new tensor (zeroed on request) put there; -> the tensor"""
    if key not in o or tuple(o[key].shape) != tuple(shape) or o[key].dtype != dtype:
        o[key] = (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=dev)
    return o[key]


SURFACE_GATE_KEYS = ("max_dist_point", "max_dist_vert", "min_cos_point", "min_cos_vert", "reject_boundary")


def surface_gates(gates=None):
    """the gates of the surface term with every one off, overridden by `gates`; an unknown key raises"""
    out = dict(max_dist_point=0.0, max_dist_vert=0.0, min_cos_point=-1.0, min_cos_vert=-1.0, reject_boundary=False)
    for k, v in (gates or {}).items():
        if k not in out:
            raise KeyError("unknown surface gate %r (have %s)" % (k, sorted(out)))
        out[k] = bool(v) if k == "reject_boundary" else float(v)
    return out


def surface_gate_block(gates):
    """a smalfit_surface_gate_args with the switches of `gates` (a dict as surface_gates takes it); the pointers are the caller's"""
    gd = surface_gates(gates)
    g = _lib.SurfaceGateArgs()
    g.max_dist_point, g.max_dist_vert = gd["max_dist_point"], gd["max_dist_vert"]
    g.min_cos_point, g.min_cos_vert = gd["min_cos_point"], gd["min_cos_vert"]
    g.reject_boundary = int(gd["reject_boundary"])
    return g


CHAMFER_GATE_KEYS = SURFACE_GATE_KEYS


def chamfer_gates(gates=None):
    """the gates of the chamfer term with every one off, overridden by `gates`; an unknown key raises"""
    out = dict(max_dist_point=0.0, max_dist_vert=0.0, min_cos_point=-1.0, min_cos_vert=-1.0, reject_boundary=False)
    for k, v in (gates or {}).items():
        if k not in out:
            raise KeyError("unknown chamfer gate %r (have %s)" % (k, sorted(out)))
        out[k] = bool(v) if k == "reject_boundary" else float(v)
    return out


_chamfer_gates_of = chamfer_gates      # (for callers whose own keyword is named chamfer_gates)


def chamfer_gates_on(gates):
    """some gate of the dict (as chamfer_gates returns it) is switched on"""
    return bool(gates["reject_boundary"] or gates["min_cos_point"] > -1 or gates["min_cos_vert"] > -1 or
                (gates["max_dist_point"] > 0 and np.isfinite(gates["max_dist_point"])) or
                (gates["max_dist_vert"] > 0 and np.isfinite(gates["max_dist_vert"])))


def chamfer_gate_block(gates):
    """a smalfit_chamfer_gate_args with the switches of `gates` (a dict as chamfer_gates takes it); the pointers are the caller's"""
    gd = chamfer_gates(gates)
    g = _lib.ChamferGateArgs()
    g.max_dist_point, g.max_dist_vert = gd["max_dist_point"], gd["max_dist_vert"]
    g.min_cos_point, g.min_cos_vert = gd["min_cos_point"], gd["min_cos_vert"]
    g.reject_boundary = int(gd["reject_boundary"])
    return g


ROBUST_KEYS = ("sigma_chamfer_point", "sigma_chamfer_vert", "sigma_surface_point", "sigma_surface_vert")


def robust(scales=None):
    """the four scales of the Geman-McClure kernel (smalfit_robust_args) with every one off, overridden by `scales`; an unknown
    key raises"""
    out = dict.fromkeys(ROBUST_KEYS, 0.0)
    for k, v in (scales or {}).items():
        if k not in out:
            raise KeyError("unknown robust key %r (have %s)" % (k, sorted(out)))
        out[k] = float(v)
    return out


_robust_of = robust      # (for callers whose own keyword is named robust)


def _scale_on(sigma):
    return bool(sigma > 0 and np.isfinite(sigma))


def robust_on(scales):
    """some scale of the dict (as robust returns it) is switched on"""
    return any(_scale_on(scales[k]) for k in ROBUST_KEYS)


def robust_block(scales):
    """a smalfit_robust_args with the scales of `scales` (a dict as robust takes it); the pointers are the caller's"""
    rd = robust(scales)
    r = _lib.RobustArgs()
    for k in ROBUST_KEYS:
        setattr(r, k, rd[k])
    return r


class MeshTargets:
    """Target meshes resident in HBM + the area-weighted point sampler (smalfit_mesh_targets; reference
    fitter_3d/utils.py:253 Meshes(...) and trainer.py:209 sample_points_from_meshes)."""

    def __init__(self, verts_list, faces_list):
        if not torch.cuda.is_available():
            raise SmalfitError("no HIP device available: smalify_amd has no CPU fallback")
        if len(verts_list) == 0 or len(verts_list) != len(faces_list):
            raise SmalfitError("need one (verts, faces) pair per target mesh")
        self.lib = _lib.load()
        self.verts_list = [_host(v, np.float32).reshape(-1, 3) for v in verts_list]
        self.faces_list = [_host(f, np.int32).reshape(-1, 3) for f in faces_list]
        vc = np.array([len(v) for v in self.verts_list], np.int32)
        fc = np.array([len(f) for f in self.faces_list], np.int32)
        vv = np.ascontiguousarray(np.concatenate(self.verts_list, axis=0))
        ff = np.ascontiguousarray(np.concatenate(self.faces_list, axis=0))
        torch.cuda.init()
        torch.cuda.current_device()
        h = C.c_void_p()
        check(self.lib.smalfit_mesh_targets_create(len(vc), vc.ctypes.data, fc.ctypes.data, vv.ctypes.data,
                                                   ff.ctypes.data, C.byref(h)), "smalfit_mesh_targets_create")
        self.handle = h
        self.device = torch.device("cuda", torch.cuda.current_device())

    def __len__(self):
        return len(self.verts_list)

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.smalfit_mesh_targets_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def build_index(self, cell_scale=0.0):
        """A uniform grid over every target mesh for the vertex -> surface scans of MeshObjective.surface / .score and
        Stage.step (smalfit_mesh_targets_build_index): built on the host, once; every result stays what it is without it, bit
        for bit.  For scan targets of 10^5 faces and more.  cell_scale: 0 = the library's own; for tests and tuning.
        Calling it again rebuilds."""
        a = _lib.ScanIndexArgs()
        a.cell_scale = float(cell_scale)
        check(_lib.resolve(self.lib, "smalfit_mesh_targets_build_index")(self.handle, C.byref(a)), "smalfit_mesh_targets_build_index")
        self.has_index = True
        return self

    has_index = False

    def index_stats(self):
        """-> one dict per target mesh: dims (3,), cells, occupied_cells, entries, oversize, largest_cell, bytes
        (smalfit_mesh_targets_index_stats); raises without an index"""
        fn = _lib.resolve(self.lib, "smalfit_mesh_targets_index_stats")
        out = []
        for n in range(len(self)):
            s = _lib.ScanIndexStats()
            check(fn(self.handle, n, C.byref(s)), "smalfit_mesh_targets_index_stats")
            out.append({"dims": tuple(s.dims), "cells": s.cells, "occupied_cells": s.occupied_cells, "entries": s.entries,
                        "oversize": s.oversize, "largest_cell": s.largest_cell, "bytes": int(s.bytes)})
        return out

    def sample(self, num_points, seed, iteration, out=None):
        """(N, num_points, 3) points; the same (seed, iteration) always gives the same points"""
        N = len(self)
        if out is None or tuple(out.shape) != (N, int(num_points), 3):
            out = torch.empty(N, int(num_points), 3, device=self.device)
        check(self.lib.smalfit_mesh_targets_sample(self.handle, _stream(), int(num_points), int(seed) & (2 ** 64 - 1),
                                                   int(iteration) & 0xFFFFFFFF, _ptr(out)), "smalfit_mesh_targets_sample")
        return out

    def sample_normals(self, num_points, seed, iteration, out=None, normals_out=None):
        """-> (points, normals), both (N, num_points, 3): the points of sample() bit for bit, and with every point the unit
        normal of the target face it lies on (smalfit_mesh_targets_sample_normals)"""
        fn = _lib.resolve(self.lib, "smalfit_mesh_targets_sample_normals")
        shape = (len(self), int(num_points), 3)
        if out is None or tuple(out.shape) != shape:
            out = torch.empty(*shape, device=self.device)
        if normals_out is None or tuple(normals_out.shape) != shape:
            normals_out = torch.empty(*shape, device=self.device)
        check(fn(self.handle, _stream(), int(num_points), int(seed) & (2 ** 64 - 1), int(iteration) & 0xFFFFFFFF, _ptr(out),
                 _ptr(normals_out)), "smalfit_mesh_targets_sample_normals")
        return out, normals_out

    def sample_attrs(self, num_points, seed, iteration, out=None, normals_out=None, boundary_out=None, normals=True, boundary=True):
        """-> (points, normals or None, boundary or None): the points of sample() bit for bit, with every point the unit normal
        of the target face it lies on (N, num_points, 3) and its boundary byte (N, num_points) uint8: 1 when that face has a
        boundary edge or a corner that ends one (smalfit_mesh_targets_sample_attrs)"""
        fn = _lib.resolve(self.lib, "smalfit_mesh_targets_sample_attrs")
        shape = (len(self), int(num_points), 3)
        if out is None or tuple(out.shape) != shape:
            out = torch.empty(*shape, device=self.device)
        if normals and (normals_out is None or tuple(normals_out.shape) != shape):
            normals_out = torch.empty(*shape, device=self.device)
        if boundary and (boundary_out is None or tuple(boundary_out.shape) != shape[:2]):
            boundary_out = torch.empty(*shape[:2], dtype=torch.uint8, device=self.device)
        check(fn(self.handle, _stream(), int(num_points), int(seed) & (2 ** 64 - 1), int(iteration) & 0xFFFFFFFF, _ptr(out),
                 _ptr(normals_out) if normals else None, C.c_void_p(boundary_out.data_ptr()) if boundary else None),
              "smalfit_mesh_targets_sample_attrs")
        return out, (normals_out if normals else None), (boundary_out if boundary else None)
