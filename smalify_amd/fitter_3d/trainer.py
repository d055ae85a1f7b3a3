"""Drop-in for reference fitter_3d/trainer.py: SMAL3DFitter, SMALParamGroup, Stage, StageManager.

What stays identical: constructor arguments, parameter names and shapes, the five optimisation schemes
(trainer.py:113-119), per-parameter learning rates, one fresh Adam per Stage (trainer.py:194, default betas), the loss
weights and their defaults (trainer.py:31), the .npz written by Stage.save_npz (trainer.py:264-279).

What is different underneath: one Stage.step is ONE C-ABI call on the current HIP stream (smalfit_fit3d_step: SMAL
forward, target-point sampling, all four loss terms, the gradient back through the SMAL model, Adam on the scheme's
parameters -- 14 kernel launches) with no autograd graph and no host synchronisation; the loss history stays on
the device until it is plotted or printed.  Stage.evaluate / Stage.step_unfused compose the same iteration from the
component entry points (smalfit_lbs_forward, smalfit_mesh_targets_sample, smalfit_mesh_objective_eval,
smalfit_lbs_backward, smalfit_adam_step) and expose the gradients.  The target points are drawn by a counter-based
generator keyed by (seed, global iteration), not by torch's global generator, so runs are reproducible.

Two reference quirks kept on purpose: log_beta_scales sits in the parameter groups but has requires_grad=False, so no
scheme ever changes it (trainer.py:64-65); deform_verts is trainable by the "deform" scheme as it is on the reference's
CPU path (on its CUDA path `nn.Parameter(...).to(device)` yields a non-leaf tensor the optimiser rejects, trainer.py:91).
"""
from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np
import torch
import torch.nn as nn

from .. import _lib, config, engine as eng, metrics as fit_metrics, model_io, runtime
from ..smal_model.smal_torch import SMAL

default_weights = dict(w_chamfer=1.0, w_edge=1.0, w_normal=0.01, w_laplacian=0.1)     # trainer.py:31
_WEIGHT_ORDER = ("w_chamfer", "w_edge", "w_normal", "w_laplacian")
# the opt-in point-to-surface term (no counterpart in the reference; include/smalfit.h): accepted in `loss_weights` beside the
# four keys above, kept apart from them, off by default
default_surface_weights = dict(w_point_surface=0.0, w_vert_surface=0.0)
_SURFACE_ORDER = ("w_point_surface", "w_vert_surface")
N_SAMPLE_POINTS = 3000                                                                 # trainer.py:209
_PARAM_ORDER = ("betas", "log_beta_scales", "global_rot", "joint_rot", "trans", "deform_verts")
# Stage.metrics draws its target points with a key of its own: the counter-based sampler gives the same points for the same
# (seed, iteration), so a score does not depend on where the fit's sampler stands -- and never repeats one of its draws
METRICS_SEED_OFFSET = 0x6D657472         # added to the stage's seed when no seed is given
METRICS_ITERATION = 0xFFFFFFFF
DEFAULT_METRIC_THRESHOLDS = (0.01, 0.02, 0.05)      # of the target's half-extent: load_meshes scales every target to [-1, 1]


class SMAL3DFitter(nn.Module):
    def __init__(self, batch_size=1, device="cuda", shape_family=-1, model_data=None, smal_data=None):
        """model_data / smal_data let tests inject synthetic stand-ins for the SMAL pickles; by default both are read
        from the paths in smalify_amd.config like the reference (trainer.py:47-58)."""
        super().__init__()
        if not torch.cuda.is_available():
            raise eng.SmalfitError("no HIP device available: smalify_amd has no CPU fallback")
        dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.batch_size = int(batch_size)
        self.n_betas = config.N_BETAS
        self.shape_family_list = np.array(shape_family)
        if smal_data is None:
            smal_data = model_io.load_pickle(config.SMAL_DATA_FILE)
        prec, mean = model_io.family_shape_prior(smal_data, shape_family, config.N_BETAS)
        self.betas_prec = torch.from_numpy(np.ascontiguousarray(prec, np.float32)).to(dev)
        self.mean_betas = torch.from_numpy(np.ascontiguousarray(mean, np.float32)).to(dev)
        N = self.batch_size
        self.betas = nn.Parameter(self.mean_betas.unsqueeze(0).repeat(N, 1))
        self.log_beta_scales = nn.Parameter(torch.zeros(N, 6, device=dev), requires_grad=False)
        self.global_rot = nn.Parameter(torch.zeros(N, 3, device=dev))          # eul_to_axis([0, 0, 0]) = 0
        self.trans = nn.Parameter(torch.zeros(N, 3, device=dev))
        self.joint_rot = nn.Parameter(torch.zeros(N, config.N_POSE, 3, device=dev))
        self.global_mask = torch.ones(1, 3, device=dev)                        # unused by forward, as in the reference
        self.rotation_mask = torch.ones(config.N_POSE, 3, device=dev)
        self.smal_model = SMAL(dev, shape_family_id=shape_family, model_data=model_data)
        self.faces = self.smal_model.faces.unsqueeze(0).repeat(N, 1, 1)
        self.deform_verts = nn.Parameter(torch.zeros(N, *self.smal_model.v_template.shape, device=dev))
        self._theta = torch.zeros(N, 35, 3, device=dev)

    # ---- C-ABI plumbing ---------------------------------------------------------------------------------------
    def _engine(self):
        return runtime.get_engine(self.smal_model.device_model, self.batch_size, self.smal_model.engine_image_size)

    def _pack_theta(self):
        self._theta[:, 0].copy_(self.global_rot.detach())
        self._theta[:, 1:].copy_(self.joint_rot.detach())
        return self._theta

    def lbs_verts(self):
        """SMAL(betas, [global_rot | joint_rot], betas_logscale) -> (N,V,3), trainer.py:95-100"""
        e = self._engine()
        return e.lbs_forward(self.betas.detach().contiguous(), self._pack_theta(),
                             self.log_beta_scales.detach().contiguous(), want_Rs=False, want_v_shaped=False)[0]

    def forward(self):
        """verts + trans + deform_verts (trainer.py:94-108), composed on the device by the objective's first kernel;
        detached -- gradients come from Stage.step"""
        o = _objective_for(self, N_SAMPLE_POINTS).eval(self.lbs_verts(), self.trans.detach().contiguous(),
                                                        self.deform_verts.detach().contiguous(), None, (0.0, 0.0, 0.0, 0.0))
        return o["verts"]


class SMALParamGroup:
    """Same parameter map and per-parameter learning rates as trainer.py:111-153."""
    param_map = {
        "init": ["global_rot", "trans"],
        "default": ["global_rot", "joint_rot", "trans", "betas", "log_beta_scales"],
        "shape": ["global_rot", "trans", "betas", "log_beta_scales"],
        "pose": ["global_rot", "trans", "joint_rot"],
        "deform": ["deform_verts"],
    }

    def __init__(self, model, group="smbld", lrs=None):
        self.model = model
        self.group = group
        assert group in self.param_map, f"Group {group} not in list of available params: {list(self.param_map.keys())}"
        self.lrs = dict(lrs) if lrs is not None else {}

    def names(self):
        return list(self.param_map[self.group])

    def __iter__(self):
        out = []
        for param_name in self.param_map[self.group]:
            d = {"params": [getattr(self.model, param_name)], "name": param_name}
            if param_name in self.lrs:
                d["lr"] = self.lrs[param_name]
            out.append(d)
        return iter(out)


# smalfit_fit3d_step and its wider forms, by the number of opt-in blocks their signatures hold behind the step's own: the surface
# block, its gate block, the chamfer gate block, the robust block
_STEP_ENTRY_POINTS = ("smalfit_fit3d_step", "smalfit_fit3d_step_surface", "smalfit_fit3d_step_gated", "smalfit_fit3d_step_partial",
                      "smalfit_fit3d_step_robust")


class Stage:
    """One stage of optimisation (trainer.py:157-262)."""

    def __init__(self, nits: int, scheme: str, smal_3d_fitter: SMAL3DFitter, target_meshes, mesh_names=[],
                 name="optimise", loss_weights=None, lr=1e-3, out_dir="static_fits_output", custom_lrs=None,
                 device="cuda", seed=0, iteration_offset=0, scan_index=False, clip_lengths=None, share_shape=True, temporal=None,
                 temporal_verts=None, surface_gates=None, chamfer_gates=None, robust=None):
        self.n_it = int(nits)
        self.name = name
        self.out_dir = out_dir
        self.target_meshes = target_meshes
        self.mesh_names = mesh_names
        self.smal_3d_fitter = smal_3d_fitter
        self.device = smal_3d_fitter.device
        self.loss_weights = default_weights.copy()
        self.surface_weights = default_surface_weights.copy()
        if loss_weights is not None:
            for k, v in loss_weights.items():
                if k in self.surface_weights:
                    self.surface_weights[k] = float(v)
                    continue
                if k not in self.loss_weights:
                    raise KeyError("unknown loss weight %r (have %s)" % (k, sorted(self.loss_weights) + sorted(self.surface_weights)))
                self.loss_weights[k] = float(v)
        # the gates of the surface term for partial scans (include/smalfit.h): all off unless given, here or as a `surface_gates`
        # block of the stage's YAML; an unknown key raises, as an unknown loss weight does
        self.surface_gates = eng.surface_gates(surface_gates)
        # ... and the same three kinds of gate on the chamfer term's two scans (constructor or a `chamfer_gates` block of the YAML)
        self.chamfer_gates = eng.chamfer_gates(chamfer_gates)
        # the Geman-McClure kernel on the matches the gates keep (include/smalfit.h): four scales, all off unless given, here or as
        # a `robust` block of the stage's YAML; with or without the gates
        self.robust = eng.robust(robust)
        # a grid over the targets for the vertex -> surface scans of step() and metrics() (include/smalfit.h): for dense scan
        # targets; it changes no result.  Built here, once per set of targets; the targets carry it from then on
        self.scan_index = bool(scan_index)
        if self.scan_index and not target_meshes.has_index:
            target_meshes.build_index()
        if custom_lrs is not None:
            for attr in custom_lrs:
                assert hasattr(smal_3d_fitter, attr), f"attr '{attr}' not in SMAL."
        self.param_group = SMALParamGroup(smal_3d_fitter, scheme, custom_lrs)
        self.scheduler = None
        self.lr = float(lr)
        if len(target_meshes) != smal_3d_fitter.batch_size:
            raise ValueError("%d target meshes for a fitter of batch size %d" % (len(target_meshes), smal_3d_fitter.batch_size))
        # fresh Adam state per stage (trainer.py:194); frozen parameters (requires_grad=False) get none
        self._adam = {}
        for g in self.param_group:
            p = g["params"][0]
            if p.requires_grad:
                self._adam[g["name"]] = dict(lr=float(g.get("lr", self.lr)), m=torch.zeros_like(p), v=torch.zeros_like(p))
        fit = smal_3d_fitter
        # a scan sequence (include/smalfit.h): the batch as clips of one animal each, in batch order; within a clip one shape and the
        # temporal terms between consecutive poses.  None: the meshes are unrelated, and nothing of this is constructed or called
        self.clip_lengths = None if clip_lengths is None else tuple(eng.check_clip_lengths(clip_lengths, fit.batch_size))
        self.share_shape = bool(share_shape)
        self.temporal = eng.temporal_weights(temporal)
        self._sequence = None
        self._seq_args = None          # smalfit_sequence_args of step(), built on the first step
        self._seq_losses = None
        # ... and the velocity and acceleration terms on the posed vertices of a clip; both weights 0 unless given, and then
        # evaluations and steps are the calls of before
        self.temporal_verts = eng.temporal_vertex_weights(temporal_verts)
        self._vert_args = None         # smalfit_sequence_vertex_args of step(), built on the first step while a weight is positive
        self._vert_losses = None
        self._vert_out = None
        if temporal_verts is not None and self.clip_lengths is None:
            raise ValueError("temporal_verts ties the posed vertices within a clip: give clip_lengths with it")
        if self.clip_lengths is not None:
            self._sequence = eng.ScanSequence(self.clip_lengths, fit.batch_size)
            if self.share_shape and "betas" in self._adam:
                _require_tied_shapes(fit, self.clip_lengths)     # one host read, here only
        V = int(fit.smal_model.v_template.shape[0])
        self.n_verts = V
        self.faces = fit.faces.detach()
        self.src_verts = fit().detach()
        self._objective = _objective_for(fit, N_SAMPLE_POINTS)
        self._buffers = {}
        self._points = None
        self._last_points = None
        self.seed = int(seed)
        self.iteration_offset = int(iteration_offset)      # global iteration of this stage's first step (StageManager)
        self._loss_history = torch.zeros(max(self.n_it, 1), device=self.device)
        self._done = 0
        self._t = 0              # Adam step count of this stage
        self._args = None        # smalfit_fit3d_args, built on the first step
        self._surface_args = None      # smalfit_surface_term_args of step(), built with it when a surface weight is positive
        self._surface_losses = None
        self._gate_args = None         # smalfit_surface_gate_args of step(), built with the surface block while a gate is on
        self._surface_kept = None
        self._point_normals = None
        self._cgate_args = None        # smalfit_chamfer_gate_args of step(), built on the first step while a chamfer gate is on
        self._chamfer_kept = None
        self._point_boundary = None
        self._robust_args = None       # smalfit_robust_args of step(), built on the first step while a scale applies
        self._robust_weights = None
        self.consider_loss = lambda loss_name: self.loss_weights[f"w_{loss_name}"] > 0

    # ---- evaluation ----------------------------------------------------------------------------------------------
    @property
    def losses_to_plot(self):
        """total loss per completed iteration (host floats; reading it synchronises)"""
        return self._loss_history[:self._done].cpu().tolist()

    @property
    def last_points(self):
        """the target points of the most recent evaluation or step, (N, 3000, 3)"""
        return self._last_points if self._last_points is not None else self._points

    @property
    def last_terms(self):
        """device tensor (5,): chamfer, edge, normal, laplacian (unweighted) and the weighted total"""
        return self._buffers.get("losses")

    @property
    def last_surface_terms(self):
        """device tensor (3,): L_ps, L_vs and the weighted surface term of the most recent evaluation or step; None while the
        term is off"""
        return self._surface_losses

    @property
    def surface_on(self):
        return any(self.surface_weights[k] > 0 for k in _SURFACE_ORDER)

    @property
    def gates_on(self):
        """some gate of the surface term is switched on (with all of them off a step is the ungated call)"""
        g = self.surface_gates
        return (g["reject_boundary"] or g["min_cos_point"] > -1 or g["min_cos_vert"] > -1 or
                (g["max_dist_point"] > 0 and np.isfinite(g["max_dist_point"])) or
                (g["max_dist_vert"] > 0 and np.isfinite(g["max_dist_vert"])))

    @property
    def last_surface_kept(self):
        """device tensor (N,2) int32: the kept points | kept vertices of every mesh in the most recent gated evaluation or step;
        None while the term or its gates are off"""
        return self._surface_kept

    @property
    def chamfer_gates_on(self):
        """some gate of the chamfer term is switched on (with all of them off a step is the call of before)"""
        return eng.chamfer_gates_on(self.chamfer_gates)

    @property
    def last_chamfer_kept(self):
        """device tensor (N,2) int32: the kept points | kept vertices of every mesh in the chamfer term of the most recent gated
        evaluation or step; None while the term or its gates are off"""
        return self._chamfer_kept

    @property
    def robust_on(self):
        """some scale of the robust kernel is switched on"""
        return eng.robust_on(self.robust)

    def _robust_chamfer(self):
        r = self.robust
        return self.loss_weights["w_chamfer"] > 0 and (eng._scale_on(r["sigma_chamfer_point"]) or eng._scale_on(r["sigma_chamfer_vert"]))

    def _robust_surface(self):
        r, sw = self.robust, self.surface_weights
        return ((sw["w_point_surface"] > 0 and eng._scale_on(r["sigma_surface_point"])) or
                (sw["w_vert_surface"] > 0 and eng._scale_on(r["sigma_surface_vert"])))

    def _robust_applies(self):
        """a scale is on for a term that is on: otherwise evaluations and steps are the calls of before"""
        return self._robust_chamfer() or self._robust_surface()

    @property
    def last_robust_weights(self):
        """dict(chamfer=, surface=) of device tensors (N,2): the sums of w over the kept points | kept vertices of every mesh in
        the most recent robust evaluation or step (a term without a scale on: None); None while no scale applies"""
        return self._robust_weights

    @property
    def last_temporal_losses(self):
        """device tensor (4,): the temporal terms on joint_rot, global_rot and trans and their sum, of the most recent evaluation or
        step; None without clip_lengths"""
        return self._seq_losses

    @property
    def last_temporal_vertex_losses(self):
        """device tensor (3,): the velocity and acceleration terms on the posed vertices and their sum, of the most recent
        evaluation or step; None while both weights are off"""
        return self._vert_losses

    def _vertex_terms_on(self):
        return self._sequence is not None and eng.temporal_vertex_on(self.temporal_verts)

    def _chamfer_gated(self):
        return self.chamfer_gates_on and self.loss_weights["w_chamfer"] > 0

    def _weights(self):
        return [self.loss_weights[k] for k in _WEIGHT_ORDER]

    def evaluate(self, iteration, points=None):
        """loss terms and gradients at the current parameters -> (total (device scalar), grads by parameter name)"""
        fit = self.smal_3d_fitter
        e = fit._engine()
        betas = fit.betas.detach().contiguous()
        ls = fit.log_beta_scales.detach().contiguous()
        theta = fit._pack_theta()
        lbs = e.lbs_forward(betas, theta, ls, want_Rs=False, want_v_shaped=False)[0]
        gated = self.surface_on and self.gates_on
        cgated = self._chamfer_gated()
        cg = self.chamfer_gates
        normals = boundary = None
        surface_normals = gated and self.surface_weights["w_point_surface"] > 0 and self.surface_gates["min_cos_point"] > -1
        chamfer_normals = cgated and (cg["min_cos_point"] > -1 or cg["min_cos_vert"] > -1)
        if points is None and cgated and (chamfer_normals or cg["reject_boundary"]):
            # the points with what the chamfer gates ask of them (and the surface gates' normals, drawn once)
            points, normals, boundary = self.target_meshes.sample_attrs(
                N_SAMPLE_POINTS, self.seed, self.iteration_offset + iteration, out=self._sample_buffer(), normals_out=self._point_normals,
                boundary_out=self._point_boundary, normals=bool(chamfer_normals or surface_normals), boundary=bool(cg["reject_boundary"]))
            self._point_normals = normals if normals is not None else self._point_normals
            self._point_boundary = boundary if boundary is not None else self._point_boundary
        elif points is None and surface_normals:
            points, normals = self.target_meshes.sample_normals(N_SAMPLE_POINTS, self.seed, self.iteration_offset + iteration,
                                                                out=self._sample_buffer(), normals_out=self._point_normals)
            self._point_normals = normals
        elif points is None and (self.loss_weights["w_chamfer"] > 0 or self.surface_weights["w_point_surface"] > 0):
            points = self.target_meshes.sample(N_SAMPLE_POINTS, self.seed, self.iteration_offset + iteration, out=self._sample_buffer())
        self._last_points = points            # the sampler's buffer is never rebound: smalfit_fit3d_step writes through its raw pointer
        o = self._objective.eval(lbs, fit.trans.detach().contiguous(), fit.deform_verts.detach().contiguous(), points,
                                 self._weights(), out=self._buffers, chamfer_gates=cg if cgated else None,
                                 point_normals=normals if chamfer_normals else None, point_boundary=boundary if cgated else None,
                                 targets=self.target_meshes if cgated else None,
                                 robust=self.robust if self._robust_chamfer() else None)
        self._buffers = o
        self._chamfer_kept = o["kept"] if cgated else None
        self._robust_weights = (dict(chamfer=o["chamfer_weight_sums"] if self._robust_chamfer() else None, surface=None)
                                if self._robust_applies() else None)
        total = o["losses"][4]
        if self.surface_on:
            # the stand-alone call's gradient joins the objective's before the LBS adjoint
            wp, wv = (self.surface_weights[k] for k in _SURFACE_ORDER)
            sf = self._objective.surface(o["verts"], self.target_meshes, points if wp > 0 else None, wp, wv,
                                         gates=self.surface_gates if gated else None,
                                         point_normals=normals if wp > 0 and surface_normals else None,
                                         robust=self.robust if self._robust_surface() else None)
            self._surface_kept = sf.get("kept")
            if self._robust_surface():
                self._robust_weights["surface"] = sf["surface_weight_sums"]
            o["dverts"] += sf["dverts"]
            o["dtrans"] += sf["dtrans"]
            self._surface_losses = sf["losses"]
            total = total + sf["losses"][2]
        if self._vertex_terms_on():
            # the stand-alone call's gradient joins where the surface term's does, behind it
            self._vert_out = self._sequence.vertex_term(o["verts"], self.temporal_verts, out=self._vert_out)
            o["dverts"] += self._vert_out["dverts"]
            o["dtrans"] += self._vert_out["dtrans"]
            self._vert_losses = self._vert_out["losses"]
        dbeta, dtheta, dls = e.lbs_backward(betas, theta, ls, o["dverts"], None)
        if self._sequence is not None:
            # the coupling alone on the gradients of the trained parameters, where the fused step applies it: behind the LBS adjoint
            pose = "global_rot" in self._adam or "joint_rot" in self._adam
            self._seq_losses = self._sequence.couple(
                fit.global_rot.detach().contiguous(), fit.joint_rot.detach().contiguous(), fit.trans.detach().contiguous(),
                g_betas=dbeta if "betas" in self._adam else None, g_theta=dtheta if pose else None,
                g_trans=o["dtrans"] if "trans" in self._adam else None, share_shape=self.share_shape, temporal=self.temporal,
                losses=self._seq_losses)
            total = total + self._seq_losses[3]
            if self._vertex_terms_on():
                total = total + self._vert_losses[2]
        grads = {"betas": dbeta, "global_rot": dtheta[:, 0].contiguous(), "joint_rot": dtheta[:, 1:].contiguous(),
                 "log_beta_scales": dls, "trans": o["dtrans"], "deform_verts": o["dverts"]}
        return total, grads

    def forward(self, src_mesh=None):
        """total loss at the current parameters (the reference takes the offset source mesh; the engine composes it)"""
        return self.evaluate(self._done)[0]

    def step(self, epoch):
        """one iteration (trainer.py:229-241): loss, gradients and Adam on the parameters of the scheme in ONE C-ABI
        call (smalfit_fit3d_step).  Returns the total loss before the update (device scalar)."""
        fit = self.smal_3d_fitter
        e = fit._engine()
        a = self._step_args()
        for name in _PARAM_ORDER:
            setattr(a, name, getattr(fit, name).data_ptr())
        a.weights = (C.c_float * 4)(*self._weights())
        a.iteration = (self.iteration_offset + int(epoch)) & 0xFFFFFFFF
        self._t += 1
        a.adam_t = self._t
        dev_targets = getattr(self.target_meshes, "_dev", self.target_meshes)
        # the blocks that are on, in the order the entry points take them; the surface gates ride on the surface block
        sf = gate = None
        if self.surface_on:
            sf = self._surface_block()
            sf.w_point_surface, sf.w_vert_surface = (self.surface_weights[k] for k in _SURFACE_ORDER)
            gate = self._gate_block() if self.gates_on else None
        cgate = self._chamfer_gate_block() if self._chamfer_gated() else None
        rb = self._robust_block() if self._robust_applies() else None
        if self._sequence is not None:
            # a scan sequence: the widest step, with the sequence block behind the four others
            q = self._sequence_block()
            if self._vertex_terms_on():
                # ... and the vertex block behind that
                vq = self._vertex_block()
                name = "smalfit_scan_sequence_vertex_step"
                eng.check(_lib.resolve(e.lib, name)(self._sequence.handle, e.handle, self._objective.handle, dev_targets.handle,
                                                    eng._stream(), C.byref(a), *eng._refs((sf, gate, cgate, rb)), C.byref(q),
                                                    C.byref(vq)), name)
                self._last_points = self._points
                return self._vert_total[0]
            name = "smalfit_scan_sequence_step"
            eng.check(_lib.resolve(e.lib, name)(self._sequence.handle, e.handle, self._objective.handle, dev_targets.handle, eng._stream(),
                                                C.byref(a), *eng._refs((sf, gate, cgate, rb)), C.byref(q)), name)
            self._last_points = self._points
            return self._seq_total[0]
        # one call, through the narrowest entry point whose signature holds the last block that is on
        name, blocks = eng._narrowest(_STEP_ENTRY_POINTS, sf, gate, cgate, rb)
        eng.check(_lib.resolve(e.lib, name)(e.handle, self._objective.handle, dev_targets.handle, eng._stream(), C.byref(a),
                                            *eng._refs(blocks)), name)
        self._last_points = self._points
        # with the surface term the grand total is formed by the step: the four terms + the surface term
        return self._step_total[0] if sf is not None else self._buffers["losses"][4]

    def step_unfused(self, epoch):
        """the same iteration as five separate C-ABI calls + one smalfit_adam_step per parameter; leaves the gradients
        in `.grad` of the trained parameters (development / inspection path, ~3x the host time of step())"""
        loss, grads = self.evaluate(epoch)
        fit = self.smal_3d_fitter
        self._t += 1
        for name, st in self._adam.items():
            p = getattr(fit, name)
            g = grads[name]
            p.grad = g
            eng.adam_step(p.data, g, st["m"], st["v"], st["lr"], self._t, beta1=0.9, beta2=0.999, eps=1e-8)
        return loss

    def metrics(self, thresholds=DEFAULT_METRIC_THRESHOLDS, num_points=N_SAMPLE_POINTS, seed=None):
        """How good the fit is now, per mesh (no counterpart in the reference; definitions: include/smalfit.h).  One forward
        (smal_3d_fitter()), num_points target points drawn with a seed and iteration of their own, one smalfit_mesh_score call:
        exact point-to-surface distances both ways.  Changes nothing a later step reads.  -> the dict of
        smalify_amd.metrics.summarise_mesh_score (host floats; reading it synchronises)"""
        verts = self.smal_3d_fitter()
        key = (self.seed + METRICS_SEED_OFFSET if seed is None else int(seed)) & (2 ** 64 - 1)
        points = self.target_meshes.sample(int(num_points), key, METRICS_ITERATION) if num_points else None
        objective = _objective_for(self.smal_3d_fitter, max(int(num_points), N_SAMPLE_POINTS))
        thresholds = tuple(float(t) for t in thresholds)
        o = objective.score(verts, self.target_meshes, points, thresholds)
        return fit_metrics.summarise_mesh_score(o["sums"], o.get("within"), num_verts=self.n_verts, num_points=int(num_points),
                                                thresholds=thresholds)

    def _sample_buffer(self):
        """the one (N, 3000, 3) tensor the sampler writes into, allocated once and kept for the life of the stage (the cached
        argument block of step() holds its device pointer)"""
        if self._points is None:
            self._points = torch.empty(self.smal_3d_fitter.batch_size, N_SAMPLE_POINTS, 3, device=self.device)
        return self._points

    def _step_args(self):
        if self._args is None:
            fit = self.smal_3d_fitter
            N = fit.batch_size
            a = _lib.Fit3dArgs()
            a.num_meshes, a.num_betas, a.num_points = N, int(fit.betas.shape[1]), N_SAMPLE_POINTS
            for name in _PARAM_ORDER:
                if name == "log_beta_scales":          # read by the forward, never trained (trainer.py:64-65)
                    continue
                st = self._adam.get(name)
                setattr(a, "lr_" + name, st["lr"] if st else 0.0)
                setattr(a, "m_" + name, st["m"].data_ptr() if st else None)
                setattr(a, "v_" + name, st["v"].data_ptr() if st else None)
            a.beta1, a.beta2, a.eps = 0.9, 0.999, 1e-8
            a.points = None
            a.seed = self.seed & (2 ** 64 - 1)
            if "losses" not in self._buffers:
                self._buffers["losses"] = torch.zeros(5, device=self.device)
            a.points_out = self._sample_buffer().data_ptr()
            a.losses = self._buffers["losses"].data_ptr()
            a.verts_out = None
            self._args = a
        return self._args

    def _surface_block(self):
        """the smalfit_surface_term_args of step(): the step's own vertices and points, the term's three figures"""
        if self._surface_args is None:
            sf = _lib.SurfaceTermArgs()
            sf.num_meshes = self.smal_3d_fitter.batch_size
            self._step_losses = torch.zeros(3, device=self.device)
            self._step_total = torch.zeros(1, device=self.device)
            sf.losses, sf.step_total = self._step_losses.data_ptr(), self._step_total.data_ptr()
            self._surface_args = sf
        self._surface_losses = self._step_losses
        return self._surface_args

    def _gate_block(self):
        """the smalfit_surface_gate_args of step(): the stage's switches, the kept counts (the step samples its own points and
        draws their normals with them)"""
        if self._gate_args is None:
            self._gate_args = eng.surface_gate_block(self.surface_gates)
            self._step_kept = torch.zeros(self.smal_3d_fitter.batch_size, 2, dtype=torch.int32, device=self.device)
            self._gate_args.kept = self._step_kept.data_ptr()
        self._surface_kept = self._step_kept
        return self._gate_args

    def _chamfer_gate_block(self):
        """the smalfit_chamfer_gate_args of step(): the stage's switches, the kept counts (the step samples its own points and
        draws their normals and boundary bytes with them)"""
        if self._cgate_args is None:
            self._cgate_args = eng.chamfer_gate_block(self.chamfer_gates)
            self._step_chamfer_kept = torch.zeros(self.smal_3d_fitter.batch_size, 2, dtype=torch.int32, device=self.device)
            self._cgate_args.kept = self._step_chamfer_kept.data_ptr()
        self._chamfer_kept = self._step_chamfer_kept
        return self._cgate_args

    def _sequence_block(self):
        """the smalfit_sequence_args of step(): the stage's switch and weights, the four temporal figures, the grand total"""
        if self._seq_args is None:
            self._seq_step_losses = torch.zeros(4, device=self.device)
            self._seq_total = torch.zeros(1, device=self.device)
            self._seq_args, _ = self._sequence.block(self.share_shape, self.temporal, self._seq_step_losses, self._seq_total)
        self._seq_losses = self._seq_step_losses
        return self._seq_args

    def _vertex_block(self):
        """the smalfit_sequence_vertex_args of step(): the stage's two weights, the three figures, the grand total"""
        if self._vert_args is None:
            self._vert_step_losses = torch.zeros(3, device=self.device)
            self._vert_total = torch.zeros(1, device=self.device)
            self._vert_args, _ = self._sequence.vertex_block(self.temporal_verts, self._vert_step_losses, self._vert_total)
        self._vert_losses = self._vert_step_losses
        return self._vert_args

    def _robust_block(self):
        """the smalfit_robust_args of step(): the stage's scales, the weight sums of both terms"""
        if self._robust_args is None:
            self._robust_args = eng.robust_block(self.robust)
            N = self.smal_3d_fitter.batch_size
            self._step_robust = dict(chamfer=torch.zeros(N, 2, device=self.device), surface=torch.zeros(N, 2, device=self.device))
            self._robust_args.chamfer_weight_sums = self._step_robust["chamfer"].data_ptr()
            self._robust_args.surface_weight_sums = self._step_robust["surface"].data_ptr()
        self._robust_weights = dict(chamfer=self._step_robust["chamfer"] if self._robust_chamfer() else None,
                                    surface=self._step_robust["surface"] if self._robust_surface() else None)
        return self._robust_args

    def run(self, plot=False, progress=True, report_every=50):
        """Run the entire Stage (trainer.py:257-270).  The description line is refreshed every `report_every`
        iterations: each refresh reads the loss back and so synchronises with the device."""
        it = range(self.n_it)
        bar = None
        if progress:
            try:
                from tqdm import tqdm
                bar = tqdm(it)
                it = bar
            except ImportError:
                bar = None
        for i in it:
            loss = self.step(i)
            self._loss_history[i].copy_(loss)
            self._done = i + 1
            if bar is not None and (i % report_every == 0 or i == self.n_it - 1):
                bar.set_description(f"STAGE = {self.name}, TOT_LOSS = {float(loss):.6f}")
        if plot:
            self.plot()

    def plot(self):
        from .utils import plot_meshes
        verts = self.smal_3d_fitter()
        figtitle = f"{self.name}, its = {self.n_it}"
        plot_meshes(self.target_meshes, verts.cpu().numpy(), self.faces[0].cpu().numpy(), self.mesh_names, title=self.name,
                    figtitle=figtitle, out_dir=os.path.join(self.out_dir, "meshes"))

    def save_npz(self, labels=None):
        """same keys as trainer.py:264-279"""
        out = {}
        for param in ["global_rot", "joint_rot", "betas", "log_beta_scales", "trans", "deform_verts"]:
            out[param] = getattr(self.smal_3d_fitter, param).cpu().detach().numpy()
        out["verts"] = self.smal_3d_fitter().cpu().detach().numpy()
        out["faces"] = self.faces.cpu().detach().numpy()
        out["labels"] = labels
        if self.clip_lengths is not None:
            out["clip_lengths"] = np.asarray(self.clip_lengths, np.int64)
        os.makedirs(self.out_dir, exist_ok=True)
        np.savez(os.path.join(self.out_dir, f"{self.name}.npz"), **out)


def _objective_for(fitter, max_points):
    """one smalfit_mesh_objective per fitter (topology tables + work buffers), shared by its stages"""
    obj = getattr(fitter, "_mesh_objective", None)
    if obj is None or obj.max_points < max_points or obj.max_meshes < fitter.batch_size:
        obj = eng.MeshObjective(int(fitter.smal_model.v_template.shape[0]), fitter.smal_model.f, fitter.batch_size, max_points)
        fitter._mesh_objective = obj
    return obj


def _clip_rows_tied(x, clip_lengths):
    """every row of the host array x is bit-equal to the first row of its clip"""
    x = np.ascontiguousarray(x)
    bits = x.view(np.uint32) if x.dtype == np.float32 else x
    start = 0
    for length in clip_lengths:
        if not (bits[start:start + length] == bits[start:start + 1]).all():
            return False
        start += length
    return True


def _require_tied_shapes(fitter, clip_lengths):
    host = torch.cat([fitter.betas.detach(), fitter.log_beta_scales.detach()], dim=1).cpu().numpy()
    if not _clip_rows_tied(host, clip_lengths):
        raise ValueError("share_shape: the betas / log_beta_scales rows of a clip are not bit-equal; call "
                         "smalify_amd.fitter_3d.trainer.tie_shapes(fitter, clip_lengths) before the stage is built")


def tie_shapes(fitter, clip_lengths, how="first"):
    """One shape per clip before a sequence stage: every betas row of a clip is overwritten with one row -- how="first": the
    clip's first row; how="mean": the float32 mean of the clip's rows.  log_beta_scales is never trained and is not written: rows
    of it that differ within a clip raise ValueError.  clip_lengths: positive integers with sum fitter.batch_size, clips in batch
    order.  Reading the rows synchronises."""
    lengths = eng.check_clip_lengths(clip_lengths, fitter.batch_size)
    if how not in ("first", "mean"):
        raise ValueError("tie_shapes: how must be 'first' or 'mean', got %r" % (how,))
    if not _clip_rows_tied(fitter.log_beta_scales.detach().cpu().numpy(), lengths):
        raise ValueError("tie_shapes: log_beta_scales rows differ within a clip; they are never trained, set them equal first")
    betas = fitter.betas.detach()
    start = 0
    for length in lengths:
        rows = betas[start:start + length]
        row = rows[0].clone() if how == "first" else rows.mean(dim=0)
        rows.copy_(row.unsqueeze(0).expand_as(rows))
        start += length
    return fitter


# rigid_prealign draws its target points with a key of its own, the way Stage.metrics does: never one of the fit's draws
PREALIGN_SEED_OFFSET = 0x70726561        # added to the seed
PREALIGN_ITERATION = 0xFFFFFFFE


def _rotation_exp(r):
    """Rodrigues in float64: axis-angle (3,) -> (3,3)"""
    r = np.asarray(r, np.float64)
    th = float(np.linalg.norm(r))
    K = np.array([[0.0, -r[2], r[1]], [r[2], 0.0, -r[0]], [-r[1], r[0], 0.0]])
    if th < 1e-8:
        return np.eye(3) + K + 0.5 * (K @ K)
    return np.eye(3) + (np.sin(th) / th) * K + ((1.0 - np.cos(th)) / (th * th)) * (K @ K)


def _rotation_log(R):
    """(3,3) -> axis-angle (3,) in float64, angle in [0, pi].  R is first projected onto the rotations (a float32 matrix is not
    exactly orthonormal).  Up to a quarter turn the axis is the skew part's; beyond it, where the skew part fades towards pi, it
    comes from the unit quaternion, solved for its largest component first (Shepperd 1978): no entry is divided by a small one,
    so a float64 rotation comes back to float64 accuracy at every angle, pi included"""
    U, _, Vt = np.linalg.svd(np.asarray(R, np.float64))
    R = U @ np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt)) or 1.0]) @ Vt
    w = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = float(np.linalg.norm(w)), 0.5 * (float(np.trace(R)) - 1.0)
    if c >= 0:
        if s > 1e-6:
            return w * (float(np.arctan2(s, c)) / s)
        return w                                   # angle ~ 0: theta / sin(theta) -> 1
    q = _rotation_quaternion(R)
    if q[0] < 0:
        q = -q                                     # angle in [0, pi]; at pi itself (q[0] = 0) either axis is the rotation's
    n = float(np.linalg.norm(q[1:]))
    return q[1:] * (2.0 * float(np.arctan2(n, q[0])) / n)


def _rotation_quaternion(R):
    """the unit quaternion (w, x, y, z) of a rotation matrix, either sign: the component of largest square is taken from the
    diagonal, the other three from the off-diagonal sums and differences divided by it (it is at least 1/2)"""
    d = np.array([R[0, 0] + R[1, 1] + R[2, 2], R[0, 0] - R[1, 1] - R[2, 2], R[1, 1] - R[0, 0] - R[2, 2], R[2, 2] - R[0, 0] - R[1, 1]])
    i = int(np.argmax(d))
    h = 0.5 * np.sqrt(1.0 + d[i])
    off = {(0, 1): R[2, 1] - R[1, 2], (0, 2): R[0, 2] - R[2, 0], (0, 3): R[1, 0] - R[0, 1],
           (1, 2): R[0, 1] + R[1, 0], (1, 3): R[0, 2] + R[2, 0], (2, 3): R[1, 2] + R[2, 1]}
    q = np.array([h if j == i else off[(min(i, j), max(i, j))] / (4.0 * h) for j in range(4)])
    return q / np.linalg.norm(q)


def rigid_prealign(fitter, target_meshes, starts=None, iterations=30, num_points=N_SAMPLE_POINTS, seed=0, w_point=1.0, w_vert=1.0,
                   trim_point=1.0, trim_vert=1.0):
    """Stand the SMAL meshes where their targets stand before the first stage: multi-start ICP of fitter() onto points drawn on
    the targets (engine.RigidAligner; smalfit_rigid_align, include/smalfit.h), then the winning [R | t] of every mesh folded into
    the parameters: global_rot <- log(R exp(global_rot)) (the conversion on the host in float64) and trans such that the new
    fitter() is R (old fitter()) + t -- the root rotation turns the mesh about its rest root joint, so trans is taken from a
    second forward: the mean over the vertices of R (v_old + trans_old) + t - v_new.  betas, log_beta_scales and joint_rot are not
    touched.  deform_verts is added after the pose and would not turn with it: any non-zero entry raises ValueError.
    starts: None (the 24 rotations of the cube) or (K,3,3) proper rotations.  Opt-in: no stage calls this.
    -> one dict per mesh: best (the winning start), score, angle (radians turned), angle_degrees, kept_rotation (of the winning
    start), identity_score (the score of the identity start, None when it is not among the starts), transform (the winning
    [R | t], 12 floats in rows).  Reading it synchronises.
    trim_point / trim_vert: fractions in (0, 1] of the drawn points / of the vertices that every iteration keeps, those of smallest
    d^2 (trimmed ICP, smalfit_trimmed_rigid_align): for a scan that shows part of the animal, or a floor beside it.  Below 1 in
    either, every row also holds trim_point, trim_vert, kept_points, kept_verts (the counts) and trim_dist_point, trim_dist_vert:
    the distance of the farthest kept pair of the winning start, a direct hint for the stages' max_dist_* gates."""
    N = fitter.batch_size
    if len(target_meshes) != N:
        raise ValueError("%d target meshes for a fitter of batch size %d" % (len(target_meshes), N))
    if bool(torch.any(fitter.deform_verts.detach() != 0)):
        raise ValueError("rigid_prealign: deform_verts is not zero; it is added after the pose and would not turn with the mesh")
    num_points, iterations = int(num_points), int(iterations)
    key = (int(seed) + PREALIGN_SEED_OFFSET) & (2 ** 64 - 1)
    points = target_meshes.sample(num_points, key, PREALIGN_ITERATION)
    verts = fitter().contiguous()
    V = int(verts.shape[1])
    host_starts = None if starts is None else np.ascontiguousarray(np.asarray(starts, np.float32).reshape(-1, 3, 3))
    K = _lib.NUM_CUBE_ROTATIONS if host_starts is None else int(host_starts.shape[0])
    aligner = eng.RigidAligner(N, V, num_points, max(K, 1))
    trim_point, trim_vert = float(trim_point), float(trim_vert)
    trimmed = trim_point != 1.0 or trim_vert != 1.0
    o = aligner.align(verts, points, starts=host_starts, iterations=iterations, w_point=w_point, w_vert=w_vert,
                      trim_point=trim_point, trim_vert=trim_vert, kept=trimmed)
    T = o["best_transform"].cpu().numpy().astype(np.float64).reshape(N, 3, 4)
    best = o["best"].cpu().numpy()
    scores = o["scores"].cpu().numpy()
    kept = o["kept_rotation"].cpu().numpy()
    # the identity among the starts: start 0 of the built-in ones, else the first caller's start that is exactly I
    identity = 0 if host_starts is None else next((k for k in range(K) if np.array_equal(host_starts[k], np.eye(3, dtype=np.float32))), None)
    v_old = fitter.lbs_verts().detach().cpu().numpy().astype(np.float64)
    trans_old = fitter.trans.detach().cpu().numpy().astype(np.float64)
    rot_old = fitter.global_rot.detach().cpu().numpy().astype(np.float64)
    rot_new = np.stack([_rotation_log(T[n, :, :3] @ _rotation_exp(rot_old[n])) for n in range(N)])
    fitter.global_rot.data.copy_(torch.from_numpy(rot_new.astype(np.float32)).to(fitter.global_rot.device))
    v_new = fitter.lbs_verts().detach().cpu().numpy().astype(np.float64)
    want = np.einsum("nij,nvj->nvi", T[:, :, :3], v_old + trans_old[:, None, :]) + T[:, None, :, 3]
    trans_new = (want - v_new).mean(axis=1)
    fitter.trans.data.copy_(torch.from_numpy(trans_new.astype(np.float32)).to(fitter.trans.device))
    report = []
    for n in range(N):
        b = int(best[n])
        angle = float(np.linalg.norm(_rotation_log(T[n, :, :3])))
        report.append(dict(best=b, score=float(scores[n, b]), angle=angle, angle_degrees=float(np.degrees(angle)),
                           kept_rotation=int(kept[n, b]), identity_score=None if identity is None else float(scores[n, identity]),
                           transform=[float(v) for v in T[n].reshape(-1)]))
    if trimmed:
        trim_d2 = o["trim_d2"].cpu().numpy().astype(np.float64)
        for n, row in enumerate(report):
            row.update(trim_point=trim_point, trim_vert=trim_vert, kept_points=int(o["keep_point"]), kept_verts=int(o["keep_vert"]),
                       trim_dist_point=float(np.sqrt(trim_d2[n, row["best"], 1])), trim_dist_vert=float(np.sqrt(trim_d2[n, row["best"], 0])))
    return report


class StageManager:
    """Container for multiple stages of optimisation (trainer.py:282-323)."""

    def __init__(self, out_dir="static_fits_output", labels=None):
        self.stages = []
        self.out_dir = out_dir
        self.labels = labels

    def run(self, plot=True, progress=True, metrics=False, metric_thresholds=DEFAULT_METRIC_THRESHOLDS):
        """metrics: score the fit after every stage (Stage.metrics) and write metrics.json beside the .npz files: per stage
        the thresholds, one row per mesh and the batch figures.  Off by default, and then nothing is computed or written."""
        report = {}
        for stage in self.stages:
            stage.run(plot=plot, progress=progress)
            stage.save_npz(labels=self.labels)
            if metrics:
                summary = stage.metrics(thresholds=metric_thresholds)
                names = self._mesh_names(stage, summary["batch"]["meshes"])
                report[stage.name] = fit_metrics.mesh_score_report(summary, metric_thresholds, names)
                print("%s: %s" % (stage.name, fit_metrics.mesh_score_line(summary, metric_thresholds)))
        if metrics:
            os.makedirs(self.out_dir, exist_ok=True)
            with open(os.path.join(self.out_dir, "metrics.json"), "w") as fh:
                json.dump(dict(stages=report), fh, indent=1)
        self.plot_losses()

    def _mesh_names(self, stage, count):
        names = [str(n) for n in (self.labels if self.labels is not None else stage.mesh_names or [])]
        return names if len(names) == count and len(set(names)) == count else ["mesh_%d" % i for i in range(count)]

    def plot_losses(self, out_src="losses"):
        """semilog plot of the total loss over all stages (trainer.py:299-319)"""
        import matplotlib
        matplotlib.use("Agg")
        from matplotlib import pyplot as plt
        fig, ax = plt.subplots()
        it_start = 0
        for stage in self.stages:
            hist = stage.losses_to_plot
            ax.semilogy(np.arange(it_start, it_start + len(hist)), hist, label=stage.name)
            it_start += stage.n_it
        ax.set_xlabel("Epoch")
        ax.set_ylabel("Total loss")
        ax.legend()
        os.makedirs(self.out_dir, exist_ok=True)
        plt.tight_layout()
        fig.savefig(os.path.join(self.out_dir, out_src + ".png"))
        plt.close(fig)

    def add_stage(self, stage):
        # every stage continues the sampler's iteration counter where the previous one stopped
        stage.iteration_offset = sum(s.n_it for s in self.stages)
        self.stages.append(stage)
