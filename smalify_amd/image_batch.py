"""A batch of UNRELATED images fitted in one call, each with its own shape.

The reference fits a dataset of single images (StanfordExtra: BASELINE config 1, `load_stanford_sequence`) one image per
SMALFitter, i.e. with N = 1 -- on this chip the worst case there is: an iteration is a chain of a dozen dependent launches
and a one-image fit leaves the machine idle between them.  `ImageBatchFitter` runs N such fits side by side through
`smalfit_fit_args.subject_frames = 1`: every image has its own betas, limb scales, shape-prior term and loss; nothing is
summed across images, so image n's result does not depend on which other images share its batch.

Reference semantics per image (file:line into the reference): the parameters and initial values of a one-image SMALFitter
(smal_fitter/smal_fitter.py:48-97), the schedule and the per-stage Adam of optimize_to_joints.py:90-137 with one window of
one frame (no temporal term: a single frame has no neighbour), the checkpoint dict of smal_fitter.py:213-219.
"""
from __future__ import annotations

import os
import pickle

import numpy as np
import torch

from . import config
from . import engine as eng
from . import fitter as fit
from . import smal_topology as topo

PARAM_NAMES = fit.PARAM_NAMES


def flat_layout(N):
    """-> ({name: (offset, count)}, {name: shape}, total) of the flat parameter / gradient / moment buffers of N images:
    [betas(N*20) | log_beta_scales(N*6) | joint_rotations(N*102) | global_rotation(N*3) | trans(N*3)] -- stage 0's set
    (global_rotation, trans) and the all-parameter set are each ONE contiguous Adam range, like FusedFitter's."""
    offsets, off = {}, 0
    for name, count in (("betas", N * 20), ("log_beta_scales", N * 6), ("joint_rotations", N * 102),
                        ("global_rotation", N * 3), ("trans", N * 3)):
        offsets[name] = (off, count)
        off += count
    shapes = dict(betas=(N, 20), log_beta_scales=(N, 6), joint_rotations=(N, 34, 3), global_rotation=(N, 3), trans=(N, 3))
    return offsets, shapes, off


def trainable_names(stage_id, allow_limb_scaling=True):
    """optimize_to_joints.py:98-104: stage 0 moves the animal only; later stages train everything (limb scales if allowed)"""
    if stage_id == 0:
        return ("global_rotation", "trans")
    names = ["betas", "joint_rotations", "global_rotation", "trans"]
    if allow_limb_scaling:
        names.insert(1, "log_beta_scales")
    return tuple(names)


def adam_ranges(offsets, names):
    """merged [begin, end) ranges of the flat buffers that cover exactly the tensors `names`"""
    segs = []
    for k in PARAM_NAMES:
        if k not in names:
            continue
        o, c = offsets[k]
        if segs and segs[-1][1] == o:
            segs[-1][1] = o + c
        else:
            segs.append([o, o + c])
    return [tuple(s) for s in segs]


class ImageBatchFitter(fit.FusedFitter):
    """FusedFitter's surface for N independent images: `trainable`, `begin_stage`, `evaluate`, `run_iterations`, `step`,
    `run_schedule`, `frame_parameters`, `export_checkpoints`, `load_checkpoint`, and `image_losses()`.

    use_unity_prior: the 26-dim prior over [betas_n | log_beta_scales_n], every image starting from the prior's mean limb
    scales (what SMALFitter does for its one shared tensor, smal_fitter.py:61); otherwise the 20-dim prior and limb scales
    that start at zero.  The engine must hold the matching shape prior (Engine.set_shape_prior)."""

    def __init__(self, engine: eng.Engine, target_joints, target_visibility, target_sil, use_unity_prior=True,
                 mean_betas=None, mean_log_scales=None, allow_limb_scaling=True, sil_storage="auto"):
        self._last_eval = None
        super().__init__(engine, target_joints, target_visibility, target_sil, 1, use_unity_prior=use_unity_prior,
                         mean_betas=mean_betas, mean_log_scales=mean_log_scales, allow_limb_scaling=allow_limb_scaling,
                         sil_storage=sil_storage)
        self.losses_per_image = torch.zeros(self.N, eng.NUM_LOSS_TERMS, device=engine.device, dtype=torch.float32)

    # ---- layout -----------------------------------------------------------------------------------------------
    def _limb_scales_shared(self):
        return False                           # nothing is shared between images

    def _parameter_layout(self, N):
        return flat_layout(N)

    def _initial_shape(self, mean_betas, mean_log_scales, f32):
        if mean_betas is not None:
            self.p["betas"].copy_(torch.as_tensor(np.asarray(mean_betas)[:20], **f32)[None].expand(self.N, 20))
        if mean_log_scales is not None and self.unity:
            self.p["log_beta_scales"].copy_(torch.as_tensor(np.asarray(mean_log_scales), **f32)[None].expand(self.N, 6))

    def _sequence_kwargs(self):
        return dict(window=1, temporal=False, subject_frames=1)

    # ---- evaluation ---------------------------------------------------------------------------------------------
    def evaluate(self, weights, w_temp=0.0, stage_id=1, want=None, **outs):
        self._last_eval = (tuple(float(w) for w in weights), stage_id)
        return super().evaluate(weights, 0.0, stage_id, want, **outs)

    def run_iterations(self, weights, w_temp, lr, stage_id, iterations):
        """`iterations` epochs of every image's loop in one library call.  w_temp is accepted for FusedFitter's signature
        and ignored: unrelated images have no temporal term."""
        self._last_eval = (tuple(float(w) for w in weights), stage_id)
        return super().run_iterations(weights, 0.0, lr, stage_id, iterations)

    def prepare_schedule(self, opt_weights=None):
        """FusedFitter.prepare_schedule with the temporal weight this class evaluates with (0): the blocks it builds are the
        ones run_iterations looks up"""
        W = np.array(config.OPT_WEIGHTS if opt_weights is None else opt_weights).T
        for stage_id, w in enumerate(W):
            self._stage_plan(w[:6], 0.0, float(w[8]), stage_id, self.trainable(stage_id))

    def image_losses(self, weights=None, stage_id=None):
        """-> (N, 9) device tensor: image n's nine loss terms (LOSS_NAMES order) at the current parameters, with the weights
        and stage of the last evaluate / run_iterations unless given.  One evaluation; `losses` then holds the column sums,
        the gradients are those of that evaluation.  Meant for once per fit or per stage: the call marshals a fresh
        argument block (~100 us of host work) and runs the rasteriser's per-frame-loss instantiations plus one more
        launch; the loop itself (run_iterations) never asks for rows."""
        if weights is None or stage_id is None:
            if self._last_eval is None:
                raise eng.SmalfitError("image_losses: give weights and stage_id (nothing has been evaluated yet)")
            weights, stage_id = (self._last_eval[0] if weights is None else weights), (self._last_eval[1] if stage_id is None else stage_id)
        self.evaluate(weights, 0.0, stage_id, want=self.trainable(stage_id), losses_per_frame=self.losses_per_image)
        return self.losses_per_image

    def _forward_kwargs(self):
        return self._sequence_kwargs()

    def image_metrics(self, thresholds=(0.15,), want_mask=False):
        """FusedFitter.metrics with one row per image: row n of sil_counts / keypoint_dist / pck_counts is image n's, and
        does not depend on which other images share its batch.  The first thing to ask after a batch: which fits failed."""
        return self.metrics(thresholds=thresholds, want_mask=want_mask)

    # ---- what only a sequence has ---------------------------------------------------------------------------------
    def _not_for_images(self, *a, **k):
        raise eng.SmalfitError("independent images are not sharded over ranks: give every rank its own ImageBatchFitter")

    local_step = shard_run = shared_step = shared_grad = boundary_records = num_shared = _not_for_images

    # ---- checkpoints: image n's file is what a one-image FusedFitter fit writes ------------------------------------
    def frame_parameters(self):
        gr = (self.p["global_rotation"] * self.global_mask).cpu().numpy()
        jr = (self.p["joint_rotations"] * self.rotation_mask).cpu().numpy()
        tr = self.p["trans"].cpu().numpy()
        betas = self.p["betas"].cpu().numpy()
        ls = self.p["log_beta_scales"].cpu().numpy()
        return [{"global_rotation": gr[i].astype(np.float32), "joint_rotations": jr[i].astype(np.float32),
                 "betas": betas[i].astype(np.float32), "log_betascale": ls[i].astype(np.float32),
                 "trans": tr[i].astype(np.float32)} for i in range(self.N)]

    def load_checkpoint(self, checkpoint_path, epoch):
        """per image what SMALFitter.load_checkpoint reads for a one-image fit (smal_fitter.py:192-207): image n from
        <checkpoint_path>/<n:04>/<epoch>.pkl, its own betas and limb scales (the mean over one frame)"""
        dev = self.flat.device
        for n in range(self.N):
            with open(os.path.join(checkpoint_path, "{0:04}".format(n), "{0}.pkl".format(epoch)), "rb") as f:
                d = pickle.load(f)
            self.p["global_rotation"][n] = torch.from_numpy(np.asarray(d["global_rotation"], np.float32)).to(dev)
            self.p["joint_rotations"][n] = torch.from_numpy(np.asarray(d["joint_rotations"], np.float32)).to(dev).view(34, 3)
            self.p["trans"][n] = torch.from_numpy(np.asarray(d["trans"], np.float32)).to(dev)
            self.p["betas"][n] = torch.from_numpy(np.asarray(d["betas"], np.float32)[:topo.NUM_BETAS]).to(dev)
            self.p["log_beta_scales"][n] = torch.from_numpy(np.asarray(d["log_betascale"], np.float32).reshape(6)).to(dev)
