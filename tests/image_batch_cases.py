"""Problems and expected values for batches of INDEPENDENT images (smalfit_fit_args.subject_frames = 1,
smalify_amd.image_batch.ImageBatchFitter), shared by tests/test_image_batch_cpu.py and tests/test_gpu_image_batch.py.

An independent image IS a one-frame FitProblem of the oracle (window 1, no temporal term), so the expected values of a
batch are N separate calls of oracle.smal_oracle.loss_and_grads / Adam -- the oracle itself is unchanged.  Every image has
its own ground-truth shape, limb scales, pose and translation (tests/parity_cases.random_pose with its own seed and depth).
Nothing here needs a GPU; nothing here asserts.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import smal_oracle as so
from smalify_amd import config as cfg
from smalify_amd import model_io, synthetic
from tests.lbs_forms import skin_form      # noqa: F401  (the cases' launch forms: ic.skin_form(N))
from tests import parity_cases as pc

TERMS = ("joint", "pose", "splay", "betas", "sil_reproj", "temp_joint", "temp_global", "temp_trans", "limit")
PARAMS = ("betas", "log_beta_scales", "global_rotation", "joint_rotations", "trans")

# test 1: batch size -> the skinning launch run_lbs_forward takes for it (tests/lbs_forms.skin_form, asserted on the CPU)
EVAL_CASES = ((1, "plain"), (3, "plain"), (6, "split"), (20, "split"), (64, "wide"))
S_EVAL = 64


def stage_weights(stage):
    W = np.array(cfg.OPT_WEIGHTS).T
    return W[stage][:6].copy(), float(W[stage][7]), float(W[stage][8])      # weights, epochs, lr


def image_seed(n, seed=300):
    return seed + 17 * n


def image_depth(n):
    return 1.25 + 0.05 * (n % 9)


def make_images(N, S, seed=300, unity=True, dtype=torch.float64):
    """-> list of N dicts: prob (one-frame FitProblem), near (a perturbed state near the image's own ground truth),
    tg (tj (1,25,2), vis (1,25), tsil (1,S,S)).  unity=False: the 20-dim prior (the leading block of the synthetic prior)
    and no limb scales."""
    md, _ = pc.get_oracle_model()
    om = so.OracleModel(md, dtype=dtype)
    pp = synthetic.synthetic_pose_prior()
    sp = synthetic.synthetic_shape_prior()
    out = []
    for n in range(N):
        _, near, tg = pc.make_problem_cpu(1, S, 1, seed=image_seed(n, seed), z=image_depth(n))
        prec, mean = (sp[0], sp[1]) if unity else shape_prior_20()
        prob = so.FitProblem(om, S, tg["tj"], tg["vis"], tg["tsil"], pp[0], pp[1], pp[2], prec, mean, 1,
                             use_unity_prior=unity, dtype=dtype)
        if not unity:
            near = dict(near, log_beta_scales=np.zeros(6, np.float32))
        out.append(dict(prob=prob, near=near, tg=tg))
    return out


def shape_prior_20():
    sp = synthetic.synthetic_shape_prior()
    return np.ascontiguousarray(sp[0][:20, :20]), np.ascontiguousarray(sp[1][:20])


def initial_state(unity=True):
    """a one-image SMALFitter's initial parameters (smal_fitter.py:58-97)"""
    sp = synthetic.synthetic_shape_prior()
    return dict(betas=sp[1][:20].astype(np.float32).copy(),
                log_beta_scales=(sp[1][20:26] if unity else np.zeros(6)).astype(np.float32).copy(),
                global_rotation=model_io.initial_global_rotation()[None].astype(np.float32).copy(),
                joint_rotations=np.zeros((1, 34, 3), np.float32), trans=np.zeros((1, 3), np.float32))


def stack(states):
    """N one-image parameter dicts -> the batch's tensors: betas (N,20), log_beta_scales (N,6), the rest (N,...)"""
    return dict(betas=np.stack([s["betas"] for s in states]).astype(np.float32),
                log_beta_scales=np.stack([s["log_beta_scales"] for s in states]).astype(np.float32),
                global_rotation=np.concatenate([s["global_rotation"] for s in states]).astype(np.float32),
                joint_rotations=np.concatenate([s["joint_rotations"] for s in states]).astype(np.float32),
                trans=np.concatenate([s["trans"] for s in states]).astype(np.float32))


def targets(images):
    return dict(tj=np.concatenate([im["tg"]["tj"] for im in images]).astype(np.float32),
                vis=np.concatenate([im["tg"]["vis"] for im in images]).astype(np.float32),
                tsil=np.concatenate([im["tg"]["tsil"] for im in images]).astype(np.float32))


def oracle_eval(prob, state, stage, trainable=None, dtype=torch.float64):
    """-> (terms (9,), {name: gradient}) of one image: one epoch objective of a one-frame problem"""
    weights, _, _ = stage_weights(stage)
    trainable = so.trainable_names(stage) if trainable is None else trainable
    p = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in state.items()}
    vis = so.stage0_visibility(prob.vis) if stage == 0 else None
    _, sums, grads = so.loss_and_grads(prob, p, weights, 0.0, trainable, vis)
    return np.array([sums.get(t, 0.0) for t in TERMS], np.float64), {k: g.numpy().astype(np.float64) for k, g in grads.items()}


def as_dtype(image, dtype):
    """the same problem in another precision (the float32 oracle is the yardstick of the gradient bound)"""
    p = image["prob"]
    md, _ = pc.get_oracle_model()
    om = so.OracleModel(md, dtype=dtype)
    return so.FitProblem(om, p.S, image["tg"]["tj"], image["tg"]["vis"], image["tg"]["tsil"], p.pose_prec, p.pose_mean,
                         p.pose_mask, p.shape_prec, p.shape_mean, 1, use_unity_prior=p.unity, dtype=dtype)


def oracle_loop(prob, state, schedule, allow_limb_scaling=True):
    """the reference loop of ONE image in float64: schedule = [(stage, iterations)], a new Adam per stage
    (optimize_to_joints.py:96) -> final parameters (numpy)"""
    p = {k: torch.from_numpy(np.asarray(v)).double() for k, v in state.items()}
    for stage, iters in schedule:
        weights, _, lr = stage_weights(stage)
        names = so.trainable_names(stage, allow_limb_scaling)
        opt = so.Adam(names, lr)
        vis = so.stage0_visibility(prob.vis) if stage == 0 else None
        for _ in range(iters):
            _, _, grads = so.loss_and_grads(prob, p, weights, 0.0, names, vis)
            opt.step(p, grads)
    return {k: v.numpy() for k, v in p.items()}
