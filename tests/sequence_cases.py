"""Cases and restatements of the scan-sequence block (include/smalfit.h, "scan sequences"), shared by the CPU and the GPU tests:
random states per clip layout, the float64 numpy restatement, the reference's get_temporal form in torch with autograd (per clip),
the dyadic case with its closed form, and the float32 bar.  Nothing here needs a GPU."""
from __future__ import annotations

import json
import os

import numpy as np
import torch

CLIPS = ((1,), (2,), (2, 1), (1, 3, 1), (5,))
WEIGHTS = (0.7, 1.3, 2.1)                      # joint, global, trans
NUM_BETAS = 20
TERMS = (("joint_rot", 102), ("global_rot", 3), ("trans", 3))      # in the order of `losses`
MEASURED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hip_fit3d_sequence_measured.json")
RATCHET = 3.0                                  # the project's: a bar is three times the measured float32 deviation


def clip_id(clips):
    return "clips" + "-".join(str(c) for c in clips)


def state(clips, seed=0, num_betas=NUM_BETAS):
    """random parameters and incoming gradients of sum(clips) meshes, float32"""
    N = int(sum(clips))
    rng = np.random.default_rng(1000 + 17 * seed + 131 * N + len(clips))
    f = lambda *shape, scale: (rng.standard_normal(shape) * scale).astype(np.float32)
    return dict(global_rot=f(N, 3, scale=0.5), joint_rot=f(N, 34, 3, scale=0.3), trans=f(N, 3, scale=0.4),
                g_betas=f(N, num_betas, scale=1e-2), g_theta=f(N, 105, scale=1e-2), g_trans=f(N, 3, scale=1e-2))


def _ranges(clips):
    start = 0
    for length in clips:
        yield start, int(length)
        start += int(length)


def reference64(clips, st, share_shape=True, weights=WEIGHTS):
    """the definitions restated in float64 numpy -> dict(g_betas, g_theta, g_trans, losses (4,))"""
    x = {k: np.asarray(st[k], np.float64).reshape(len(st[k]), -1) for k, _ in TERMS}
    g = {k: np.asarray(st[k], np.float64).copy() for k in ("g_betas", "g_theta", "g_trans")}
    dest = dict(joint_rot=(g["g_theta"], 3), global_rot=(g["g_theta"], 0), trans=(g["g_trans"], 0))
    losses = np.zeros(4)
    for start, length in _ranges(clips):
        if share_shape and length > 1:
            g["g_betas"][start:start + length] = g["g_betas"][start:start + length].sum(axis=0)
        for t, (name, L) in enumerate(TERMS):
            w = float(weights[t])
            if w <= 0:
                continue
            arr, col = dest[name]
            for n in range(start, start + length - 1):
                d = x[name][n + 1] - x[name][n]
                losses[t] += w * float((d * d).sum()) / L
                arr[n, col:col + L] -= 2.0 * w / L * d
                arr[n + 1, col:col + L] += 2.0 * w / L * d
    losses[3] = losses[0] + losses[1] + losses[2]
    g["losses"] = losses
    return g


def reference_torch(clips, st, weights=WEIGHTS, dtype=torch.float64):
    """the reference's get_temporal (smal_fitter/smal_fitter.py:177-190), clip by clip, with masks of ones as in SMAL3DFitter:
    F.mse_loss(x[n], x[n + 1]) * w summed over the pairs; gradients by autograd, added to the incoming ones in `dtype`
    -> dict(g_theta, g_trans, losses (4,)) as float64 numpy"""
    import torch.nn.functional as F
    x = {k: torch.tensor(np.asarray(st[k]), dtype=dtype, requires_grad=True) for k, _ in TERMS}
    terms = [torch.zeros((), dtype=dtype) for _ in TERMS]
    for start, length in _ranges(clips):
        for t, (name, _) in enumerate(TERMS):
            if weights[t] <= 0:
                continue
            for n in range(start, start + length - 1):
                terms[t] = terms[t] + F.mse_loss(x[name][n], x[name][n + 1]) * weights[t]
    total = (terms[0] + terms[1]) + terms[2]
    grads = {k: torch.zeros_like(v) for k, v in x.items()}
    if total.requires_grad:
        got = torch.autograd.grad(total, list(x.values()), allow_unused=True)
        grads = {k: (g if g is not None else torch.zeros_like(v)) for (k, v), g in zip(x.items(), got)}
    N = len(st["trans"])
    g_theta = torch.tensor(np.asarray(st["g_theta"]), dtype=dtype) + torch.cat([grads["global_rot"].reshape(N, 3), grads["joint_rot"].reshape(N, 102)], dim=1)
    g_trans = torch.tensor(np.asarray(st["g_trans"]), dtype=dtype) + grads["trans"]
    return dict(g_theta=g_theta.detach().double().numpy(), g_trans=g_trans.detach().double().numpy(),
                losses=np.array([float(t.detach()) for t in terms] + [float(total.detach())], np.float64))


def deviation(a, ref):
    """max |a - ref| over max |ref| (0 where ref is all zero and a equals it)"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    err = float(np.abs(a - ref).max()) if ref.size else 0.0
    return err / scale if scale > 0 else err


def float32_restatement_deviation():
    """how far a plain float32 torch restatement lies from the float64 one over CLIPS -> dict(loss=, grad=): what the bar is 3x of"""
    loss = grad = 0.0
    for clips in CLIPS:
        st = state(clips)
        r64, r32 = reference_torch(clips, st, dtype=torch.float64), reference_torch(clips, st, dtype=torch.float32)
        if sum(clips) > len(clips):
            loss = max(loss, max(deviation(r32["losses"][t], r64["losses"][t]) for t in range(4)))
        grad = max(grad, deviation(r32["g_theta"], r64["g_theta"]), deviation(r32["g_trans"], r64["g_trans"]))
    return dict(loss=loss, grad=grad)


def measured():
    with open(MEASURED) as fh:
        return json.load(fh)


def bars():
    """-> dict(loss=, grad=): RATCHET times the recorded float32 deviation (tests/golden/hip_fit3d_sequence_measured.json)"""
    m = measured()["float32_restatement_deviation"]
    return dict(loss=RATCHET * m["loss"], grad=RATCHET * m["grad"])


# ---- the dyadic case: every parameter a multiple of 2^-6, every weight a power of two, so every sum is exact in float32 ------
DYADIC_CLIPS = (1, 3, 2)
DYADIC_WEIGHTS = (0.5, 2.0, 1.0)


def dyadic_state(clips=DYADIC_CLIPS, num_betas=NUM_BETAS):
    """parameters k / 64 with small integers k; incoming gradients 0 for the temporal destinations (so a gradient is c times an
    exact difference: one rounding, the one of the closed form) and small dyadic numbers for the betas rows"""
    N = int(sum(clips))
    rng = np.random.default_rng(7)
    d = lambda *shape: (rng.integers(-32, 33, size=shape) / 64.0).astype(np.float32)
    return dict(global_rot=d(N, 3), joint_rot=d(N, 34, 3), trans=d(N, 3), g_betas=d(N, num_betas),
                g_theta=np.zeros((N, 105), np.float32), g_trans=np.zeros((N, 3), np.float32))


def dyadic_closed_form(clips=DYADIC_CLIPS, st=None, weights=DYADIC_WEIGHTS):
    """exact arithmetic in float64 (every intermediate is a dyadic rational of few bits), rounded to float32 where the definition
    rounds: c = (2 w) / L, the product c d, the quotient S / L, the product with w"""
    st = dyadic_state(clips) if st is None else st
    f32 = np.float32
    x = {k: np.asarray(st[k], np.float64).reshape(len(st[k]), -1) for k, _ in TERMS}
    N = len(st["trans"])
    g_theta, g_trans = np.zeros((N, 105), f32), np.zeros((N, 3), f32)
    dest = dict(joint_rot=(g_theta, 3), global_rot=(g_theta, 0), trans=(g_trans, 0))
    g_betas = np.asarray(st["g_betas"], np.float64).copy()
    losses = np.zeros(4, f32)
    for t, (name, L) in enumerate(TERMS):
        w = weights[t]
        c = f32(f32(2.0 * w) / f32(L))
        S = 0.0
        arr, col = dest[name]
        for start, length in _ranges(clips):
            for n in range(start, start + length):
                d = np.zeros(L)
                if n > start:
                    d += x[name][n] - x[name][n - 1]
                if n + 1 < start + length:
                    d += x[name][n] - x[name][n + 1]
                    S += float(((x[name][n + 1] - x[name][n]) ** 2).sum())
                arr[n, col:col + L] = (np.float64(c) * d).astype(f32)      # the exact product, rounded once: fma(c, d, 0)
        assert float(f32(S)) == S
        losses[t] = f32(w) * (f32(S) / f32(L))
    losses[3] = (losses[0] + losses[1]) + losses[2]
    for start, length in _ranges(clips):
        if length > 1:
            g_betas[start:start + length] = g_betas[start:start + length].sum(axis=0)
    return dict(g_betas=g_betas.astype(f32), g_theta=g_theta, g_trans=g_trans, losses=losses)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
