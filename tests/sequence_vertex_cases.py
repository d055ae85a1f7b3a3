"""Cases and restatements of the temporal terms on posed vertices (include/smalfit.h, "scan sequences", the vertex terms), shared by
the CPU and the GPU tests: random vertex arrays per clip layout and V, the float64 numpy restatement, the same terms in torch
with autograd (per clip), the dyadic case with its closed form, uniform motion, and the float32 bar.  Nothing here needs a GPU."""
from __future__ import annotations

import json
import os

import numpy as np
import torch

CLIPS = ((1,), (2,), (3,), (4,), (5,), (2, 1), (1, 3, 1), (3, 2))
VERTS = (1, 255, 256, 257)                     # one vertex; a block less one, a full block, a block and one
WEIGHTS = (0.7, 1.9)                           # velocity, acceleration
WEIGHT_SETS = ((0.7, 0.0), (0.0, 1.9), WEIGHTS)       # each weight alone, and both
MEASURED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hip_fit3d_sequence_vertex_measured.json")
RATCHET = 3.0                                  # the project's: a bar is three times the measured float32 deviation


def clip_id(clips):
    return "clips" + "-".join(str(c) for c in clips)


def verts(clips, V, seed=0):
    """(N, V, 3) float32: one blob per clip, moving and deforming a little from mesh to mesh"""
    N = int(sum(clips))
    rng = np.random.default_rng(2000 + 17 * seed + 131 * N + 7 * len(clips) + V)
    base = 0.3 * rng.standard_normal((1, V, 3))
    drift = 0.05 * np.cumsum(rng.standard_normal((N, 1, 3)), axis=0)
    wobble = 0.02 * rng.standard_normal((N, V, 3))
    return (base + drift + wobble).astype(np.float32)


def _ranges(clips):
    start = 0
    for length in clips:
        yield start, int(length)
        start += int(length)


def reference64(clips, x, weights=WEIGHTS):
    """the definitions restated in float64 numpy -> dict(dverts (N,V,3), dtrans (N,3), losses (3,))"""
    x = np.asarray(x, np.float64)
    N, V = x.shape[:2]
    L = 3.0 * V
    wv, wa = (float(w) for w in weights)
    g = np.zeros_like(x)
    losses = np.zeros(3)
    for start, length in _ranges(clips):
        if wv > 0:
            for n in range(start, start + length - 1):
                d = x[n + 1] - x[n]
                losses[0] += wv * float((d * d).sum()) / L
                g[n] -= 2.0 * wv / L * d
                g[n + 1] += 2.0 * wv / L * d
        if wa > 0:
            for n in range(start + 1, start + length - 1):
                a = (x[n - 1] - x[n]) + (x[n + 1] - x[n])
                losses[1] += wa * float((a * a).sum()) / L
                g[n - 1] += 2.0 * wa / L * a
                g[n] -= 4.0 * wa / L * a
                g[n + 1] += 2.0 * wa / L * a
    losses[2] = losses[0] + losses[1]
    return dict(dverts=g, dtrans=g.sum(axis=1), losses=losses)


def reference_torch(clips, x, weights=WEIGHTS, dtype=torch.float64):
    """the same terms in torch, clip by clip: F.mse_loss(x[n], x[n + 1]) * w over the pairs, F.mse_loss of the second difference
    against zero * w over the centres; the gradient by autograd, d trans as its sum over the vertices, all in `dtype`
    -> dict(dverts, dtrans, losses (3,)) as float64 numpy"""
    import torch.nn.functional as F
    X = torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True)
    terms = [torch.zeros((), dtype=dtype), torch.zeros((), dtype=dtype)]
    for start, length in _ranges(clips):
        if weights[0] > 0:
            for n in range(start, start + length - 1):
                terms[0] = terms[0] + F.mse_loss(X[n], X[n + 1]) * weights[0]
        if weights[1] > 0:
            for n in range(start + 1, start + length - 1):
                a = (X[n - 1] - X[n]) + (X[n + 1] - X[n])
                terms[1] = terms[1] + F.mse_loss(a, torch.zeros_like(a)) * weights[1]
    total = terms[0] + terms[1]
    grad = torch.autograd.grad(total, X)[0] if total.requires_grad else torch.zeros_like(X)
    return dict(dverts=grad.detach().double().numpy(), dtrans=grad.detach().sum(dim=1).double().numpy(),
                losses=np.array([float(terms[0].detach()), float(terms[1].detach()), float(total.detach())], np.float64))


def deviation(a, ref):
    """max |a - ref| over max |ref| (the absolute error where ref is all zero)"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    err = float(np.abs(a - ref).max()) if ref.size else 0.0
    return err / scale if scale > 0 else err


def all_cases():
    for clips in CLIPS:
        for V in VERTS:
            for weights in WEIGHT_SETS:
                yield clips, V, weights


def worst(results):
    """results: iterable of (got, ref) dicts -> dict(loss=, dtrans=, grad=): the largest deviation of each kind"""
    out = dict(loss=0.0, dtrans=0.0, grad=0.0)
    for got, ref in results:
        out["loss"] = max(out["loss"], max(deviation(got["losses"][t], ref["losses"][t]) for t in range(3)))
        out["dtrans"] = max(out["dtrans"], deviation(got["dtrans"], ref["dtrans"]))
        out["grad"] = max(out["grad"], deviation(got["dverts"], ref["dverts"]))
    return out


def float32_restatement_deviation():
    """how far a plain float32 torch restatement lies from the float64 one over all_cases -> dict(loss=, dtrans=, grad=): what the
    bar is 3x of"""
    return worst((reference_torch(c, verts(c, V), w, torch.float32), reference_torch(c, verts(c, V), w, torch.float64))
                 for c, V, w in all_cases())


def measured():
    with open(MEASURED) as fh:
        return json.load(fh)


WRITE_ENV = "SMALFIT_WRITE_SEQUENCE_VERTEX_MEASURED"       # =1: write the record in place; =<path>: write it there


def record(update):
    """with WRITE_ENV set: merge `update` into the record (the file in place, or a copy of it at the path given) -> True"""
    where = os.environ.get(WRITE_ENV)
    if not where:
        return False
    path = MEASURED if where == "1" else where
    doc = {}
    for src in (path, MEASURED):
        if os.path.exists(src):
            with open(src) as fh:
                doc = json.load(fh)
            break
    doc.update(update)
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    return True


def record_float32_restatement(host_shim_worst):
    """the CPU half of the record: the float32 torch restatement's deviation, the bar it sets, the host shim's own deviation"""
    dev = float32_restatement_deviation()
    return record({
        "what": "temporal terms on posed vertices: the float32 bar of tests/sequence_vertex_cases.py and what was measured against it",
        "cases": "tests/sequence_vertex_cases.py CLIPS x VERTS x WEIGHT_SETS on verts(clips, V, seed=0); the GPU also GPU_VERTS and GPU_CLIPS",
        "metric": "max |a - ref| / max |ref| against the float64 restatement, the largest over the cases",
        "float32_restatement_deviation": dev,
        "ratchet": RATCHET,
        "bar": {k: RATCHET * v for k, v in dev.items()},
        "host_shim_vs_float64": host_shim_worst})


def bars():
    """-> dict(loss=, dtrans=, grad=): RATCHET times the recorded float32 deviation
    (tests/golden/hip_fit3d_sequence_vertex_measured.json)"""
    m = measured()["float32_restatement_deviation"]
    return {k: RATCHET * m[k] for k in ("loss", "dtrans", "grad")}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the dyadic case: every coordinate a multiple of 2^-6 and both c = (2 w) / (3 V) a power of two, so every sum is exact --------
DYADIC_CLIPS = (1, 5, 3, 2)
DYADIC_VERTS = (5, 257)


def dyadic_weights(V):
    """w = 3 V / 8 and 3 V / 32: c_vel = 1/4 and c_acc = 1/16 exactly"""
    return (3.0 * V / 8.0, 3.0 * V / 32.0)


def dyadic_verts(V, clips=DYADIC_CLIPS):
    N = int(sum(clips))
    rng = np.random.default_rng(11 + V)
    return (rng.integers(-32, 33, size=(N, V, 3)) / 64.0).astype(np.float32)


def dyadic_closed_form(V, clips=DYADIC_CLIPS, weights=None):
    """exact arithmetic in float64 (every intermediate is a dyadic rational of few bits; asserted), rounded to float32 where the
    definition rounds and the value is not exact: the quotient S / L and its product with w"""
    f32 = np.float32
    weights = dyadic_weights(V) if weights is None else weights
    x = np.asarray(dyadic_verts(V, clips), np.float64)
    N = x.shape[0]
    L = f32(3 * V)
    c = [float(f32(f32(2.0) * f32(w)) / L) if w > 0 else 0.0 for w in weights]
    assert all(ci == 0.0 or np.log2(ci) == int(np.log2(ci)) for ci in c)          # powers of two: every product below is exact
    t = np.zeros_like(x)
    S = [0.0, 0.0]
    for start, length in _ranges(clips):
        a = np.zeros_like(x)
        for n in range(start + 1, start + length - 1):
            a[n] = (x[n - 1] - x[n]) + (x[n + 1] - x[n])
        for n in range(start, start + length):
            D = np.zeros_like(x[n])
            A = -2.0 * a[n]
            if n > start:
                D += x[n] - x[n - 1]
                A += a[n - 1]
            if n + 1 < start + length:
                D += x[n] - x[n + 1]
                A += a[n + 1]
                S[0] += float(((x[n + 1] - x[n]) ** 2).sum())
            S[1] += float((a[n] ** 2).sum())
            t[n] = c[1] * A + c[0] * D
    dtrans = t.sum(axis=1)
    assert np.array_equal(t.astype(f32).astype(np.float64), t) and np.array_equal(dtrans.astype(f32).astype(np.float64), dtrans)
    assert all(float(f32(s)) == s for s in S)
    losses = np.zeros(3, f32)
    for i in range(2):
        losses[i] = f32(weights[i]) * (f32(S[i]) / L) if weights[i] > 0 else f32(0)
    losses[2] = losses[0] + losses[1]
    return dict(dverts=t.astype(f32), dtrans=dtrans.astype(f32), losses=losses)


def uniform_motion(clips, V):
    """x[n] = x0 + n u with dyadic x0 and u: every acceleration is exactly 0"""
    N = int(sum(clips))
    rng = np.random.default_rng(5 + V)
    x0 = rng.integers(-32, 33, size=(1, V, 3)) / 64.0
    u = rng.integers(-8, 9, size=(1, 1, 3)) / 64.0
    u[0, 0, 0] = 3.0 / 64.0                                                            # (never standing still)
    return (x0 + np.arange(N)[:, None, None] * u).astype(np.float32)
