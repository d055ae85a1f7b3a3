"""Value-edge cases for the pose maths, shared by tests/test_value_forms_cpu.py (which proves on the host that every case is
in the regime it names and that float32 arithmetic alone stays inside the fixed bars there) and tests/test_gpu_value_forms.py
(the HIP kernels against the float64 oracle).  Everything the suite compared with the oracle before drew its state from
parity_cases.random_pose (joint rotations 0.2 randn, limb log-scales 0.15 randn, z ~ 1.45, Bernoulli visibility); a fit starts
with every joint rotation exactly 0, moves through 1e-5 .. 1e-2 rad, and meets all-zero visibility rows and targets of -1.

  A. fused_cases()      states of one Engine.fit_eval call (3 frames, 64 x 64, window 2, stage-1 weights without silhouette)
  B. *_sweep / *_cases  inputs of the stand-alone operators of the C ABI, with float64 references and float32 yardsticks

Bounds (bound()): a deviation from the float64 oracle passes below the project's existing bar for the quantity, or below
YARD x the float32 ORACLE's own deviation on the same inputs where that is larger -- float32 arithmetic alone is worth that much
and the reference has it too (tests/test_gpu_eval_fixtures.py).  Nothing here imports the GPU at module level."""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle import smal_oracle as so
from smalify_amd import config as cfg
from smalify_amd import model_io, synthetic
from tests import parity_cases as pc

YARD = 2.0
RATCHET = 3.0
FLOOR_VALUE, FLOOR_GRAD = 1e-6, 1e-5
BAR = {"rodrigues_fwd": 2e-6, "rodrigues_bwd": 2e-5, "chain": 2e-5, "camera": 2e-5, "term": 1e-4, "grad": 5e-4, "adam": 1e-6}
# The one bar that is not an existing one.  The antisymmetric part of R is sin(a) r: at small angles it is the WHOLE rotation (about
# theta itself) while the forward's 2e-6 max-abs sees nothing below 1e-6 rad -- an axis taken from theta + 1e-8 instead of theta is
# an absolute error of 1e-8 in R.  It is the product of four float32 results (1 / a, theta / a, sinf, the product), each good to
# an ulp or two, so 8 float32 epsilons relative; where the symmetric part (1 - cos a) r r^T is the larger one (towards pi) its
# rounding is left in the difference R - R^T and the float32 oracle's own deviation takes over.
BAR["rodrigues_skew"] = 8 * float(np.finfo(np.float32).eps)
# final parameters of a sharded fit (tests/test_gpu_shard_step.py): against the unsharded HIP fit tests/test_gpu_sharded.py's bar,
# against the float64 oracle loop north_star's
BAR["sharded_vs_unsharded"], BAR["fit_vs_oracle"] = 2e-5, 1e-4

M, S, WINDOW, W_TEMP = 3, 64, 2, 100.0
LOSS_NAMES = ("joint", "pose", "splay", "betas", "sil_reproj", "temp_joint", "temp_global", "temp_trans", "limit")
PARAMS = ("betas", "log_beta_scales", "global_rotation", "joint_rotations", "trans")
SENTINEL = 12345.0
PAD = 64


def bound(kind, yard):
    """the larger of the existing bar and YARD x the float32 oracle's own deviation"""
    return max(BAR[kind], YARD * (yard if yard == yard else 0.0))


def rel(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def unit_rows(rs, n):
    d = rs.randn(n, 3)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def axis_rows(n, start=0):
    """axis-aligned unit rows: two components exactly zero (every third row holds them as -0.0), signs alternating"""
    d = np.zeros((n, 3))
    for i in range(n):
        if (i + start) % 3 == 2:
            d[i] = -0.0
        d[i, (i + start) % 3] = 1.0 if (i + start) % 2 == 0 else -1.0
    return d


# ------------------------------------------------------------------------------------------------
# A. fused evaluation
# ------------------------------------------------------------------------------------------------
def stage1_weights():
    w = np.array(cfg.OPT_WEIGHTS).T[1][:6].astype(np.float64).copy()
    w[1] = 0.0                # no silhouette term: the oracle needs no rasteriser
    w[4] = 0.0                # the limit column only counts in the `limits` case
    return w


_BASE = {}


def base_state(frames=M, seed=61):
    """the random state every case starts from: (params, target joints, visibility), float32.  Targets are the projection of
    a ground-truth random_pose plus unit noise, as in parity_cases.make_problem_cpu"""
    if (frames, seed) not in _BASE:
        _, cur, tg = pc.make_problem_cpu(frames, S, WINDOW, seed, with_sil=False)
        _BASE[(frames, seed)] = ({k: np.ascontiguousarray(v, np.float32) for k, v in cur.items()},
                                 np.ascontiguousarray(tg["tj"], np.float32), np.ascontiguousarray(tg["vis"], np.float32))
    p, tj, vis = _BASE[(frames, seed)]
    return {k: v.copy() for k, v in p.items()}, tj.copy(), vis.copy()


def _case(name, p, tj, vis, weights=None, w_temp=W_TEMP, limits=None):
    return dict(name=name, params={k: np.ascontiguousarray(v, np.float32) for k, v in p.items()},
                tj=np.ascontiguousarray(tj, np.float32), vis=np.ascontiguousarray(vis, np.float32),
                weights=stage1_weights() if weights is None else np.asarray(weights, np.float64), w_temp=float(w_temp), limits=limits)


DECADES = tuple(10.0 ** (-7 + k) for k in range(7))
BAND = 3e-4
AXIS_MAGNITUDES = (1e-5, 3e-4, 0.2, math.pi)
NEAR_PI = {3: math.pi - 1e-3, 9: math.pi, 14: math.pi + 1e-3, 20: 2 * math.pi, 27: 2 * math.pi + 0.3, 32: 4.0}
BIG_SCALES = (1.5, -1.5, 1.0, -1.0, 0.7, -0.7)
NEAR_PLANE_Z = 2.55
WEIGHT_COLUMNS = {"w_j2d": 0, "w_betas": 2, "w_pose": 3, "w_splay": 5}       # columns of (w_j2d, w_sil, w_betas, w_pose, w_limit, w_splay)
WEIGHT_SLOTS = {"w_j2d": ("joint",), "w_betas": ("betas",), "w_pose": ("pose",), "w_splay": ("splay",),
                "w_temp": ("temp_joint", "temp_global", "temp_trans")}
W_LIMIT = 100.0
LIMIT_KINDS = ("at_hi", "at_lo", "hi_in", "hi_out", "lo_in", "lo_out", "far_out", "inside")


FUSED_NAMES = ("rest", "decades", "band", "axis", "near_pi", "big_shape", "near_plane", "visibility", "identical", "one_frame",
               "weights_off/w_j2d", "weights_off/w_betas", "weights_off/w_pose", "weights_off/w_splay", "weights_off/w_temp",
               "weights_off/all", "limits")


def limit_placement():
    """(rotations (M,34,3) float32, kinds (M,34,3) of LIMIT_KINDS indices or -1 where the table has no limit): every finite
    entry of the table gets one placement, the pattern shifted by one from frame to frame"""
    lo, hi = model_io.joint_limit_table()
    lo, hi = np.asarray(lo, np.float32).reshape(34, 3), np.asarray(hi, np.float32).reshape(34, 3)
    x = np.zeros((M, 34, 3), np.float32)
    kinds = -np.ones((M, 34, 3), np.int64)
    up, down = np.float32(np.inf), np.float32(-np.inf)
    for f in range(M):
        k = f
        for j in range(34):
            for a in range(3):
                l, h = lo[j, a], hi[j, a]
                if not (np.isfinite(l) and np.isfinite(h) and l < h):
                    continue
                kind = k % len(LIMIT_KINDS)
                x[f, j, a] = (h, l, np.nextafter(h, down), np.nextafter(h, up), np.nextafter(l, up), np.nextafter(l, down),
                              (h + np.float32(0.5)) if (k // len(LIMIT_KINDS)) % 2 == 0 else (l - np.float32(0.5)),
                              np.float32(0.5) * (l + h))[kind]
                kinds[f, j, a] = kind
                k += 1
    return x, kinds, lo, hi


def fused_cases():
    """{name: case}: the states of section A (weights_off and one_frame are families: weights_off/<column>, one_frame)"""
    out = {}
    rs = np.random.RandomState(71)

    p, tj, vis = base_state()
    for k in ("global_rotation", "joint_rotations", "betas", "log_beta_scales"):
        p[k][...] = 0.0
    out["rest"] = _case("rest", p, tj, vis)

    p, tj, vis = base_state()
    for j in range(34):
        p["joint_rotations"][:, j] = unit_rows(rs, M) * DECADES[j % 7]
    out["decades"] = _case("decades", p, tj, vis)

    p, tj, vis = base_state()
    p["joint_rotations"][...] = (unit_rows(rs, M * 34) * BAND).reshape(M, 34, 3)
    out["band"] = _case("band", p, tj, vis)

    p, tj, vis = base_state()
    mags = np.array([AXIS_MAGNITUDES[(f + j) % 4] for f in range(M) for j in range(34)])
    p["joint_rotations"][...] = (axis_rows(M * 34) * mags[:, None]).reshape(M, 34, 3)
    out["axis"] = _case("axis", p, tj, vis)

    p, tj, vis = base_state()
    for j, a in NEAR_PI.items():
        p["joint_rotations"][:, j] = unit_rows(rs, M) * a
    g = p["global_rotation"][1].astype(np.float64)
    p["global_rotation"][1] = g / np.linalg.norm(g) * math.pi
    out["near_pi"] = _case("near_pi", p, tj, vis)

    p, tj, vis = base_state()
    p["log_beta_scales"][...] = BIG_SCALES
    p["betas"][...] = 2.0 * np.where(rs.rand(20) < 0.5, -1.0, 1.0)
    out["big_shape"] = _case("big_shape", p, tj, vis)

    for seed in range(61, 81):      # the first random state that straddles the plane with no keypoint closer to it than 0.02
        p, tj, vis = base_state(seed=seed)
        p["trans"][:, 2] = NEAR_PLANE_Z
        out["near_plane"] = _case("near_plane", p, tj, vis)
        zv = keypoint_depths(out["near_plane"])
        if (zv > 0).any() and (zv < 0).any() and np.abs(zv).min() >= 0.025:
            break

    p, tj, vis = base_state()
    vis[0] = 1.0
    vis[1] = 0.0
    vis[2] = 0.0
    vis[2, :3] = 1.0
    vis[0, 4], vis[2, 1] = 0.5, 2.0                 # the reference's .bool(): non-zero means visible
    tj[1, :, :] = -1.0                              # what the loaders write for an unannotated keypoint
    tj[1, 5], tj[1, 6], tj[2, 7], tj[2, 8] = (1e4, -1e4), (-1e4, 1e4), (1e4, 1e4), (-1e4, -1.0)
    tj[0, 9] += (1e3, -1e3)                         # a visible target far off the image: a large residual
    out["visibility"] = _case("visibility", p, tj, vis)

    p, tj, vis = base_state()
    for k in ("global_rotation", "joint_rotations", "trans"):
        p[k][1] = p[k][0]
    out["identical"] = _case("identical", p, tj, vis)

    p, tj, vis = base_state()
    p1 = {k: (v[:1] if k in ("global_rotation", "joint_rotations", "trans") else v) for k, v in p.items()}
    out["one_frame"] = _case("one_frame", p1, tj[:1], vis[:1])

    for col in WEIGHT_SLOTS:
        p, tj, vis = base_state()
        w = stage1_weights()
        if col == "w_temp":
            out["weights_off/" + col] = _case("weights_off/" + col, p, tj, vis, w, 0.0)
        else:
            w[WEIGHT_COLUMNS[col]] = 0.0
            out["weights_off/" + col] = _case("weights_off/" + col, p, tj, vis, w)
    p, tj, vis = base_state()
    out["weights_off/all"] = _case("weights_off/all", p, tj, vis, np.zeros(6), 0.0)

    p, tj, vis = base_state()
    x, kinds, lo, hi = limit_placement()
    placed = kinds >= 0
    p["joint_rotations"][placed] = x[placed]
    w = stage1_weights()
    w[4] = W_LIMIT
    out["limits"] = _case("limits", p, tj, vis, w, limits=(lo, hi))
    return out


_ORACLE_MODELS = {}


def oracle_model(dtype):
    if dtype not in _ORACLE_MODELS:
        md, om = pc.get_oracle_model()
        _ORACLE_MODELS[dtype] = om if dtype == torch.float64 else so.OracleModel(md, dtype=dtype)
    return _ORACLE_MODELS[dtype]


def keypoint_depths(case):
    """z_view of the 25 keypoints of every frame (float64 oracle)"""
    p = case["params"]
    n = p["global_rotation"].shape[0]
    theta = torch.from_numpy(np.concatenate([p["global_rotation"][:, None], p["joint_rotations"]], 1)).double()
    with torch.no_grad():
        _, j, _, _ = so.smal_forward(oracle_model(torch.float64), torch.from_numpy(np.tile(p["betas"], (n, 1))).double(), theta,
                                     torch.from_numpy(np.tile(p["log_beta_scales"], (n, 1))).double())
    return (so.CAM_DIST - (j[:, so.CANONICAL, 2] + torch.from_numpy(p["trans"]).double()[:, None, 2])).numpy()


def limit_tie_correction(case):
    """what the oracle's autograd adds to d/d joint_rotations at rotations EXACTLY at a limit: torch.max(x, 0) splits the tie,
    slope 1/2, where the kernel's convention is `flat at the limit`, slope 0.  Returns the (M,34,3) array to SUBTRACT from the
    oracle's gradient: +-0.5 w_limit / (102 B_n) at the ties (B_n: frames in the frame's window), 0 elsewhere."""
    x = case["params"]["joint_rotations"]
    out = np.zeros(x.shape, np.float64)
    if case["limits"] is None or case["weights"][4] <= 0:
        return out
    lo, hi = case["limits"]
    n = x.shape[0]
    for f in range(n):
        start = (f // WINDOW) * WINDOW
        bn = min(WINDOW, n - start)
        k = 0.5 * case["weights"][4] / (102.0 * bn)
        out[f][x[f] == hi] += k
        out[f][x[f] == lo] -= k
    return out


_REFERENCES = {}


def oracle_eval(case, dtype=torch.float64):
    """(terms (9,) in LOSS_NAMES order, {tensor: gradient}) of the oracle in `dtype`, every tensor trainable; computed once per
    (case, dtype) and shared.  The joint-limit ties carry the kernel's documented convention (limit_tie_correction)."""
    key = (case["name"], dtype)
    if key not in _REFERENCES:
        pp, sp = synthetic.synthetic_pose_prior(), synthetic.synthetic_shape_prior()
        n = case["tj"].shape[0]
        prob = so.FitProblem(oracle_model(dtype), S, case["tj"], case["vis"], np.zeros((n, S, S), np.float32), pp[0], pp[1], pp[2],
                             sp[0], sp[1], WINDOW, use_unity_prior=True, dtype=dtype, joint_limits=case["limits"])
        params = {k: torch.from_numpy(v).to(dtype) for k, v in case["params"].items()}
        _, sums, grads = so.loss_and_grads(prob, params, case["weights"], case["w_temp"], PARAMS)
        terms = np.array([float(sums.get(t, 0.0)) for t in LOSS_NAMES], np.float64)
        g = {k: (grads[k].double().numpy().copy() if k in grads else np.zeros(case["params"][k].shape)) for k in PARAMS}
        g["joint_rotations"] = g["joint_rotations"] - limit_tie_correction(case)
        _REFERENCES[key] = (terms, g)
    return _REFERENCES[key]


def fused_deviations(terms, grads, ref_terms, ref_grads):
    """{quantity: (deviation, bar kind)} of one evaluation against the float64 reference: every term held to ITSELF, or to
    1e-3 x the objective when it is a negligible part of it (tests/test_gpu_eval_fixtures.py); the total; every gradient tensor
    as rel-L2; d/d joint_rotations per joint over that joint's M x 3 entries -- one rel-L2 over all joints is dominated by the
    joints with large gradients.  A joint whose reference norm is below 1e-6 of the tensor's is held to that floor instead:
    its absolute error over 1e-6 x the tensor's norm."""
    terms, ref_terms = np.asarray(terms, np.float64), np.asarray(ref_terms, np.float64)
    out = {}
    scale = abs(ref_terms.sum())
    for i, t in enumerate(LOSS_NAMES):
        if ref_terms[i] == 0.0 and terms[i] == 0.0:
            continue
        out["term/" + t] = (abs(terms[i] - ref_terms[i]) / max(abs(ref_terms[i]), 1e-3 * scale, 1e-30), "term")
    if scale > 0 or terms.sum() != 0:
        out["total"] = (abs(terms.sum() - ref_terms.sum()) / max(scale, 1e-30), "term")
    for k in PARAMS:
        a, b = np.asarray(grads[k], np.float64).reshape(ref_grads[k].shape), ref_grads[k]
        if not a.any() and not b.any():
            continue
        out["grad/" + k] = (rel(a, b), "grad")
    a, b = np.asarray(grads["joint_rotations"], np.float64).reshape(ref_grads["joint_rotations"].shape), ref_grads["joint_rotations"]
    whole = np.linalg.norm(b)
    if whole > 0:
        for j in range(34):
            out["grad/joint_rotations[%02d]" % j] = (float(np.linalg.norm(a[:, j] - b[:, j]) / max(np.linalg.norm(b[:, j]), 1e-6 * whole)), "grad")
    return out


# ------------------------------------------------------------------------------------------------
# B. stand-alone operators
# ------------------------------------------------------------------------------------------------
RODRIGUES_MAGNITUDES = (0.0, 1e-8, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 3e-4, 3e-3, 0.1, 1.0, math.pi - 1e-3, math.pi, math.pi + 1e-3,
                        2 * math.pi, 4 * math.pi + 0.5)
RODRIGUES_LABELS = {math.pi - 1e-3: "pi-1e-3", math.pi: "pi", math.pi + 1e-3: "pi+1e-3", 2 * math.pi: "2pi", 4 * math.pi + 0.5: "4pi+0.5"}
RODRIGUES_ROWS = 256
RODRIGUES_COUNTS = (1, 255, 256, 257, 1025)
RODRIGUES_COUNT_MAGNITUDE = 0.2


def magnitude_label(m):
    return RODRIGUES_LABELS.get(m, "%g" % m)


def rodrigues_sweep():
    """[(magnitude, kind, theta (256,3) float32, G (256,3,3) float32)]: kinds `random` and `axis` (two zero components)"""
    rs = np.random.RandomState(83)
    out = []
    for m in RODRIGUES_MAGNITUDES:
        for kind in ("random", "axis"):
            d = unit_rows(rs, RODRIGUES_ROWS) if kind == "random" else axis_rows(RODRIGUES_ROWS)
            out.append((m, kind, np.ascontiguousarray(d * m, np.float32), rs.randn(RODRIGUES_ROWS, 3, 3).astype(np.float32)))
    return out


def rodrigues_count_case(count):
    rs = np.random.RandomState(89 + count)
    return (np.ascontiguousarray(unit_rows(rs, count) * RODRIGUES_COUNT_MAGNITUDE, np.float32), rs.randn(count, 3, 3).astype(np.float32))


def rodrigues_oracle(theta, G, dtype=torch.float64):
    """(R (n,3,3), d/d theta of <G, R>) of the oracle in `dtype`, as float64 arrays"""
    t = torch.from_numpy(theta).to(dtype).requires_grad_(True)
    R = so.rodrigues(t)
    (R * torch.from_numpy(G).to(dtype)).sum().backward()
    return R.detach().double().numpy(), t.grad.double().numpy()


def skew_part(R):
    """(n,3) axial vector of (R - R^T) / 2 = sin(a) r"""
    return 0.5 * np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], 1)


def rodrigues_deviations(R, dth, theta, G):
    """-> ((forward max-abs, adjoint rel-L2, rel-L2 of the forward's antisymmetric part) of the result, the same of the float32
    oracle, the float64 adjoint), against the float64 oracle"""
    R64, d64 = rodrigues_oracle(theta, G)
    R32, d32 = rodrigues_oracle(theta, G, torch.float32)
    R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    return ((float(np.abs(R - R64).max()), rel(dth, d64), rel(skew_part(R), skew_part(R64))),
            (float(np.abs(R32 - R64).max()), rel(d32, d64), rel(skew_part(R32), skew_part(R64))), d64)


CHAIN_COUNTS = (1, 63, 64, 65, 130)
CHAIN_SCALES = (None, 0.3, 3.0)


def chain_case(count, scale):
    """Rs from rotations that hold the near-pi magnitudes, Js, log scales of +-scale with random signs (None: no scales) and
    the upstream gradients, all float32"""
    rs = np.random.RandomState(97 + count)
    th = 0.5 * rs.randn(count, 35, 3)
    for j, a in NEAR_PI.items():
        th[:, j] = unit_rows(rs, count) * a
    Rs = so.rodrigues(torch.from_numpy(th.reshape(-1, 3))).reshape(count, 35, 3, 3).float().numpy().copy()
    Js = (0.3 * rs.randn(count, 35, 3)).astype(np.float32)
    ls = None if scale is None else (scale * np.where(rs.rand(count, 6) < 0.5, -1.0, 1.0)).astype(np.float32)
    return dict(Rs=Rs, Js=Js, ls=ls, dnewJ=rs.randn(count, 35, 3).astype(np.float32), dA=rs.randn(count, 35, 4, 4).astype(np.float32))


def chain_oracle(c, parents, dtype=torch.float64):
    """{newJ, A, dRs, dJs, dls} of so.kinematic_chain in `dtype` with the weighting of
    test_global_rigid_transformation_adjoint_host, as float64 arrays"""
    R = torch.from_numpy(c["Rs"]).to(dtype).requires_grad_(True)
    J = torch.from_numpy(c["Js"]).to(dtype).requires_grad_(True)
    L = torch.from_numpy(c["ls"]).to(dtype).requires_grad_(True) if c["ls"] is not None else None
    g_t, g_r, a_t = so.kinematic_chain(R, J, [int(p) for p in parents], L)
    dA = torch.from_numpy(c["dA"]).to(dtype)
    ((g_t * torch.from_numpy(c["dnewJ"]).to(dtype)).sum() + (g_r * dA[:, :, :3, :3]).sum() + (a_t * dA[:, :, :3, 3]).sum()).backward()
    n = R.shape[0]
    A = torch.zeros(n, 35, 4, 4, dtype=dtype)
    A[:, :, :3, :3], A[:, :, :3, 3], A[:, :, 3, 3] = g_r.detach(), a_t.detach(), 1.0
    out = {"newJ": g_t.detach(), "A": A, "dRs": R.grad, "dJs": J.grad}
    if L is not None:
        out["dls"] = L.grad
    return {k: v.double().numpy() for k, v in out.items()}


PROJECT_SHAPES = ((1, 1), (1, 25), (1, 300), (3, 1), (3, 25), (3, 300))
PROJECT_DEPTHS = (1.0, 0.1, 0.05, -0.05)


def project_case(frames, P):
    """points (frames, P, 3) whose z_view cycles through PROJECT_DEPTHS, upstream gradient (frames, P, 2), depth index per point"""
    rs = np.random.RandomState(101 + 7 * frames + P)
    n = frames * P
    which = (np.arange(n) + P) % len(PROJECT_DEPTHS)
    pts = np.concatenate([0.3 * rs.randn(n, 2), (so.CAM_DIST - np.array(PROJECT_DEPTHS)[which])[:, None]], 1).astype(np.float32)
    return pts.reshape(frames, P, 3), rs.randn(frames, P, 2).astype(np.float32), which


def project_oracle(pts, g, dtype=torch.float64):
    t = torch.from_numpy(pts).to(dtype).requires_grad_(True)
    proj = so.project_points(t, S)
    (proj * torch.from_numpy(g).to(dtype)).sum().backward()
    return proj.detach().double().numpy(), t.grad.double().numpy()


PRIOR_COUNTS = (1, 2, 64, 200)


def prior_case(N, mean, seed=103):
    """x (N,105): row 0 alternates +-pi, row 1 its negative, row 2 the mean itself, the rest random; and the upstream gradient"""
    rs = np.random.RandomState(seed + N)
    x = (0.3 * rs.randn(N, 105)).astype(np.float32)
    x[0, ::2], x[0, 1::2] = np.float32(math.pi), np.float32(-math.pi)
    if N > 1:
        x[1] = -x[0]
    if N > 2:
        x[2] = mean
    return x, rs.randn(N, 105).astype(np.float32)


def prior_oracle(x, dout, prior, dtype=torch.float64):
    prec, mean, mask = (torch.from_numpy(np.asarray(a, np.float32)).to(dtype) for a in prior)
    t = torch.from_numpy(x).to(dtype).requires_grad_(True)
    out = so.pose_prior_residual2(t, prec, mean, mask)
    (out * torch.from_numpy(dout).to(dtype)).sum().backward()
    return out.detach().double().numpy(), t.grad.double().numpy()


def temporal_case(N, identical=False, seed=107):
    rs = np.random.RandomState(seed + N)
    g, j, t = (0.3 * rs.randn(N, 3)).astype(np.float32), (0.2 * rs.randn(N, 34, 3)).astype(np.float32), (0.1 * rs.randn(N, 3)).astype(np.float32)
    if identical and N > 1:
        g[1], j[1], t[1] = g[0], j[0], t[0]
    gm = np.array([1.0, 0.0, 1.0], np.float32)
    rm = (rs.rand(34, 3) < 0.7).astype(np.float32)
    rm[0] = 0.0
    return g, j, t, gm, rm


def temporal_oracle(g, j, t, gm, rm, w_temp, dtype=torch.float64):
    """(losses (3,) joint, global, trans; gradients wrt the RAW parameters) with the masks applied as the fitter does"""
    G, J, T = (torch.from_numpy(a).to(dtype).requires_grad_(True) for a in (g, j, t))
    p = {"global_rotation": G if gm is None else G * torch.from_numpy(gm).to(dtype),
         "joint_rotations": J if rm is None else J * torch.from_numpy(rm).to(dtype), "trans": T}
    jl, gl, tl = so.temporal_terms(p, w_temp)
    (jl + gl + tl).backward()
    z = lambda a: np.zeros(a.shape) if a.grad is None else a.grad.double().numpy()  # noqa: E731
    return np.array([float(x.detach()) for x in (jl, gl, tl)]), z(G), z(J), z(T)


ADAM_COUNTS = (1, 255, 256, 257)
ADAM_STEPS = (1, 2, 1000)
ADAM_HYPER = (0.02, 0.5, 0.999, 1e-8)


def adam_case(count, t, seed=109):
    """(p, g, m, v) float32: gradients of exactly 0, 1e-20 and 1e+15 with mixed signs among random ones; zero moments at
    t = 1, and at the exactly-zero gradients for every t (there the parameter must not move)"""
    rs = np.random.RandomState(seed + 13 * count + t)
    p = rs.randn(count).astype(np.float32)
    g = (rs.randn(count) * 10.0 ** rs.uniform(-3, 1, count)).astype(np.float32)
    kind = (np.arange(count) + t) % 7
    sign = np.where(rs.rand(count) < 0.5, -1.0, 1.0)
    g[kind == 0] = 0.0
    g[kind == 1] = (1e-20 * sign[kind == 1]).astype(np.float32)
    g[kind == 2] = (1e15 * sign[kind == 2]).astype(np.float32)
    m = (rs.randn(count) * 0.1).astype(np.float32)
    v = (rs.rand(count) * 0.1).astype(np.float32)
    if t == 1:
        m[:], v[:] = 0.0, 0.0
    m[kind == 0], v[kind == 0] = 0.0, 0.0
    return p, g, m, v, kind == 0


def adam_reference(p, g, m, v, t, hyper=ADAM_HYPER):
    """the float64 replica of torch.optim.Adam's update (tests/test_host_math.py::test_adam_host) from float32 inputs"""
    lr, b1, b2, eps = (float(np.float32(x)) for x in hyper)
    p, g, m, v = (a.astype(np.float64) for a in (p, g, m, v))
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    p = p - lr / (1 - b1 ** t) * m / (np.sqrt(v) / math.sqrt(1 - b2 ** t) + eps)
    return p, m, v


# segments of smalfit_adam_segments over a flat buffer of ADAM_FLAT floats: 1 to 4 ranges, one of them empty
ADAM_FLAT = 900
ADAM_SEGMENT_SETS = (((3, 258),), ((0, 1), (10, 10)), ((5, 261), (300, 300), (301, 558)), ((0, 255), (256, 257), (400, 400), (600, 857)))
