"""The expected values and the cases of the Geman-McClure robust kernel on both data terms (smalfit_robust_args,
smalfit_mesh_objective_eval_robust, smalfit_mesh_surface_eval_robust, smalfit_fit3d_step_robust), shared by
tests/test_robust_cpu.py (the host shim) and tests/test_gpu_robust.py (HIP through the C-ABI).  Nothing here asserts or needs a
GPU.  Test infrastructure, not the library: a numpy brute force written from the definitions include/smalfit.h words:

  s^2            sigma sigma, the float32 product (a scale is off when sigma <= 0 or not finite, and for a skipped direction)
  u, rho, w      u = s^2 / (s^2 + d^2), rho = d^2 u, w = u u for a KEPT match; off: rho = d^2, w = 1
  matching       that of the gated terms (tests/chamfer_gate_cases.py, tests/surface_gate_cases.py), untouched
  chamfer        1/(N S) sum over kept s of rho + 1/(N V) sum over kept v of rho;
                 d / d y_v = w_chamfer [2/(N V) [v kept] w(d^2_v) (y_v - x_nn'(v)) + 2/(N S) sum over kept s with nn(s) = v of w(d^2_s) (y_v - x_s)]
  surface term   L_ps, L_vs sum rho; a vertex receives w_vs 2/(N V) w r, the corners of a point's face -w_ps 2/(N S) w b_i r
  weight sums    per mesh the sum of w over the kept points | kept vertices; a skipped direction 0

evaluated in float64 (the oracle) or, by the same code, in float32 (the yardstick).  The flag rules are the gated terms' own."""
from __future__ import annotations

import ctypes as C

import numpy as np

from smalify_amd import _lib
from tests import chamfer_gate_cases as cc
from tests import mesh_score_cases as mc
from tests import surface_gate_cases as gc

KEYS = ("sigma_chamfer_point", "sigma_chamfer_vert", "sigma_surface_point", "sigma_surface_vert")
FLAG_CAP = 0.03                     # of a scene's queries, on the oracle alone
ROUNDINGS = 8                       # float32 roundings of at most 2^-24 each between the inputs and a weight: 4.8e-7 < WEIGHT_BAR
WEIGHT_BAR = 1e-6                   # relative, per-query weights and rho against float64 on the same correspondence
W_D_MAX = 3.0 * np.sqrt(3.0) / 16.0   # max over d of w(d^2) d = (3 sqrt 3 / 16) sigma, reached at d = sigma / sqrt 3


def scales(**kw):
    out = dict.fromkeys(KEYS, 0.0)
    out.update(kw)
    return out


def scale_on(sigma):
    s = np.float32(sigma)
    return bool(s > 0 and np.isfinite(s))


def s2_of(sigma):
    """sigma^2 as the host forms it (float32)"""
    s = np.float32(sigma)
    return np.float32(s * s)


def gm(d2, sigma, dtype=np.float64):
    """-> (rho, w) of the squared distances d2 under scale sigma; a scale that is off gives (d2, 1)"""
    d2 = np.asarray(d2, dtype)
    if not scale_on(sigma):
        return d2.copy(), np.ones_like(d2)
    s2 = dtype(s2_of(sigma))
    u = (s2 / (s2 + d2)).astype(dtype)
    return (d2 * u).astype(dtype), (u * u).astype(dtype)


def chamfer_robust(verts, faces, points, point_normals, point_boundary, w_chamfer, gates, sig, dtype=np.float64, delta=None):
    """cc.chamfer_gated's matches with the kernel on the kept ones -> its dict with chamfer, dverts, dtrans replaced and
    rho / weights per direction (lists over the meshes, 0 for a dropped query), sums (N,2) of rho, weight_sums (N,2)"""
    base = cc.chamfer_gated(verts, faces, points, point_normals, point_boundary, w_chamfer, gates or {}, dtype=dtype, delta=delta)
    verts, points = np.asarray(verts, dtype), np.asarray(points, dtype)
    N, V = verts.shape[:2]
    S = points.shape[1]
    w = dtype(max(w_chamfer, 0.0))
    on = w_chamfer > 0
    grad = np.zeros((N, V, 3), dtype)
    sums, wsums = np.zeros((N, 2), dtype), np.zeros((N, 2), dtype)
    rp, rv, wp, wv = [], [], [], []
    for n in range(N):
        p, v = base["point"][n], base["vert"][n]
        rho_p, w_p = gm(p["d2"], sig["sigma_chamfer_point"] if on else 0.0, dtype)
        rho_v, w_v = gm(v["d2"], sig["sigma_chamfer_vert"] if on else 0.0, dtype)
        rho_p, w_p = np.where(p["kept"], rho_p, 0), np.where(p["kept"], w_p, 0)
        rho_v, w_v = np.where(v["kept"], rho_v, 0), np.where(v["kept"], w_v, 0)
        rp.append(rho_p), rv.append(rho_v), wp.append(w_p), wv.append(w_v)
        sums[n] = rho_p.sum(dtype=dtype), rho_v.sum(dtype=dtype)
        wsums[n] = (w_p.sum(dtype=dtype), w_v.sum(dtype=dtype)) if on else (0, 0)
        cy, cx = w * dtype(2) / (dtype(V) * dtype(N)), w * dtype(2) / (dtype(S) * dtype(N))
        vk, pk = v["kept"], p["kept"]
        grad[n][vk] += cy * w_v[vk, None] * (verts[n][vk] - points[n][v["index"][vk]])
        np.add.at(grad[n], p["index"][pk], cx * w_p[pk, None] * (verts[n][p["index"][pk]] - points[n][pk]))
    chamfer = sums[:, 0].sum(dtype=dtype) / dtype(N * S) + sums[:, 1].sum(dtype=dtype) / dtype(N * V)
    out = dict(base)
    out.update(chamfer=chamfer, dverts=grad, dtrans=grad.sum(1, dtype=dtype), sums=sums, weight_sums=wsums, rho_point=rp, rho_vert=rv,
               w_point=wp, w_vert=wv)
    return out


def surface_robust(verts, faces, targets, points, point_normals, w_ps, w_vs, gates, sig, dtype=np.float64, delta=None):
    """gc.gated_term's matches with the kernel on the kept ones -> its dict with L_ps, L_vs, term, rows, dverts, dtrans replaced
    and w_point / w_vert (lists over the meshes), weight_sums (N,2)"""
    base = gc.gated_term(verts, faces, targets, points, point_normals, w_ps, w_vs, gates or {}, dtype=dtype, delta=delta)
    verts = np.asarray(verts, dtype)
    N, V = verts.shape[:2]
    f = np.asarray(faces, np.int64)
    rows, wsums = np.zeros((N, 2), dtype), np.zeros((N, 2), dtype)
    grad = np.zeros((N, V, 3), dtype)
    wp, wv = [], []
    two = dtype(2)
    if w_ps > 0:
        S = np.asarray(points).shape[1]
        for n in range(N):
            o = base["point"][n]
            rho, w = gm(o["d2"], sig["sigma_surface_point"], dtype)
            rho, w = np.where(o["kept"], rho, 0), np.where(o["kept"], w, 0)
            wp.append(w)
            rows[n, 0], wsums[n, 0] = rho.sum(dtype=dtype), w.sum(dtype=dtype)
            coef = dtype(w_ps) * two / (dtype(S) * dtype(N))
            fc = np.where(o["kept"], o["face"], 0)
            for i in range(3):
                np.add.at(grad[n], f[fc, i], -coef * w[:, None] * o["bary"][:, i:i + 1] * o["r"])
    if w_vs > 0:
        for n in range(N):
            o = base["vert"][n]
            rho, w = gm(o["d2"], sig["sigma_surface_vert"], dtype)
            rho, w = np.where(o["kept"], rho, 0), np.where(o["kept"], w, 0)
            wv.append(w)
            rows[n, 1], wsums[n, 1] = rho.sum(dtype=dtype), w.sum(dtype=dtype)
            grad[n] += dtype(w_vs) * two / (dtype(V) * dtype(N)) * w[:, None] * o["r"]
    L_ps = rows[:, 0].sum(dtype=dtype) / dtype(N * np.asarray(points).shape[1]) if w_ps > 0 else dtype(0)
    L_vs = rows[:, 1].sum(dtype=dtype) / dtype(N * V) if w_vs > 0 else dtype(0)
    out = dict(base)
    out.update(L_ps=L_ps, L_vs=L_vs, term=dtype(max(w_ps, 0)) * L_ps + dtype(max(w_vs, 0)) * L_vs, rows=rows, dverts=grad,
               dtrans=grad.sum(1, dtype=dtype), w_point=wp, w_vert=wv, weight_sums=wsums)
    return out


# ---------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------
NOISE = 0.15                        # the spread of random_problem's points about the vertices: the scale its tests use


def random_problem(V, S, seed, N=1):
    """N ribbons of V vertices, S points around each with random unit normals and random boundary bytes (the problem of
    tests/test_gpu_chamfer_gate.py) -> fit (N,V,3), faces, points (N,S,3), normals, boundary bytes"""
    fit = np.stack([mc.ribbon(V, seed=seed + 7 * n)[0] for n in range(N)])
    faces = mc.ribbon(V, seed=0)[1]
    rs = np.random.RandomState(seed + 300)
    pts = np.stack([(fit[n][rs.randint(0, V, S)] + NOISE * rs.randn(S, 3)).astype(np.float32) for n in range(N)])
    nrm = rs.randn(N, S, 3)
    nrm = (nrm / np.linalg.norm(nrm, axis=2, keepdims=True)).astype(np.float32)
    return fit, faces, pts, nrm, (rs.rand(N, S) < 0.3).astype(np.uint8)


QUERY_COUNTS = (1, 63, 64, 65, 130)
SCANNED_COUNTS = (1, 2, 511, 512, 513, 1023, 1024, 1025, 1027)       # the chunk edges of the gated (512) and ungated (1024) scans


def sweep():
    """(tag, V, S, seed) of the size sweep: the query counts, then every scanned count in both roles (a mesh has three vertices
    at the least)"""
    out = [("queries %d" % q, max(q, 3), q, q) for q in QUERY_COUNTS]
    for x in SCANNED_COUNTS:
        out.append(("role 0 scanned %d" % x, max(x, 3), 65, 10 * x))
        out.append(("role 1 scanned %d" % x, 65, x, 10 * x + 1))
    return out


SWEEP_SIGMA = scales(sigma_chamfer_point=NOISE, sigma_chamfer_vert=2 * NOISE)      # the points' own spread, and twice that
SWEEP_GATES = dict(max_dist_point=0.45, max_dist_vert=0.45, min_cos_point=0.0, min_cos_vert=-0.2, reject_boundary=True)
SOUP_SIGMA = scales(sigma_surface_point=0.05, sigma_surface_vert=0.3)      # the points' spread about the soup | the soup's triangle size
SOUP_GATES = dict(max_dist_point=0.2, max_dist_vert=0.3, min_cos_point=0.0, min_cos_vert=-0.2, reject_boundary=True)
SOUP_QUERY_FACES = 513              # the scanned faces of the query-count cases: one past the staged chunk
SOUP_QUERY_SEED = 2                 # added to 10 Q; every draw below meets FLAG_CAP (tests/test_robust_cpu.py)


def soup_problem(F, S, seed, N=1, V=None):
    """N ribbons of V vertices (F + 2 unless given) against N soups of F faces, S points near each soup with random unit normals
    (the problem of tests/test_gpu_surface_gate.py)"""
    V = V or F + 2
    fit = np.stack([mc.ribbon(V, seed=seed + 7 * n)[0] for n in range(N)])
    faces = mc.ribbon(V, seed=0)[1]
    targets = [mc.soup(F, seed=seed + 100 + n) for n in range(N)]
    pts = np.stack([mc.points_near(targets[n][0], targets[n][1], S, seed=seed + 200 + n, sigma=0.05) for n in range(N)])
    nrm = np.random.RandomState(seed + 300).randn(N, S, 3)
    nrm = (nrm / np.linalg.norm(nrm, axis=2, keepdims=True)).astype(np.float32)
    return fit, faces, targets, pts, nrm


def counts_around(F0, slices):
    """F0 and the counts either side of every slice boundary of F0 triangles cut in `slices` (tests/test_gpu_surface_term.py's rule)"""
    span = -(-F0 // slices)
    out = {F0}
    for k in range(1, slices + 1):
        out |= {k * span - 1, k * span, k * span + 1}
    return sorted(f for f in out if f >= 1)


def surface_sweep(slices_of):
    """(tag, F, Q, V, seed) of the surface term's size sweep; slices_of(queries, faces): the host's slice rule"""
    out = []
    for F0 in mc.scanned_counts(512):
        for F in counts_around(F0, slices_of(65, F0)):
            out.append(("faces %d" % F, F, 65, 65, F))
    for Q in QUERY_COUNTS:
        out.append(("queries %d" % Q, SOUP_QUERY_FACES, Q, max(Q, 3), 10 * Q + SOUP_QUERY_SEED))
    return list(dict((c[0], c) for c in out).values())


STRAY_SIGMA = 0.25                  # of stray_scene: two cells of the plates' grid (a point lies up to 0.09 from a vertex), the stray
                                    # cluster 2 and more away


def stray_scene(seed=0, n=9, S_near=100, S_stray=30):
    """a fitted n x n plate; the target is a slightly turned and lifted copy of it AND, far below and to the side, a small plate of
    its own (a floor, a stand): a stray cluster that shows neither a rim towards the fit nor a flipped normal.  Points on both
    -> dict(fit (1,V,3), faces, targets [(verts, faces)], points (1,S,3), point_normals, point_boundary, stray (S,) bool)"""
    rs = np.random.RandomState(4000 + seed)
    fv, ff = gc.plate(n, hole=())
    fit = (fv + np.float32(0.002) * rs.randn(*fv.shape)).astype(np.float32)
    tv = (fv.astype(np.float64) @ gc._rotation(rs, 0.02).T + np.array([0.013, -0.007, 0.02])).astype(np.float32)
    sv, sf = gc.plate(4, hole=(), z=0.0, size=0.5)
    sv = (sv.astype(np.float64) @ gc._rotation(rs, 0.3).T + np.array([1.7, 0.4, -1.9])).astype(np.float32)
    pa, na, ba, _ = cc.sample_on(tv, ff, S_near, rs)
    pb, nb, bb, _ = cc.sample_on(sv, sf, S_stray, rs)
    target = (np.concatenate([tv, sv]), np.concatenate([ff, sf + len(tv)]).astype(np.int32))
    stray = np.concatenate([np.zeros(S_near, bool), np.ones(S_stray, bool)])
    return dict(fit=fit[None], faces=ff, targets=[target], points=np.concatenate([pa, pb])[None],
                point_normals=np.concatenate([na, nb])[None], point_boundary=np.concatenate([ba, bb])[None], stray=stray)


SCENE_SEEDS = (0, 1, 2)
# the oracle scenes of the gated terms (posed stand-in pieces) under the kernel: the scale is a few times their gates' cap
CHAMFER_SCENE_SIGMA = 2 * cc.ORACLE_GATES["max_dist_vert"]
SURFACE_SCENE_SIGMA = 2 * gc.ORACLE_GATES["max_dist_vert"]
ALL_ON = scales(sigma_chamfer_point=0.11, sigma_chamfer_vert=0.17, sigma_surface_point=0.13, sigma_surface_vert=0.19)
EACH_SCALE = tuple(scales(**{k: ALL_ON[k]}) for k in KEYS) + (ALL_ON,)


# ---------------------------------------------------------------------------------------------------------------
# refusals: every rule of smalfit_plan.h::robust_args_refusal in its order
# ---------------------------------------------------------------------------------------------------------------
SIZE_TEXT = "smalfit_robust_args.struct_size does not match this library (built against another smalfit.h?)"
FACTS = dict(chamfer_call=True, surface_call=True, chamfer_on=True, point_dir=True, vert_dir=True)


def valid_block():
    """a block every rule accepts in a step with both terms on (pointers are dummies)"""
    r = _lib.RobustArgs()
    r.sigma_chamfer_point, r.sigma_chamfer_vert, r.sigma_surface_point, r.sigma_surface_vert = 0.1, 0.2, 0.3, 0.4
    r.chamfer_weight_sums, r.surface_weight_sums = 0x10000, 0x11000
    r.chamfer_point_weights, r.chamfer_vert_weights, r.surface_point_weights, r.surface_vert_weights = 0x12000, 0x13000, 0x14000, 0x15000
    return r


_set = gc._set
_none = _set()
SQUARE = "the float32 square of %s is not a normal number"
OFF = "%s given while %s is off"
NO_CHAMFER = "chamfer weight outputs given to a call that does not evaluate the chamfer term"
NO_SURFACE = "surface weight outputs given to a call that does not evaluate the surface term"
# (name, change to the block, facts, text) in the order of the rules
REFUSALS = (
    ("struct_size", _set(struct_size=C.sizeof(_lib.RobustArgs) - 8), {}, SIZE_TEXT),
    ("struct_size before a bad square", _set(struct_size=0, sigma_chamfer_point=1e-30), {}, SIZE_TEXT),
    ("chamfer point square underflows", _set(sigma_chamfer_point=1e-20), {}, SQUARE % "sigma_chamfer_point"),
    ("chamfer point square is subnormal", _set(sigma_chamfer_point=1.0e-19), {}, SQUARE % "sigma_chamfer_point"),
    ("chamfer point square overflows", _set(sigma_chamfer_point=1e20), {}, SQUARE % "sigma_chamfer_point"),
    ("chamfer vertex square", _set(sigma_chamfer_vert=3e19), {}, SQUARE % "sigma_chamfer_vert"),
    ("surface point square", _set(sigma_surface_point=1e-23), {}, SQUARE % "sigma_surface_point"),
    ("surface vertex square", _set(sigma_surface_vert=2e19), {}, SQUARE % "sigma_surface_vert"),
    ("the squares in their order", _set(sigma_surface_vert=2e19, sigma_chamfer_vert=1e-25), {}, SQUARE % "sigma_chamfer_vert"),
    ("a bad square of a skipped direction", _set(sigma_surface_vert=2e19, surface_vert_weights=None), dict(vert_dir=False),
     SQUARE % "sigma_surface_vert"),
    ("chamfer sums into the surface call", _set(chamfer_point_weights=None, chamfer_vert_weights=None), dict(chamfer_call=False), NO_CHAMFER),
    ("chamfer weights into the surface call", _set(chamfer_weight_sums=None, chamfer_point_weights=None), dict(chamfer_call=False), NO_CHAMFER),
    ("surface sums into the chamfer call", _set(surface_point_weights=None, surface_vert_weights=None), dict(surface_call=False), NO_SURFACE),
    ("chamfer point weights, scale 0", _set(sigma_chamfer_point=0.0), {}, OFF % ("chamfer_point_weights", "sigma_chamfer_point")),
    ("chamfer point weights, scale negative", _set(sigma_chamfer_point=-1.0), {}, OFF % ("chamfer_point_weights", "sigma_chamfer_point")),
    ("chamfer point weights, scale infinite", _set(sigma_chamfer_point=float("inf")), {}, OFF % ("chamfer_point_weights", "sigma_chamfer_point")),
    ("chamfer point weights, scale NaN", _set(sigma_chamfer_point=float("nan")), {}, OFF % ("chamfer_point_weights", "sigma_chamfer_point")),
    ("chamfer point weights, the term off", _none, dict(chamfer_on=False), OFF % ("chamfer_point_weights", "sigma_chamfer_point")),
    ("chamfer vertex weights, scale off", _set(sigma_chamfer_vert=0.0), {}, OFF % ("chamfer_vert_weights", "sigma_chamfer_vert")),
    ("surface point weights, scale off", _set(sigma_surface_point=0.0), {}, OFF % ("surface_point_weights", "sigma_surface_point")),
    ("surface point weights, direction skipped", _none, dict(point_dir=False), OFF % ("surface_point_weights", "sigma_surface_point")),
    ("surface vertex weights, scale off", _set(sigma_surface_vert=0.0), {}, OFF % ("surface_vert_weights", "sigma_surface_vert")),
    ("surface vertex weights, direction skipped", _none, dict(vert_dir=False), OFF % ("surface_vert_weights", "sigma_surface_vert")),
    ("the weights in their order", _set(sigma_chamfer_vert=0.0, sigma_surface_vert=0.0), {}, OFF % ("chamfer_vert_weights", "sigma_chamfer_vert")),
)
_NO_WEIGHTS = dict(chamfer_point_weights=None, chamfer_vert_weights=None, surface_point_weights=None, surface_vert_weights=None)
# accepted edges: (name, change to the block, facts)
ACCEPTED = (
    ("as is", _none, {}),
    ("every scale off, sums alone", _set(sigma_chamfer_point=0.0, sigma_chamfer_vert=-1.0, sigma_surface_point=float("nan"),
                                        sigma_surface_vert=float("inf"), **_NO_WEIGHTS), {}),
    ("no output at all", _set(chamfer_weight_sums=None, surface_weight_sums=None, **_NO_WEIGHTS), {}),
    ("the smallest square that is normal", _set(sigma_chamfer_point=1.0842022e-19), {}),       # 2^-63: its square is 2^-126
    ("the largest square that is finite", _set(sigma_surface_vert=1.8446743e19), {}),          # just under 2^64
    ("sums of a skipped direction read 0", _set(surface_point_weights=None), dict(point_dir=False)),
    ("the chamfer call ignores the surface scales", _set(surface_weight_sums=None, surface_point_weights=None, surface_vert_weights=None),
     dict(surface_call=False, point_dir=False, vert_dir=False)),
    ("the surface call ignores the chamfer scales", _set(chamfer_weight_sums=None, chamfer_point_weights=None, chamfer_vert_weights=None),
     dict(chamfer_call=False, chamfer_on=False)),
    ("the chamfer term off: its scales are off", _set(chamfer_point_weights=None, chamfer_vert_weights=None), dict(chamfer_on=False)),
)

# the plan's table: (scales on (cp, cv, sp, sv), facts) -> (chamfer, surface_point, surface_vert, which s2 are > 0)
PLAN_TABLE = (
    ((0, 0, 0, 0), {}, (False, False, False, (0, 0, 0, 0))),
    ((1, 0, 0, 0), {}, (True, False, False, (1, 0, 0, 0))),
    ((0, 1, 0, 0), {}, (True, False, False, (0, 1, 0, 0))),
    ((0, 0, 1, 0), {}, (False, True, False, (0, 0, 1, 0))),
    ((0, 0, 0, 1), {}, (False, False, True, (0, 0, 0, 1))),
    ((1, 1, 1, 1), {}, (True, True, True, (1, 1, 1, 1))),
    ((1, 1, 1, 1), dict(chamfer_on=False), (False, True, True, (0, 0, 1, 1))),
    ((1, 1, 1, 1), dict(chamfer_call=False), (False, True, True, (0, 0, 1, 1))),
    ((1, 1, 1, 1), dict(surface_call=False), (True, False, False, (1, 1, 0, 0))),
    ((1, 1, 1, 1), dict(point_dir=False), (True, False, True, (1, 1, 0, 1))),
    ((1, 1, 1, 1), dict(vert_dir=False), (True, True, False, (1, 1, 1, 0))),
)
