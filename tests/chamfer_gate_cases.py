"""The expected values and the cases of the gated chamfer term (smalfit_mesh_objective_eval_gated, smalfit_fit3d_step_partial,
smalfit_mesh_targets_sample_attrs), shared by tests/test_chamfer_gate_cpu.py (the host shim) and tests/test_gpu_chamfer_gate.py
(HIP through the C-ABI).  Nothing here asserts or needs a GPU.  Test infrastructure, not the library: a numpy brute force written
from the definitions include/smalfit.h words, with no reference code:

  d^2            |q - x|^2, nearest = the lowest index among the least d^2
  compatible     <a, b> >= c for the two unit normals; a zero normal gives 0 on the left; c <= -1 is off
  point -> vertex   nn(s) = the nearest vertex compatible with m_s; kept when it exists and d^2 <= tau^2 (tau^2 the float32 product;
                 tau <= 0 or not finite: off); a dropped point has nn = -1
  vertex -> point   nn'(v) = the nearest point compatible with u_v; kept when it exists, d^2 <= tau^2 and not (reject_boundary and
                 the WINNER's boundary byte != 0)
  loss           1/(N S) sum over kept s of d^2 + 1/(N V) sum over kept v of d^2 (the denominators stay N S and N V)
  gradient       w [2/(N V) [v kept] (y_v - x_nn'(v)) + 2/(N S) sum over kept s with nn(s) = v of (y_v - x_s)]

evaluated in float64 (the oracle) or, by the same code, in float32 (the yardstick).

FLAGGING (float64): a query is flagged, and left out of exact comparisons, when its distance is within delta (DELTA_ULP ulp(L),
the bar of tests/mesh_score_cases.py) of tau; when the winner changes between the thresholds c - EPS and c + EPS; or when the
runner-up's d^2 is within the float32 rounding of d^2 of the winner's (TIE_ROUNDINGS x 2^-24 x d^2: the three differences, the
three products and the two additions of either candidate).

EPS: four times the float32 shim's largest deviation of the dot product of two unit normals from float64 on the scenes below
(tests/test_chamfer_gate_cpu.py measures it again and holds it to the record), the device being free to contract differently."""
from __future__ import annotations

import ctypes as C

import numpy as np

from smalify_amd import _lib
from tests import surface_gate_cases as gc

DELTA_ULP = gc.DELTA_ULP
FLAG_CAP = 0.03
DOT_DEVIATION_MEASURED = 1.2e-7     # largest |dot32 - dot64| of the shim over the scenes below (the CPU test prints it)
EPS = 4 * DOT_DEVIATION_MEASURED
TIE_ROUNDINGS = 8.0
CHUNK = 512                         # kChamGateChunk of smalfit_plan.h (the CPU test reads it back from the shim)


def open_gates():
    return dict(max_dist_point=0.0, max_dist_vert=0.0, min_cos_point=-1.0, min_cos_vert=-1.0, reject_boundary=False)


def tau2_of(tau):
    return gc.tau2_of(tau)


def ulp_l(*arrays):
    """2^-23 x the largest coordinate magnitude (tests/mesh_score_cases.py's ulp(L))"""
    return 2.0 ** -23 * max(float(np.abs(np.asarray(a, np.float64)).max()) for a in arrays)


def pair_d2(q, x, dtype=np.float64):
    """(Q,3) against (X,3) -> (Q,X)"""
    q, x = np.asarray(q, dtype), np.asarray(x, dtype)
    d = q[:, None, :] - x[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]).astype(dtype)


def gated_direction(q, qn, x, xn, xb, min_cos=-1.0, tau=0.0, reject=False, dtype=np.float64, delta=None, eps=EPS,
                    tie=TIE_ROUNDINGS * 2.0 ** -24):
    """every query against every scanned element -> dict(index (-1: none found), kept, d2 (0 for the dropped), found); with delta
    (float64) also `flagged`.  qn / xn: (Q,3) / (X,3) unit normals, read when min_cos > -1; xb: (X,) boundary bytes, read with reject"""
    d2 = pair_d2(q, x, dtype)
    Q = len(d2)
    inf = dtype(np.inf)
    cos_on = min_cos > -1.0
    c = dtype(np.float32(min_cos))
    if cos_on:
        dots = (np.asarray(qn, dtype) @ np.asarray(xn, dtype).T).astype(dtype)
        with np.errstate(invalid="ignore"):
            d2m = np.where(dots >= c, d2, inf)
    else:
        d2m = d2
    d2m = np.where(np.isnan(d2m), inf, d2m)
    rows = np.arange(Q)
    win = np.argmin(d2m, 1)                      # (the first of equal minima: the lowest index)
    dw = d2m[rows, win]
    found = np.isfinite(dw)
    t2 = dtype(tau2_of(tau))
    keep = found & ~(dw > t2)
    if reject:
        keep &= ~(np.asarray(xb)[win] != 0)
    out = dict(index=np.where(found, win, -1), kept=keep, d2=np.where(keep, dw, dtype(0)).astype(dtype), found=found)
    if delta is not None:
        d = np.sqrt(np.where(found, dw, 0.0))
        flagged = np.zeros(Q, bool)
        if np.isfinite(t2):
            flagged |= found & (np.abs(d - np.sqrt(t2)) <= delta)
        if cos_on:
            for shift in (-eps, eps):
                with np.errstate(invalid="ignore"):
                    dm = np.where(dots >= c + shift, d2, inf)
                w2 = np.argmin(dm, 1)
                f2 = np.isfinite(dm[rows, w2])
                flagged |= (f2 != found) | (f2 & found & (w2 != win))
        if d2m.shape[1] > 1:
            rest = d2m.copy()
            rest[rows, win] = inf
            second = rest.min(1)
            with np.errstate(invalid="ignore"):
                flagged |= found & np.isfinite(second) & (second - dw <= tie * second)
        out["flagged"] = flagged
    return out


def chamfer_gated(verts, faces, points, point_normals, point_boundary, w_chamfer, gates, dtype=np.float64, delta=None, eps=EPS,
                  tie=TIE_ROUNDINGS * 2.0 ** -24):
    """verts (N,V,3) the composed vertices, faces (F,3), points (N,S,3), point_normals (N,S,3) or None, point_boundary (N,S) or None
    -> dict(chamfer, dverts (N,V,3), dtrans (N,3), kept (N,2), vert_normals, point / vert: the gated_direction dicts per mesh)"""
    g = dict(open_gates(), **gates)
    verts = np.asarray(verts, dtype)
    points = np.asarray(points, dtype)
    N, V = verts.shape[:2]
    S = points.shape[1]
    need_normals = g["min_cos_point"] > -1 or g["min_cos_vert"] > -1
    kept = np.zeros((N, 2), np.int64)
    grad = np.zeros((N, V, 3), dtype)
    sums = np.zeros((N, 2), dtype)
    hp, hv, vn = [], [], []
    w = dtype(max(w_chamfer, 0.0))
    for n in range(N):
        u = gc.vertex_normals(verts[n], faces, dtype) if need_normals else None
        m = None if point_normals is None else np.asarray(point_normals[n], dtype)
        b = None if point_boundary is None else np.asarray(point_boundary[n])
        vn.append(u)
        p = gated_direction(points[n], m, verts[n], u, None, g["min_cos_point"], g["max_dist_point"], False, dtype, delta, eps, tie)
        v = gated_direction(verts[n], u, points[n], m, b, g["min_cos_vert"], g["max_dist_vert"], bool(g["reject_boundary"]), dtype,
                            delta, eps, tie)
        hp.append(p)
        hv.append(v)
        kept[n] = p["kept"].sum(), v["kept"].sum()
        sums[n] = p["d2"].sum(dtype=dtype), v["d2"].sum(dtype=dtype)
        cy, cx = w * dtype(2) / (dtype(V) * dtype(N)), w * dtype(2) / (dtype(S) * dtype(N))
        vk = v["kept"]
        grad[n][vk] += cy * (verts[n][vk] - points[n][v["index"][vk]])
        pk = p["kept"]
        np.add.at(grad[n], p["index"][pk], cx * (verts[n][p["index"][pk]] - points[n][pk]))
    chamfer = sums[:, 0].sum(dtype=dtype) / dtype(N * S) + sums[:, 1].sum(dtype=dtype) / dtype(N * V)
    return dict(chamfer=chamfer, dverts=grad, dtrans=grad.sum(1, dtype=dtype), kept=kept, vert_normals=vn, point=hp, vert=hv, sums=sums)


# ---------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------
def sample_on(tv, tf, S, rs):
    """S points on random faces of (tv, tf) -> (points float32, their faces' unit normals float32, boundary bytes uint8, faces)"""
    fi = rs.randint(0, len(tf), S)
    w = rs.dirichlet((1.0, 1.0, 1.0), S)
    pts = (w[:, :, None] * np.asarray(tv, np.float64)[tf[fi]]).sum(1).astype(np.float32)
    pn = gc.face_unit_normals(tv, tf)[fi].astype(np.float32)
    pb = (gc.boundary(len(tv), tf)[0][fi] != 0).astype(np.uint8)
    return pts, pn, pb, fi


def oracle_scene(seed, faces_wanted=500, share=0.3, S=130, gap=0.03):
    """a posed piece of the stand-in mesh, a patch of its faces removed, as the fitted surface; the target is another pose of the
    piece with another patch removed AND, gap x L behind it, a copy of that wound the other way (a thin sheet: its points face away
    from the fitted surface); S points on the two with their normals and boundary bytes
    -> dict(fit (1,V,3), faces, target (verts, faces), points (1,S,3), point_normals (1,S,3), point_boundary (1,S))"""
    rs = np.random.RandomState(2000 + seed)
    v, f0 = gc.standin_piece(faces_wanted, seed)
    L = float(np.abs(v).max())
    tv = (v.astype(np.float64) @ gc._rotation(rs, 0.03).T + 0.01 * L * rs.randn(3)).astype(np.float32)
    tv, tf = gc.drop_unused(*gc.remove_patch(tv, f0, share, seed))
    mean_n = gc.face_normals(tv, tf).sum(0)
    mean_n /= np.linalg.norm(mean_n)
    back = (tv.astype(np.float64) - gap * L * mean_n).astype(np.float32)
    tv, tf = np.concatenate([tv, back]), np.concatenate([tf, tf[:, ::-1] + len(tv)]).astype(np.int32)
    v, f = gc.drop_unused(*gc.remove_patch(v, f0, 0.15, seed + 50))
    fit = (v.astype(np.float64) @ gc._rotation(rs, 0.03).T + 0.004 * L * rs.randn(*v.shape)).astype(np.float32)
    pts, pn, pb, _ = sample_on(tv, tf, S, rs)
    return dict(fit=fit[None], faces=f, target=(tv, tf), points=pts[None], point_normals=pn[None], point_boundary=pb[None])


ORACLE_SEEDS = (0, 1, 2)
ORACLE_GATES = dict(max_dist_point=0.04, max_dist_vert=0.04, min_cos_point=0.3, min_cos_vert=0.3, reject_boundary=True)
EACH_GATE = (dict(max_dist_point=0.04), dict(max_dist_vert=0.04), dict(min_cos_point=0.3), dict(min_cos_vert=0.3),
             dict(reject_boundary=True), ORACLE_GATES)


def plate_points(n=5, hole=((1, 1), (2, 1), (1, 2), (2, 2)), per_cell=3, seed=0):
    """points on every face of a plate with a hole, with the faces' normals and boundary bytes"""
    tv, tf = gc.plate(n, hole=hole)
    rs = np.random.RandomState(seed)
    fi = np.repeat(np.arange(len(tf)), per_cell)
    w = rs.dirichlet((2.0, 2.0, 2.0), len(fi))
    pts = (w[:, :, None] * tv.astype(np.float64)[tf[fi]]).sum(1).astype(np.float32)
    pn = gc.face_unit_normals(tv, tf)[fi].astype(np.float32)
    pb = (gc.boundary(len(tv), tf)[0][fi] != 0).astype(np.uint8)
    return (tv, tf), pts, pn, pb


# ---------------------------------------------------------------------------------------------------------------
# refusals: every rule of smalfit_plan.h::chamfer_gate_args_refusal in its order
# ---------------------------------------------------------------------------------------------------------------
SIZE_TEXT = "smalfit_chamfer_gate_args.struct_size does not match this library (built against another smalfit.h?)"
SAMPLED_TEXT = "point_normals and point_boundary must be NULL in a step that samples its points: it draws its own"


def valid_gate():
    """a gate block every rule accepts for the caller's points (pointers are dummies)"""
    g = _lib.ChamferGateArgs()
    g.max_dist_point, g.max_dist_vert, g.min_cos_point, g.min_cos_vert, g.reject_boundary = 0.1, 0.1, 0.5, 0.5, 1
    g.point_normals, g.point_boundary, g.kept = 0x10000, 0x15000, 0x11000
    g.point_kept, g.vert_kept, g.point_nn, g.vert_nn = 0x12000, 0x13000, 0x14000, 0x16000
    return g


_set = gc._set
_none = _set()
# (name, change to the gate, facts, text) in the order of the rules
REFUSALS = (
    ("struct_size", _set(struct_size=C.sizeof(_lib.ChamferGateArgs) - 8), {}, SIZE_TEXT),
    ("min_cos_point above 1", _set(min_cos_point=1.5), {}, "min_cos_point must be <= 1 and not NaN"),
    ("min_cos_point NaN", _set(min_cos_point=float("nan")), {}, "min_cos_point must be <= 1 and not NaN"),
    ("min_cos_vert above 1", _set(min_cos_vert=1.0000001), {}, "min_cos_vert must be <= 1 and not NaN"),
    ("min_cos_vert NaN", _set(min_cos_vert=float("nan")), {}, "min_cos_vert must be <= 1 and not NaN"),
    ("kept missing", _set(kept=None), {}, "kept missing"),
    ("kept missing with the term off", _set(kept=None), dict(chamfer_on=False), "kept missing"),
    ("normals into a sampling step", _set(point_boundary=None), dict(step=True), SAMPLED_TEXT),
    ("boundary bytes into a sampling step", _set(point_normals=None), dict(step=True), SAMPLED_TEXT),
    ("normals into a sampling step with the term off", _none, dict(step=True, chamfer_on=False), SAMPLED_TEXT),
    ("no normals for the caller's points", _set(point_normals=None), {}, "a min_cos gate needs point_normals with the caller's points"),
    ("no normals, the vertex test alone", _set(point_normals=None, min_cos_point=-1.0), {},
     "a min_cos gate needs point_normals with the caller's points"),
    ("no normals for a step's own points", _set(point_normals=None), dict(step=True, step_has_points=True),
     "a min_cos gate needs point_normals with the caller's points"),
    ("no boundary bytes for the caller's points", _set(point_boundary=None), {}, "reject_boundary needs point_boundary with the caller's points"),
)
# accepted edges: (name, change to the gate, facts)
ACCEPTED = (
    ("as is", _none, {}),
    ("every gate off", _set(max_dist_point=0.0, max_dist_vert=-1.0, min_cos_point=-1.0, min_cos_vert=-2.0, reject_boundary=0,
                            point_normals=None, point_boundary=None), {}),
    ("thresholds of exactly 1", _set(min_cos_point=1.0, min_cos_vert=1.0), {}),
    ("infinite distances", _set(max_dist_point=float("inf"), max_dist_vert=float("nan")), {}),
    ("no optional output", _set(point_kept=None, vert_kept=None, point_nn=None, vert_nn=None), {}),
    ("a sampling step draws its own", _set(point_normals=None, point_boundary=None), dict(step=True)),
    ("a step with the caller's points and their attributes", _none, dict(step=True, step_has_points=True)),
    ("tests off need no normals", _set(min_cos_point=-1.0, min_cos_vert=-1.0, point_normals=None), {}),
    ("no boundary rule needs no bytes", _set(reject_boundary=0, point_boundary=None), {}),
    ("attributes given and not needed", _set(min_cos_point=-1.0, min_cos_vert=-1.0, reject_boundary=0), {}),
    ("the term off: ignored, whatever is missing", _set(point_normals=None, point_boundary=None), dict(chamfer_on=False)),
)
