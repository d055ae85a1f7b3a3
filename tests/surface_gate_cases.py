"""The expected values and the cases of the gated point-to-surface term (smalfit_mesh_surface_eval_gated, smalfit_fit3d_step_gated,
smalfit_mesh_targets_sample_normals), shared by tests/test_surface_gate_cpu.py (the host shim) and tests/test_gpu_surface_gate.py
(HIP through the C-ABI).  Nothing here asserts or needs a GPU.  Test infrastructure, not the library: a numpy brute force written
from the definitions include/smalfit.h words, on top of tests/surface_term_cases.py (d, the candidate order, the tie rule, r):

  compatible     g |g| / |n|^2 >= c |c| with g = <u, n>, n = (b - a) x (c - a); 0 on the left for a degenerate face or a zero u;
                 c <= -1 is off
  gated nearest  the lowest face index among the least d^2 of the compatible faces; none compatible: the query finds nothing
  normals        fitted vertex: the sum of its incident faces' n over its length, zero for a zero length; target point: the unit
                 normal of its face
  truncation     dropped when d^2 > tau^2, tau^2 the float32 product
  boundary       vertex -> target only: the winner is a segment and (it is a boundary edge, or its parameter is exactly 0 / 1 and
                 the start / end corner is a boundary vertex)
  kept           found a face and no gate dropped it; a dropped query counts 0 everywhere, the denominators stay N S and N V

evaluated in float64 (the oracle) or, by the same code, in float32 (the yardstick).

FLAGGING (float64): a query is flagged when its distance is within delta (surface_term_cases.DELTA_ULP ulp(L)) of tau, when the
compatibility test within EPS of the threshold could change its answer -- the winners under c |c| - EPS and under c |c| + EPS are
not both the winner: this is the case when the winning face's signed squared cosine is within EPS of the threshold, or a face
that would overtake it is (the runner-up) -- or by the reach rule of surface_term_cases among the compatible faces.

EPS: the float32 shim's signed squared cosine against float64 on these very inputs (test_surface_gate_cpu.py measures it again
and holds it to the record): largest deviation COS_DEVIATION_MEASURED, EPS = 4 x that, the device being free to contract the
products differently than the host compiler.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from smalify_amd import _lib
from tests import mesh_score_cases as mc
from tests import surface_term_cases as stc

DELTA_ULP = stc.DELTA_ULP
FLAG_CAP = stc.FLAG_CAP
COS_DEVIATION_MEASURED = 2.96e-7    # largest |ssc32 - ssc64| of the shim over the oracle scenes below: 2.953e-7 (the CPU test prints it)
EPS = 4 * COS_DEVIATION_MEASURED


# ---------------------------------------------------------------------------------------------------------------
# normals and boundaries from their definitions
# ---------------------------------------------------------------------------------------------------------------
def face_normals(verts, faces, dtype=np.float64):
    v = np.asarray(verts, dtype)
    f = np.asarray(faces, np.int64)
    return np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]).astype(dtype)


def _unit(n, dtype):
    ln = np.sqrt((n * n).sum(-1, dtype=dtype))
    with np.errstate(all="ignore"):
        inv = np.where(ln > 0, dtype(1) / np.where(ln > 0, ln, dtype(1)), dtype(0))
    return (n * inv[..., None]).astype(dtype)


def face_unit_normals(verts, faces, dtype=np.float64):
    return _unit(face_normals(verts, faces, dtype), dtype)


def vertex_normals(verts, faces, dtype=np.float64):
    n = face_normals(verts, faces, dtype)
    f = np.asarray(faces, np.int64)
    s = np.zeros((len(np.asarray(verts)), 3), dtype)
    for face in range(len(f)):                       # ascending face index: the order of the definition
        for k in range(3):
            s[f[face, k]] += n[face]
    return _unit(s, dtype)


def boundary(V, faces):
    """-> (flags (F,) uint8 as mesh3d_topology.h words them, boundary edge set, boundary vertex set) from the definition"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    use = {}
    for face in range(len(f)):
        for k in range(3):
            e = tuple(sorted((int(f[face, k]), int(f[face, (k + 1) % 3]))))
            use[e] = use.get(e, 0) + 1
    edges = {e for e, cnt in use.items() if cnt == 1}
    rim = {v for e in edges for v in e}
    flags = np.zeros(len(f), np.uint8)
    for face in range(len(f)):
        for k in range(3):
            if tuple(sorted((int(f[face, k]), int(f[face, (k + 1) % 3])))) in edges:
                flags[face] |= 1 << k
            if int(f[face, k]) in rim:
                flags[face] |= 1 << (3 + k)
    return flags, edges, rim


def tau2_of(tau):
    """tau^2 as the host forms it (float32), +inf when truncation is off"""
    t = np.float32(tau)
    return np.float32(np.inf) if not (t > 0 and np.isfinite(t)) else np.float32(t * t)


def signed_sq_cos(u, n, dtype=np.float64):
    """(Q,3) against (F,3) -> (Q,F)"""
    u, n = np.asarray(u, dtype), np.asarray(n, dtype)
    g = u @ n.T
    nn = (n * n).sum(-1)
    with np.errstate(all="ignore"):
        inv = np.where(nn > 0, dtype(1) / np.where(nn > 0, nn, dtype(1)), dtype(0))
    return (g * np.abs(g) * inv[None]).astype(dtype)


# ---------------------------------------------------------------------------------------------------------------
# gated queries against a mesh
# ---------------------------------------------------------------------------------------------------------------
def gated_nearest(q, u, verts, faces, min_cos=-1.0, tau=0.0, flags=None, dtype=np.float64, delta=None, eps=EPS):
    """every query against every face -> dict(face (-1 dropped), kept, d2, bary, r, q) with zeros for the dropped; with delta
    (float64) also `flagged`.  u: (Q,3) unit normals, read when min_cos > -1.  flags: the scanned mesh's boundary flags or None"""
    qs = np.asarray(q, dtype).reshape(-1, 3)
    v = np.asarray(verts, dtype).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    Q = len(qs)
    o = stc.closest(qs[:, None, :], v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None], dtype)
    d2 = o["d2"]
    cos_on = min_cos > -1.0
    cc = dtype(np.float32(min_cos) * np.abs(np.float32(min_cos)))
    inf = dtype(np.inf)
    if cos_on:
        ssc = signed_sq_cos(u, face_normals(v, f, dtype), dtype)
        d2m = np.where(ssc >= cc, d2, inf)
    else:
        d2m = d2
    rows = np.arange(Q)
    win = np.argmin(d2m, 1)
    dw = d2m[rows, win]
    found = np.isfinite(dw)
    t2 = dtype(tau2_of(tau))
    keep = found & ~(dw > t2)
    winner = o["winner"][rows, win]
    bw = o["bary"][rows, win]
    if flags is not None:
        t = np.where(winner == 0, bw[:, 1], np.where(winner == 1, bw[:, 2], bw[:, 0]))
        fl = np.asarray(flags)[win].astype(np.int64)
        seg = winner < 3
        wk = np.minimum(winner, 2)
        edge = (fl >> wk) & 1
        start = (fl >> (3 + wk)) & 1
        end = (fl >> (3 + (wk + 1) % 3)) & 1
        hit = seg & ((edge == 1) | ((t == 0) & (start == 1)) | ((t == 1) & (end == 1)))
        keep &= ~hit
    out = dict(face=np.where(keep, win, -1), kept=keep, d2=np.where(keep, dw, dtype(0)).astype(dtype),
               bary=np.where(keep[:, None], bw, dtype(0)).astype(dtype), r=np.where(keep[:, None], o["r"][rows, win], dtype(0)).astype(dtype),
               q=o["q"][rows, win])
    if delta is not None:
        d = np.sqrt(np.where(found, dw, 0.0))
        flagged = np.zeros(Q, bool)
        if np.isfinite(t2):
            flagged |= found & (np.abs(d - np.sqrt(t2)) <= delta)
        if cos_on:
            for shift in (-eps, eps):
                dm = np.where(ssc >= cc + shift, d2, inf)
                w2 = np.argmin(dm, 1)
                f2 = np.isfinite(dm[rows, w2])
                flagged |= (f2 != found) | (f2 & found & (w2 != win))
        reach = 2.0 * np.sqrt(2.0 * d * delta + delta * delta)
        with np.errstate(all="ignore"):
            near = np.sqrt(d2m) <= (d + delta)[:, None]
        far = np.sqrt(((o["q"] - o["q"][rows, win][:, None, :]) ** 2).sum(-1)) > reach[:, None]
        flagged |= found & (near & far).any(1)
        out["flagged"] = flagged
    return out


def open_gates():
    return dict(max_dist_point=0.0, max_dist_vert=0.0, min_cos_point=-1.0, min_cos_vert=-1.0, reject_boundary=False)


def faces_equivalent(q, u, verts, faces, got_face, want, min_cos, delta, eps=EPS):
    """which kept queries' returned faces stand for the oracle's: the same face, or -- the closest point lying on an edge or a
    corner that several faces share, where exact arithmetic ties and the lowest index is decided by rounding -- a face whose own
    float64 distance is within delta of the least and which is compatible within eps (the criterion tests/test_gpu_surface_term.py
    holds a returned face to).  -> bool per query (True for the dropped ones)"""
    kept = np.asarray(want["kept"], bool)
    got_face = np.asarray(got_face, np.int64)
    same = got_face == want["face"]
    fc = np.where(kept & (got_face >= 0), got_face, 0)
    own = stc.face_dist(q, verts, faces, fc)
    ok = np.abs(own - np.sqrt(want["d2"])) <= delta
    if min_cos > -1.0:
        n = face_normals(verts, faces)[fc]
        g = (np.asarray(u, np.float64) * n).sum(-1)
        nn = (n * n).sum(-1)
        ssc = g * np.abs(g) / np.where(nn > 0, nn, 1.0)
        ok &= ssc >= np.float32(min_cos) * np.abs(np.float32(min_cos)) - eps
    return ~kept | same | ((got_face >= 0) & ok)


def gated_term(verts, faces, targets, points, point_normals, w_ps, w_vs, gates, dtype=np.float64, delta=None, eps=EPS):
    """verts (N,V,3), faces (F,3), targets: list of N (verts, faces) or None, points / point_normals (N,S,3) or None
    -> dict(L_ps, L_vs, term, rows (N,2), kept (N,2), dverts (N,V,3), dtrans, vert_normals, point / vert: the gated_nearest dicts)"""
    g = dict(open_gates(), **gates)
    verts = np.asarray(verts, dtype)
    N, V = verts.shape[:2]
    f = np.asarray(faces, np.int64)
    rows, kept = np.zeros((N, 2), dtype), np.zeros((N, 2), np.int64)
    grad = np.zeros((N, V, 3), dtype)
    hp, hv, vn = [], [], []
    two = dtype(2)
    if w_ps > 0:
        S = np.asarray(points).shape[1]
        for n in range(N):
            o = gated_nearest(points[n], None if point_normals is None else point_normals[n], verts[n], f, g["min_cos_point"],
                              g["max_dist_point"], None, dtype, delta, eps)
            hp.append(o)
            rows[n, 0], kept[n, 0] = o["d2"].sum(dtype=dtype), o["kept"].sum()
            coef = dtype(w_ps) * two / (dtype(S) * dtype(N))
            fc = np.where(o["kept"], o["face"], 0)
            for i in range(3):
                np.add.at(grad[n], f[fc, i], -coef * o["bary"][:, i:i + 1] * o["r"])
    if w_vs > 0:
        for n in range(N):
            tv, tf = targets[n]
            u = vertex_normals(verts[n], f, dtype) if g["min_cos_vert"] > -1 else None
            vn.append(u)
            fl = boundary(len(tv), tf)[0] if g["reject_boundary"] else None
            o = gated_nearest(verts[n], u, tv, tf, g["min_cos_vert"], g["max_dist_vert"], fl, dtype, delta, eps)
            hv.append(o)
            rows[n, 1], kept[n, 1] = o["d2"].sum(dtype=dtype), o["kept"].sum()
            grad[n] += dtype(w_vs) * two / (dtype(V) * dtype(N)) * o["r"]
    L_ps = rows[:, 0].sum(dtype=dtype) / dtype(N * np.asarray(points).shape[1]) if w_ps > 0 else dtype(0)
    L_vs = rows[:, 1].sum(dtype=dtype) / dtype(N * V) if w_vs > 0 else dtype(0)
    return dict(L_ps=L_ps, L_vs=L_vs, term=dtype(max(w_ps, 0)) * L_ps + dtype(max(w_vs, 0)) * L_vs, rows=rows, kept=kept, dverts=grad,
                dtrans=grad.sum(1, dtype=dtype), vert_normals=vn, point=hp, vert=hv)


# ---------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------
def plate(n=4, hole=((1, 1),), z=0.0, flip=False, size=1.0):
    """an n x n grid of vertices over [0, size]^2 at height z, two triangles per cell wound to face +z (flip: -z), the cells in `hole`
    (column, row) left out -> (verts float32, faces int32)"""
    xs = np.linspace(0.0, size, n)
    v = np.array([(x, y, z) for y in xs for x in xs], np.float32)
    f = []
    for j in range(n - 1):
        for i in range(n - 1):
            if (i, j) in hole:
                continue
            a, b, c, d = j * n + i, j * n + i + 1, (j + 1) * n + i + 1, (j + 1) * n + i
            f += [(a, b, c), (a, c, d)]
    f = np.array(f, np.int32)
    return v, (f[:, ::-1].copy() if flip else f)


def tetrahedron():
    v = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)], np.float32)
    return v, np.array([(0, 2, 1), (0, 1, 3), (1, 2, 3), (0, 3, 2)], np.int32)


def fan_of_three():
    """three faces around the one edge (0, 1): it is used three times, not a boundary edge"""
    v = np.array([(0, 0, 0), (1, 0, 0), (0.5, 1, 0), (0.5, -1, 0), (0.5, 0, 1)], np.float32)
    return v, np.array([(0, 1, 2), (1, 0, 3), (0, 1, 4)], np.int32)


def _rotation(rs, angle):
    ax = rs.randn(3)
    ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def standin_piece(faces_wanted=700, seed=0):
    """a connected piece of the stand-in mesh: the `faces_wanted` faces whose centroids lie nearest to a seed vertex, re-indexed
    -> (verts float32, faces int32): an open, consistently wound surface with a rim"""
    v, f = stc.standin_mesh()
    rs = np.random.RandomState(seed)
    c = v[f].mean(1)
    centre = v[rs.randint(len(v))]
    pick = np.sort(np.argsort(((c - centre) ** 2).sum(1))[:faces_wanted])
    used = np.unique(f[pick])
    remap = -np.ones(len(v), np.int64)
    remap[used] = np.arange(len(used))
    return v[used].copy(), remap[f[pick]].astype(np.int32)


def drop_unused(verts, faces):
    used = np.unique(faces)
    remap = -np.ones(len(verts), np.int64)
    remap[used] = np.arange(len(used))
    return np.asarray(verts)[used].copy(), remap[faces].astype(np.int32)


def remove_patch(verts, faces, share, seed):
    """the mesh without the `share` of its faces nearest to a random centroid (a contiguous patch); vertices kept"""
    rs = np.random.RandomState(seed)
    c = np.asarray(verts)[faces].mean(1)
    centre = c[rs.randint(len(c))]
    order = np.argsort(((c - centre) ** 2).sum(1))
    keep = np.sort(order[int(share * len(faces)):])
    return np.asarray(verts, np.float32), np.asarray(faces, np.int32)[keep]


def oracle_scene(seed, faces_wanted=700, share=0.25, S=130):
    """a posed stand-in piece, one patch of its faces removed, fitted to another pose of the piece with another patch removed (either
    surface has ground the other lacks); points sampled on the target with their faces' normals
    -> dict(fit (1,V,3), faces, targets [(v, f)], points (1,S,3), point_normals (1,S,3))"""
    rs = np.random.RandomState(1000 + seed)
    v, f0 = standin_piece(faces_wanted, seed)
    L = float(np.abs(v).max())
    tv = (v.astype(np.float64) @ _rotation(rs, 0.03).T + 0.01 * L * rs.randn(3)).astype(np.float32)
    tv, tf = remove_patch(tv, f0, share, seed)
    v, f = drop_unused(*remove_patch(v, f0, 0.15, seed + 50))
    fit = (v.astype(np.float64) @ _rotation(rs, 0.03).T + 0.004 * L * rs.randn(*v.shape)).astype(np.float32)
    fi = rs.randint(0, len(tf), S)
    w = rs.dirichlet((1.0, 1.0, 1.0), S)
    pts = (w[:, :, None] * tv.astype(np.float64)[tf[fi]]).sum(1).astype(np.float32)
    pn = face_unit_normals(tv, tf)[fi].astype(np.float32)
    return dict(fit=fit[None], faces=f, targets=[(tv, tf)], points=pts[None], point_normals=pn[None])


ORACLE_SEEDS = (0, 1, 2)
ORACLE_GATES = dict(max_dist_point=0.015, max_dist_vert=0.015, min_cos_point=0.3, min_cos_vert=0.3, reject_boundary=True)
EACH_GATE = (dict(max_dist_point=0.015), dict(max_dist_vert=0.015), dict(min_cos_point=0.3), dict(min_cos_vert=0.3),
             dict(reject_boundary=True), ORACLE_GATES)

# ---------------------------------------------------------------------------------------------------------------
# refusals: every rule of smalfit_plan.h::surface_gate_args_refusal in its order
# ---------------------------------------------------------------------------------------------------------------
SIZE_TEXT = "smalfit_surface_gate_args.struct_size does not match this library (built against another smalfit.h?)"


def valid_gate():
    """a gate block every rule accepts beside surface_term_cases.valid_args() (pointers are dummies)"""
    g = _lib.SurfaceGateArgs()
    g.max_dist_point, g.max_dist_vert, g.min_cos_point, g.min_cos_vert, g.reject_boundary = 0.1, 0.1, 0.5, 0.5, 1
    g.point_normals, g.kept, g.point_kept, g.vert_kept, g.vert_normals = 0x10000, 0x11000, 0x12000, 0x13000, 0x14000
    return g


def _set(**kw):
    def change(x):
        for k, v in kw.items():
            setattr(x, k, v)
    return change


_none = _set()
# (name, change to the gate, change to the term's block, facts, text) in the order of the rules
REFUSALS = (
    ("struct_size", _set(struct_size=C.sizeof(_lib.SurfaceGateArgs) - 8), _none, {}, SIZE_TEXT),
    ("min_cos_point above 1", _set(min_cos_point=1.5), _none, {}, "min_cos_point must be <= 1 and not NaN"),
    ("min_cos_point NaN", _set(min_cos_point=float("nan")), _none, {}, "min_cos_point must be <= 1 and not NaN"),
    ("min_cos_vert above 1", _set(min_cos_vert=1.0000001), _none, {}, "min_cos_vert must be <= 1 and not NaN"),
    ("min_cos_vert NaN", _set(min_cos_vert=float("nan")), _none, {}, "min_cos_vert must be <= 1 and not NaN"),
    ("kept missing", _set(kept=None), _none, {}, "kept missing"),
    ("boundary without targets", _set(max_dist_vert=0.0, min_cos_vert=-1.0, vert_kept=None, vert_normals=None),
     _set(w_vert_surface=0.0), dict(targets=False), "a vertex gate needs the target meshes"),
    ("vertex truncation without targets", _set(reject_boundary=0, min_cos_vert=-1.0, vert_kept=None, vert_normals=None),
     _set(w_vert_surface=0.0), dict(targets=False), "a vertex gate needs the target meshes"),
    ("vertex cosine without targets", _set(reject_boundary=0, max_dist_vert=0.0, vert_kept=None, vert_normals=None),
     _set(w_vert_surface=0.0), dict(targets=False), "a vertex gate needs the target meshes"),
    ("normals into a sampling step", _none, _none, dict(step=True), "point_normals must be NULL in a step that samples its points: it draws its own"),
    ("no normals for the caller's points", _set(point_normals=None), _none, {}, "min_cos_point needs point_normals with the caller's points"),
    ("no normals for a step's own points", _set(point_normals=None), _none, dict(step=True, step_has_points=True),
     "min_cos_point needs point_normals with the caller's points"),
    ("point_kept of a skipped direction", _none, _set(w_point_surface=0.0), {}, "point_kept given while the point direction is skipped"),
    ("vert_kept of a skipped direction", _none, _set(w_vert_surface=0.0), {}, "vert_kept given while the vertex direction is skipped"),
    ("vert_normals of a skipped direction", _set(vert_kept=None), _set(w_vert_surface=0.0), {}, "vert_normals given without min_cos_vert"),
    ("vert_normals without the test", _set(min_cos_vert=-1.0), _none, {}, "vert_normals given without min_cos_vert"),
)
# accepted edges: (name, change to the gate, change to the term's block, facts)
ACCEPTED = (
    ("as is", _none, _none, {}),
    ("every gate off", _set(max_dist_point=0.0, max_dist_vert=-1.0, min_cos_point=-1.0, min_cos_vert=-2.0, reject_boundary=0,
                            point_normals=None, vert_normals=None), _none, {}),
    ("thresholds of exactly 1", _set(min_cos_point=1.0, min_cos_vert=1.0), _none, {}),
    ("infinite distances", _set(max_dist_point=float("inf"), max_dist_vert=float("nan")), _none, {}),
    ("no optional output", _set(point_kept=None, vert_kept=None, vert_normals=None), _none, {}),
    ("a sampling step draws its own normals", _set(point_normals=None), _none, dict(step=True)),
    ("a step with the caller's points and normals", _none, _none, dict(step=True, step_has_points=True)),
    ("points only, no targets", _set(max_dist_vert=0.0, min_cos_vert=-1.0, reject_boundary=0, vert_kept=None, vert_normals=None),
     _set(w_vert_surface=0.0), dict(targets=False)),
    ("point test off needs no normals", _set(min_cos_point=-1.0, point_normals=None), _none, {}),
    ("point direction skipped needs no normals", _set(point_normals=None, point_kept=None), _set(w_point_surface=0.0), {}),
)
