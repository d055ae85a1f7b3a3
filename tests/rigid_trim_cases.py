"""The trimmed rigid pre-alignment (smalfit_trimmed_rigid_align) restated in float64 numpy from the words of include/smalfit.h, on
top of tests/rigid_align_cases.py (imported, not edited), and the cases its tests share: a side scan of the lopsided blob with a
floor under it.  Infrastructure: no GPU, no library."""
from __future__ import annotations

import numpy as np

from tests import rigid_align_cases as rc

TRIM_STARTS = 24
TRIM_ITERATIONS = 30
KEEP_POINT, KEEP_VERT = 87, 77          # of 136 points and 161 vertices
UNTRIMMED_FLOOR = 1.0                   # rad: what the untrimmed call must miss R* by for the case to show anything


# ---- the definition -------------------------------------------------------------------------------------------------------------
def select(d2, keep):
    """-> bool mask of the `keep` lowest keys (d2, index): the lowest d^2, the lowest index among equal ones"""
    d2 = np.asarray(d2)
    order = np.lexsort((np.arange(len(d2)), d2))
    kept = np.zeros(len(d2), bool)
    kept[order[:keep]] = True
    return kept


def nearest_tree(q, o):
    """rc.nearest through a k-d tree, for sets too large for the (Q,O,3) table: the same nearest row wherever the nearest is unique
    (in float64, on the sets used here, it is), d^2 formed from the differences as rc.nearest forms it"""
    from scipy.spatial import cKDTree
    idx = cKDTree(o).query(q)[1]
    return idx, ((q - o[idx]) ** 2).sum(-1)


def pairs(x, p, R, t, w_point, w_vert, keep_point, keep_vert, nearest=None):
    """-> (xs, ps, w, cost, kept_v, kept_p, thr_v, thr_p): the kept weighted pairs of one iteration under [R | t], their cost, the
    masks and the threshold d^2 of each direction (None for a skipped one).  The weights stay w / count"""
    nearest = rc.nearest if nearest is None else nearest
    z = x @ R.T + t
    xs, ps, ws, cost = [], [], [], 0.0
    kept_v = kept_p = thr_v = thr_p = None
    if w_vert > 0:
        idx, d2 = nearest(z, p)
        kept_v = select(d2, keep_vert)
        thr_v = d2[kept_v].max()
        xs.append(x[kept_v]); ps.append(p[idx[kept_v]]); ws.append(np.full(int(kept_v.sum()), w_vert / len(x)))
        cost += w_vert / len(x) * d2[kept_v].sum()
    if w_point > 0:
        idx, d2 = nearest(p, z)
        kept_p = select(d2, keep_point)
        thr_p = d2[kept_p].max()
        xs.append(x[idx[kept_p]]); ps.append(p[kept_p]); ws.append(np.full(int(kept_p.sum()), w_point / len(p)))
        cost += w_point / len(p) * d2[kept_p].sum()
    return np.concatenate(xs), np.concatenate(ps), np.concatenate(ws), cost, kept_v, kept_p, thr_v, thr_p


def iterate(x, p, R, t, w_point, w_vert, keep_point, keep_vert, nearest=None):
    """one trimmed iteration -> (R, t, cost before the solve, kept rotation)"""
    xs, ps, w, cost = pairs(x, p, R, t, w_point, w_vert, keep_point, keep_vert, nearest)[:4]
    Rn, tn, determined = rc.kabsch(xs, ps, w, x.mean(0), p.mean(0))
    if not determined:
        W = w.sum()
        mx, mp = (w[:, None] * xs).sum(0) / W, (w[:, None] * ps).sum(0) / W
        return R, mp - R @ mx, cost, 1
    return Rn, tn, cost, 0


def align(x, p, keep_point, keep_vert, starts=None, iterations=TRIM_ITERATIONS, w_point=1.0, w_vert=1.0, nearest=None):
    """the whole trimmed call for one mesh in float64; keep == the count in both directions is rigid_align_cases.align"""
    x, p = np.asarray(x, np.float64), np.asarray(p, np.float64)
    starts = rc.cube_rotations() if starts is None else np.asarray(starts, np.float64)
    K = len(starts)
    Rs, ts, scores, kept = np.empty((K, 3, 3)), np.empty((K, 3)), np.empty(K), np.zeros(K, int)
    thr = np.zeros((K, 2))
    for k in range(K):
        R, t = rc.start_transform(starts[k], x, p)
        for it in range(iterations):
            Rn, tn, _, kp = iterate(x, p, R, t, w_point, w_vert, keep_point, keep_vert, nearest)
            if kp == 0 and np.array_equal(Rn, R) and np.array_equal(tn, t):
                break                                   # a fixed point: every later iteration repeats this one bit for bit
            R, t = Rn, tn
            kept[k] += kp
        out = pairs(x, p, R, t, w_point, w_vert, keep_point, keep_vert, nearest)
        scores[k] = out[3]
        thr[k] = [0.0 if out[6] is None else out[6], 0.0 if out[7] is None else out[7]]
        Rs[k], ts[k] = R, t
    return dict(R=Rs, t=ts, scores=scores, best=int(np.argmin(scores)), kept=kept, trim_d2=thr)


# ---- the cases ------------------------------------------------------------------------------------------------------------------
POSES = ("identity", "back_to_front", "cube5_skew15", "cube13_skew25")


def floor_points():
    rs = np.random.RandomState(11)
    fx = rs.uniform(-1, 1, 40)
    fz = rs.uniform(-0.6, 0.6, 40)
    return np.ascontiguousarray(np.stack([fx, np.full(40, -1.2), fz], 1), np.float32)


def _partial_cases():
    x = rc.lopsided_blob()
    seen = x[:, 1] > -0.1
    assert int(seen.sum()) == 96
    out = {}
    for name in POSES:
        c = rc.RECOVERY_CASES[name]
        p = np.ascontiguousarray(np.concatenate([rc.moved(x, c["R"], c["t"])[seen], floor_points()]), np.float32)
        out[name] = dict(name=name, x=x, p=p, R=c["R"], t=c["t"], extent=c["extent"], seen=seen, keep_point=KEEP_POINT, keep_vert=KEEP_VERT)
    return out


PARTIAL_CASES = _partial_cases()
_REFERENCE = {}


def reference(name, variant="trimmed"):
    """the float64 restatement on a partial case, computed once: variant trimmed | untrimmed (both ways) | untrimmed_points
    (w_vert = 0)"""
    key = (name, variant)
    if key not in _REFERENCE:
        c = PARTIAL_CASES[name]
        if variant == "trimmed":
            _REFERENCE[key] = align(c["x"], c["p"], c["keep_point"], c["keep_vert"])
        else:
            _REFERENCE[key] = rc.align(c["x"], c["p"], None, TRIM_ITERATIONS, 1.0, 1.0 if variant == "untrimmed" else 0.0)
    return _REFERENCE[key]


# ---- a partial, cluttered target of the stand-in model ----------------------------------------------------------------------------
MODEL_TURN = rc.cube_rotations()[9] @ rc.axis_angle([1, 2, -1], 12.0)
MODEL_SHIFT = np.array([0.3, -0.2, 0.1])
MODEL_TRIM_POINT, MODEL_TRIM_VERT = 0.8, 0.56
# the cut.  Tried and NOT admitted on the stand-in model (the float64 restatement ends a half turn or 0.2 rad off): the rest-pose
# template under any cut (it is mirror-symmetric and nearly so front to back), and on the posed mesh the cuts along coordinate 1
# at the 25 % and 35 % quantiles.  Admitted: the posed, reshaped mesh cut along coordinate 2 at the 30 % quantile
MODEL_CUT_AXIS, MODEL_CUT_QUANTILE = 2, 0.3
MODEL_POINTS = 600
# rad: the points are drawn ON the target's faces, not at its vertices, so no rigid motion brings the kept pairs to distance 0 and
# the restatement itself ends a sampling error away from R* (measured 0.024 rad with 600 points); a wrong end state is a quarter
# turn or more away.  The device is held to the restatement's own answer under the recovery caps, not to this bound
MODEL_ADMISSION = 0.1


def model_parameters(N=1, seed=0):
    """pose and shape that take the stand-in mesh off its symmetric rest pose -> (global_rot (N,3), joint_rot (N,34,3), betas (N,20))"""
    rs = np.random.RandomState(seed)
    theta = np.concatenate([0.3 * rs.randn(N, 1, 3), 0.25 * rs.randn(N, 34, 3)], 1)
    return theta[:, 0].copy(), theta[:, 1:].copy(), 0.6 * rs.randn(N, 20)


def partial_target(verts, faces, R=MODEL_TURN, t=MODEL_SHIFT, axis=MODEL_CUT_AXIS, quantile=MODEL_CUT_QUANTILE):
    """the mesh (V,3) / (F,3) turned by R and moved by t, the faces of one side removed (a face stays when all three of its
    vertices lie on the seen side of the cut below), plus a floor quad under it -> (verts float32, faces int64, seen vertex mask).
    The cut: the vertices whose coordinate `axis` is above its `quantile`: the centroid moves across the body, not along it"""
    v = np.asarray(verts, np.float64)
    faces = np.asarray(faces, np.int64)
    seen = v[:, axis] > np.quantile(v[:, axis], quantile)
    keep_faces = faces[seen[faces].all(1)]
    moved = v @ np.asarray(R).T + np.asarray(t)
    extent = float((v.max(0) - v.min(0)).max())
    lo, hi = moved.min(0), moved.max(0)
    # the floor: a quad below everything, 0.3 extents under the lowest vertex of the moved mesh along its second coordinate
    y = lo[1] - 0.3 * extent
    cx, cz, h = 0.5 * (lo[0] + hi[0]), 0.5 * (lo[2] + hi[2]), 0.15 * extent
    quad = np.array([[cx - h, y, cz - h], [cx + h, y, cz - h], [cx + h, y, cz + h], [cx - h, y, cz + h]])
    V = len(v)
    out_v = np.concatenate([moved, quad]).astype(np.float32)
    out_f = np.concatenate([keep_faces, [[V, V + 1, V + 2], [V, V + 2, V + 3]]]).astype(np.int64)
    return out_v, out_f, seen


def draw_points(verts, faces, S, seed):
    """S points drawn uniformly by area on the faces, in float64, rounded once to float32 (numpy's own draw: the CPU stand-in for
    the device's sampler)"""
    rs = np.random.RandomState(seed)
    tv, tf = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    a, b, c = tv[tf[:, 0]], tv[tf[:, 1]], tv[tf[:, 2]]
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    fi = rs.choice(len(tf), S, p=area / area.sum())
    u, w = rs.rand(S), rs.rand(S)
    su = np.sqrt(u)
    return ((1 - su)[:, None] * a[fi] + (su * (1 - w))[:, None] * b[fi] + (su * w)[:, None] * c[fi]).astype(np.float32)
