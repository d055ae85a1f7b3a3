"""The rigid pre-alignment (smalfit_rigid_align) restated in float64 numpy from the words of include/smalfit.h, and the table of
cases its tests share.  Infrastructure: no GPU, no library.  The solve here is SVD Kabsch, not the kernels' Horn / Jacobi form."""
from __future__ import annotations

import itertools

import numpy as np

RANK_EPS = 1e-5           # the header's rank test: l1 - l2 > 1e-5 sqrt(sum w |x|^2) sqrt(sum w |p|^2)
RECOVERY_ITERATIONS = 30
RECOVERY_ADMISSION = 1e-6   # rad: a recovery case counts only if this restatement alone recovers R* this well


# ---- the definition -----------------------------------------------------------------------------------------------------------
def cube_rotations():
    """the 24 signed permutation matrices of determinant +1 in the header's order"""
    out = []
    for perm in itertools.permutations(range(3)):              # lexicographic
        for signs in itertools.product((1.0, -1.0), repeat=3):  # +++, ++-, +-+, ...
            R = np.zeros((3, 3))
            for i in range(3):
                R[i, perm[i]] = signs[i]
            if np.linalg.det(R) > 0:
                out.append(R)
    return np.stack(out)


def start_transform(R, x, p):
    cX, cP = x.mean(0), p.mean(0)
    return np.asarray(R, np.float64), cP - np.asarray(R, np.float64) @ cX


def nearest(q, o):
    """for every row of q the index of the nearest row of o (lowest index among equal d^2) and that d^2"""
    d2 = ((q[:, None, :] - o[None, :, :]) ** 2).sum(-1)
    idx = d2.argmin(1)
    return idx, d2[np.arange(len(q)), idx]


def pairs(x, p, R, t, w_point, w_vert):
    """-> (xs, ps, w, cost): the weighted pair set of one iteration under [R | t] and its cost"""
    z = x @ R.T + t
    xs, ps, ws, cost = [], [], [], 0.0
    if w_vert > 0:
        idx, d2 = nearest(z, p)
        xs.append(x); ps.append(p[idx]); ws.append(np.full(len(x), w_vert / len(x)))
        cost += w_vert / len(x) * d2.sum()
    if w_point > 0:
        idx, d2 = nearest(p, z)
        xs.append(x[idx]); ps.append(p); ws.append(np.full(len(p), w_point / len(p)))
        cost += w_point / len(p) * d2.sum()
    return np.concatenate(xs), np.concatenate(ps), np.concatenate(ws), cost


def kabsch(xs, ps, w, c_x=None, c_p=None):
    """weighted least-squares rigid fit by SVD -> (R, t, determined), summed as the header says on coordinates centred at c_x / c_p.
    determined: the header's rank test, with l1 - l2 of Horn's matrix written through the singular values of H:
    2 (s2 + sign(det H) s3)"""
    c_x = np.zeros(3) if c_x is None else np.asarray(c_x, np.float64)
    c_p = np.zeros(3) if c_p is None else np.asarray(c_p, np.float64)
    xc, pc = xs - c_x, ps - c_p
    W = w.sum()
    mx, mp = (w[:, None] * xc).sum(0) / W, (w[:, None] * pc).sum(0) / W
    H = (w[:, None, None] * (xc - mx)[:, :, None] * (pc - mp)[:, None, :]).sum(0)
    U, s, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(U) * np.linalg.det(Vt))
    d = 1.0 if d == 0 else d
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    scale = np.sqrt((w * (xc ** 2).sum(1)).sum() * (w * (pc ** 2).sum(1)).sum())
    gap = 2.0 * (s[1] + d * s[2])
    return R, (c_p + mp) - R @ (c_x + mx), bool(gap > RANK_EPS * scale)


def iterate(x, p, R, t, w_point=1.0, w_vert=1.0):
    """one iteration -> (R, t, cost before the solve, kept)"""
    xs, ps, w, cost = pairs(x, p, R, t, w_point, w_vert)
    Rn, tn, determined = kabsch(xs, ps, w, x.mean(0), p.mean(0))
    if not determined:
        W = w.sum()
        mx, mp = (w[:, None] * xs).sum(0) / W, (w[:, None] * ps).sum(0) / W
        return R, mp - R @ mx, cost, 1
    return Rn, tn, cost, 0


def align(x, p, starts=None, iterations=RECOVERY_ITERATIONS, w_point=1.0, w_vert=1.0):
    """the whole call for one mesh in float64 -> dict(R (K,3,3), t (K,3), scores (K,), best, kept (K,), history (K,I+1))"""
    x, p = np.asarray(x, np.float64), np.asarray(p, np.float64)
    starts = cube_rotations() if starts is None else np.asarray(starts, np.float64)
    K = len(starts)
    Rs, ts, scores, kept, hist = np.empty((K, 3, 3)), np.empty((K, 3)), np.empty(K), np.zeros(K, int), np.empty((K, iterations + 1))
    for k in range(K):
        R, t = start_transform(starts[k], x, p)
        for it in range(iterations):
            Rn, tn, hist[k, it], kp = iterate(x, p, R, t, w_point, w_vert)
            if kp == 0 and np.array_equal(Rn, R) and np.array_equal(tn, t):
                hist[k, it:iterations] = hist[k, it]      # a fixed point: every later iteration repeats this one bit for bit
                break
            R, t = Rn, tn
            kept[k] += kp
        scores[k] = pairs(x, p, R, t, w_point, w_vert)[3]
        hist[k, iterations] = scores[k]
        Rs[k], ts[k] = R, t
    return dict(R=Rs, t=ts, scores=scores, best=int(np.argmin(scores)), kept=kept, history=hist)


def rotation_angle(Ra, Rb):
    """the angle of Ra Rb^T in radians, from the skew part and the trace (accurate near 0, where arccos of the trace is not)"""
    D = np.asarray(Ra, np.float64) @ np.asarray(Rb, np.float64).T
    s = 0.5 * np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return float(np.arctan2(s, 0.5 * (np.trace(D) - 1.0)))


def axis_angle(axis, degrees):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    th = np.deg2rad(degrees)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


# ---- the meshes ---------------------------------------------------------------------------------------------------------------
def lopsided_blob(V=161, seed=7):
    """a point set with no rotational symmetry: a long body, a head off its axis at one end, one leg.  float32, extent about 2"""
    rs = np.random.RandomState(seed)
    nb, nh = V // 2, V // 4
    body = rs.randn(nb, 3) * [0.45, 0.18, 0.12]
    head = rs.randn(nh, 3) * [0.10, 0.12, 0.08] + [0.75, 0.30, 0.10]
    leg = rs.randn(V - nb - nh, 3) * [0.05, 0.20, 0.05] + [-0.35, -0.40, 0.15]
    return np.ascontiguousarray(np.concatenate([body, head, leg]), np.float32)


def moved(x, R, t):
    """the float32 points R x + t of float32 vertices, formed in float64 and rounded once"""
    return np.ascontiguousarray(x.astype(np.float64) @ np.asarray(R).T + np.asarray(t), np.float32)


def _recovery_cases():
    cube = cube_rotations()
    x = lopsided_blob()
    extent = float((x.max(0) - x.min(0)).max())
    table = [
        ("identity", np.eye(3), np.zeros(3), None, 1.0),
        ("back_to_front", axis_angle([0, 1, 0], 180.0), np.zeros(3), None, 1.0),
        ("cube5_skew15", cube[5] @ axis_angle([1, 2, 3], 15.0), np.array([0.05, -0.02, 0.03]), None, 1.0),
        ("cube13_skew25", cube[13] @ axis_angle([-2, 1, 0.5], 25.0), np.array([-0.1, 0.04, 0.0]), None, 1.0),
        ("cube22_skew20_offset", cube[22] @ axis_angle([0.3, -1, 2], 20.0), np.array([0.5 * extent, -0.25 * extent, 0.1]), None, 1.0),
        ("cube9_skew18_subset", cube[9] @ axis_angle([2, 0.5, -1], 18.0), np.array([0.02, 0.03, -0.04]), slice(0, None, 2), 0.0),
    ]
    out = {}
    for name, R, t, subset, w_vert in table:
        p = moved(x, R, t)
        out[name] = dict(name=name, x=x, p=p if subset is None else np.ascontiguousarray(p[subset]), R=R, t=np.asarray(t, np.float64),
                         w_point=1.0, w_vert=w_vert, extent=extent)
    return out


RECOVERY_CASES = _recovery_cases()
_REFERENCE = {}


def reference(name):
    """align() of a recovery case from the 24 built-in starts, computed once and shared by the tests that need it"""
    if name not in _REFERENCE:
        c = RECOVERY_CASES[name]
        _REFERENCE[name] = align(c["x"], c["p"], None, RECOVERY_ITERATIONS, c["w_point"], c["w_vert"])
    return _REFERENCE[name]
BATCH_CASE = ("cube5_skew15", "cube13_skew25", "cube22_skew20_offset")     # N = 3, a different R* per mesh, one V and S


# ---- rank-deficient sets ---------------------------------------------------------------------------------------------------------
def coincident_points(S=65):
    return np.ascontiguousarray(np.tile(np.array([[0.3, -0.2, 0.5]], np.float32), (S, 1)))


def collinear_points(S=65, seed=3):
    rs = np.random.RandomState(seed)
    s = rs.uniform(-1, 1, S)
    return np.ascontiguousarray(np.array([0.1, 0.2, -0.1]) + s[:, None] * np.array([0.6, -0.3, 0.74]), np.float32)
