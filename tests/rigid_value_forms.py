"""The rigid pre-alignment (smalfit_rigid_align, smalfit_trimmed_rigid_align) and its host fold away from the 161-point blob at the
origin: the cases, the restated window and the references of tests/test_rigid_value_forms_cpu.py (the host shims) and
tests/test_gpu_rigid_value_forms.py (HIP through eng.RigidAligner).  Nothing here asserts or needs a GPU.

  A  scale       the same call at scale 1 and at 2^k.  Every float32 result of degree p in the lengths is 2^(p k) times the unscaled
                 BITS (DEGREES) as long as no intermediate leaves the normal range: scale_window restates, from float64 magnitudes
                 of the named intermediates of an iteration and their degrees, the k for which that holds.
  B  place       the blob on multiples of 2^-7, vertices and points shifted by o (1, -1, 0.5), o in 16, 1024, 65536: the shifted
                 inputs are exact in float32, but a transform is about the origin: t = c_P - R c_X is rounded at the size of o.
                 Nothing is bit-exact; the device is held to the float64 restatement on the same float32 inputs.
  C  non-finite  a batch of three in which one coordinate of mesh 1 is NaN or +inf: the other two meshes keep their bits, mesh 1
                 keeps the header's promise ("stay in bounds, value unspecified").
  D  template    the reference's SMAL template mesh (3889 vertices: four staged chunks of 1024) against itself moved.
  E  host fold   fitter_3d.trainer._rotation_exp / _rotation_log at the axes and angles where the conversion changes branch.

Admission (a recovery case counts only if the float64 restatement alone recovers R*):
  place          the points are snapped to the 2^-7 lattice as the vertices are (at o = 65536 float32 holds nothing finer), so no
                 rigid motion brings the pairs to distance 0 and the restatement ends a snapping error away from R*: PLACE_ADMISSION
                 bounds that error from the lattice, rc.RECOVERY_ADMISSION (for exact correspondences) cannot apply.  The device is
                 held to the restatement's own answer, not to R*.
  template       admitted untrimmed within rc.RECOVERY_ADMISSION (the mirror image of the rest pose is not a rotation of it: the
                 true start wins), and trimmed within TEMPLATE_TRIM_ADMISSION: its points are drawn on faces, the restatement ends a
                 sampling error from R* and the device is held to the restatement's answer.  The CPU file runs both."""
from __future__ import annotations

import math

import numpy as np

from tests import host_rigid_align as hr
from tests import host_rigid_trim as ht
from tests import rigid_align_cases as rc
from tests import rigid_trim_cases as tc
from tests.mesh3d_value_forms import (DIRECTION, EPS32, FLT_MAX, FLT_MIN, LATTICE, OFFSETS, SCALES, ldexp32, same_bits,  # noqa: F401
                                      times, window)

K = 24
WEIGHTS = ((1.0, 1.0), (1.0, 0.0), (0.0, 1.0))      # (w_point, w_vert): both ways, each single direction
SCALE_ITERATIONS = 30                               # of the GPU test
SCALE_ITERATIONS_CPU = 6                            # of the shim's batch test (a Python loop over the shim's iterations)
# what an output is multiplied by under a scale 2^k: key -> degree p (None: identical; a tuple: per entry of the last axis)
_T_DEGREES = (0, 0, 0, 1) * 3
DEGREES = dict(transforms=_T_DEGREES, scores=2, best=None, best_transform=_T_DEGREES, kept_rotation=None, history=2, vert_nn=None,
               point_nn=None, vert_kept=None, point_kept=None, trim_d2=2)
TRIM_KEYS = ("vert_kept", "point_kept", "trim_d2")
# one k outside each edge of the window (CPU only): below, d^2 itself (degree 2, about 1e-2 .. 1e1 at scale 1) is subnormal or 0;
# above, d^2 of the far starts is +inf
OUTSIDE = (-80, 70)
# where the rank test's right-hand side as sqrtf(M[16] * M[17]), of degree 4, overflowed to +inf and underflowed to 0 on the blob
RANK_RHS_OVERFLOWED_AT, RANK_RHS_UNDERFLOWED_AT = 33, -40

PLACE_ITERATIONS = 30
POSITION_CAP_ULPS = 4.0                 # max |z_device - z_64| in ulp(L), L the largest absolute input coordinate: a condition
# rad.  Snapping moves every coordinate of a vertex and of a point by a uniform error of standard deviation LATTICE / sqrt(12), a
# pair's residual by sqrt(2) of that; a least-squares rotation over n such pairs is off, about its weakest axis, by a standard
# deviation of that residual / (r sqrt(n)), r the blob's rms distance from its long axis (0.256: the root of the sum of its two
# smaller variances, 0.0119 + 0.0534): 9.8e-4 rad for n = 161.  Ten of those; a wrong basin is a quarter turn away
PLACE_ADMISSION = 10 * math.sqrt(2.0 / 12.0) * LATTICE / (0.256 * math.sqrt(161))

ROTATION_ROUNDINGS = 64                 # exp, the SVD projection, log and the measurement: float64 roundings of numbers below pi
FOLD_BOUND = ROTATION_ROUNDINGS * float(np.finfo(np.float64).eps)    # rad, beyond the yardstick (R against its own projection)
SENTINEL, BYTE_SENTINEL, GUARD = -7, 0xA5, 64


# ---- the whole call on the float32 host shims -------------------------------------------------------------------------------------
def pick(scores):
    """best: the lowest score, the lowest k among equal ones; a NaN never wins (all NaN: 0)"""
    b, bs = -1, 0.0
    for k, sc in enumerate(scores):
        if sc == sc and (b < 0 or sc < bs):
            b, bs = k, sc
    return max(b, 0)


def shim_align(x, p, iterations, w_point=1.0, w_vert=1.0, keep=None, start_transforms=None, starts=None):
    """the whole call for one mesh on the float32 shims -> the device's outputs without the mesh axis.  keep: None (untrimmed:
    host_rigid_align) or (keep_point, keep_vert) (host_rigid_trim).  The shim adds a direction's pairs in plain ascending order,
    the kernels in blocks of 64: the matches under a given transform are the device's, the sums agree to rounding"""
    x, p = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(p, np.float32)
    V, S = len(x), len(p)
    if start_transforms is None:
        cX, cP = hr.means(x), hr.means(p)
        cube = hr.cube_rotations() if starts is None else np.asarray(starts, np.float32)
        start_transforms = np.stack([hr.start_transform(R, cX, cP) for R in cube])
    Kc = len(start_transforms)

    def one(T):
        if keep is None:
            return hr.iterate(x, p, T, w_point, w_vert)
        return ht.iterate(x, p, T, keep[0], keep[1], w_point, w_vert)

    o = dict(transforms=np.empty((Kc, 12), np.float32), scores=np.empty(Kc, np.float32), kept_rotation=np.zeros(Kc, np.int32),
             history=np.empty((Kc, iterations + 1), np.float32), vert_nn=np.full((Kc, V), SENTINEL, np.int32),
             point_nn=np.full((Kc, S), SENTINEL, np.int32))
    if keep is not None:
        o.update(vert_kept=np.full((Kc, V), BYTE_SENTINEL, np.uint8), point_kept=np.full((Kc, S), BYTE_SENTINEL, np.uint8),
                 trim_d2=np.zeros((Kc, 2), np.float32))
    for k in range(Kc):
        T = np.asarray(start_transforms[k], np.float32).reshape(12)
        for it in range(iterations):
            r = one(T)
            o["history"][k, it] = r["cost"]
            o["kept_rotation"][k] += r["kept"]
            T = r["T"]
        r = one(T)                                  # the score's round: one more pair of scans, its solve is not used
        o["transforms"][k], o["scores"][k], o["history"][k, iterations] = T, r["cost"], r["cost"]
        if w_vert > 0:
            o["vert_nn"][k] = r["idx_v"]
        if w_point > 0:
            o["point_nn"][k] = r["idx_p"]
        if keep is not None:
            if w_vert > 0:
                o["vert_kept"][k] = r["kept_v"]
            if w_point > 0:
                o["point_kept"][k] = r["kept_p"]
            o["trim_d2"][k] = r["trim_d2"]
    o["best"] = np.int32(pick(o["scores"]))
    o["best_transform"] = o["transforms"][int(o["best"])].copy()
    return o


def scaled_equal(unit, scaled, k, keys=None):
    """-> the keys of `scaled` that are not the bits of `unit` times 2^(degree k)"""
    return [key for key in (keys or sorted(unit)) if key in DEGREES and not same_bits(times(unit[key], DEGREES[key], k), scaled[key])]


# ---- A: the cases and the window ---------------------------------------------------------------------------------------------------
def batch():
    """rc.BATCH_CASE: N = 3, a different R* per mesh -> (x (3,161,3), p (3,161,3))"""
    cs = [rc.RECOVERY_CASES[n] for n in rc.BATCH_CASE]
    return np.stack([c["x"] for c in cs]), np.stack([c["p"] for c in cs])


def partial():
    """tc.PARTIAL_CASES['cube5_skew15'] -> (x (161,3), p (136,3), keep_point, keep_vert)"""
    c = tc.PARTIAL_CASES["cube5_skew15"]
    return c["x"], c["p"], c["keep_point"], c["keep_vert"]


def _spacing32(a):
    """the distance from |a| rounded to float32 to the next float32 above it"""
    return np.spacing(np.abs(np.asarray(a)).astype(np.float32)).astype(np.float64)


def iteration_items(x, p, R, t, w_point, w_vert, keep=None):
    """(magnitudes, degree) of the named float32 intermediates of one iteration under [R | t], in float64: the scans' differences
    and d^2, each direction's 19 unweighted sums (as the blocks' slots and their running totals hold them: bounded by the sums of
    the absolute values), the 19 combined sums, the weighted means, H, Horn's 4x4 matrix, the two roots of the rank test and their
    product, and the translation"""
    x, p = np.asarray(x, np.float64), np.asarray(p, np.float64)
    cX, cP = x.mean(0), p.mean(0)
    z = x @ R.T + t
    items = [(z, 1), (t, 1)]
    M = np.zeros(19)
    for on, q, o, count, kp, qx in ((w_vert > 0, z, p, len(x), None if keep is None else keep[1], True),
                                    (w_point > 0, p, z, len(p), None if keep is None else keep[0], False)):
        if not on:
            continue
        idx, d2 = rc.nearest(q, o)
        d = q - o[idx]
        sel = np.ones(len(q), bool) if kp is None else tc.select(d2, kp)
        xs, ps = (x[sel], p[idx[sel]]) if qx else (x[idx[sel]], p[sel])
        xc, pc = xs - cX, ps - cP
        rows = np.concatenate([np.ones((len(xc), 1)), xc, pc, (xc[:, :, None] * pc[:, None, :]).reshape(-1, 9),
                               (xc ** 2).sum(1, keepdims=True), (pc ** 2).sum(1, keepdims=True), d2[sel][:, None]], 1)
        # a difference of two float32 numbers is a multiple of the spacing of the smaller: where a correspondence is exact, d is
        # rounding alone and its square is the smallest d^2 there is
        u = np.minimum(_spacing32(q), _spacing32(o[idx]))
        items += [(d, 1), (d * d, 2), (d2, 2), (u, 1), (u * u, 2)]
        deg = (0,) + (1,) * 6 + (2,) * 12
        for i in range(19):
            items += [(rows[:, i], deg[i]), (np.abs(rows[:, i]).sum(), deg[i])]
        M += (w_vert if qx else w_point) / count * rows.sum(0)
    W = M[0]
    mx, mp = M[1:4] / W, M[4:7] / W
    H = M[7:16].reshape(3, 3) - np.outer(M[1:4], mp)
    A = np.array([[H[0, 0] + H[1, 1] + H[2, 2], H[1, 2] - H[2, 1], H[2, 0] - H[0, 2], H[0, 1] - H[1, 0]],
                  [0, H[0, 0] - H[1, 1] - H[2, 2], H[0, 1] + H[1, 0], H[2, 0] + H[0, 2]],
                  [0, 0, -H[0, 0] + H[1, 1] - H[2, 2], H[1, 2] + H[2, 1]],
                  [0, 0, 0, -H[0, 0] - H[1, 1] + H[2, 2]]])
    ra, rb = math.sqrt(M[16]), math.sqrt(M[17])
    items += [(M[1:7], 1), (M[7:19], 2), (mx, 1), (mp, 1), (cX + mx, 1), (cP + mp, 1), (H, 2), (np.outer(M[1:4], mp), 2), (A, 2),
              (np.abs(H).sum(), 2), (np.linalg.eigvalsh(A + A.T - np.diag(np.diag(A))), 2), (ra, 1), (rb, 1),
              (rc.RANK_EPS * ra * rb, 2)]
    return items


def scale_items(x, p, w_point, w_vert, keep=None, trace_iterations=3):
    """iteration_items along the float64 restatement: every start's first `trace_iterations` rounds"""
    x, p = np.asarray(x, np.float64), np.asarray(p, np.float64)
    items = []
    for R0 in rc.cube_rotations():
        R, t = rc.start_transform(R0, x, p)
        for _ in range(trace_iterations + 1):
            items += iteration_items(x, p, R, t, w_point, w_vert, keep)
            if keep is None:
                R, t = rc.iterate(x, p, R, t, w_point, w_vert)[:2]
            else:
                R, t = tc.iterate(x, p, R, t, w_point, w_vert, keep[0], keep[1])[:2]
    return items


def scale_window(x, p, w_point=1.0, w_vert=1.0, keep=None):
    """(lo, hi): for lo <= k <= hi every named intermediate that is not 0 stays a normal float32 number at scale 2^k.  One binade is
    taken off the top: the magnitudes are float64 sums, a float32 running total may round above them.  A sum that cancels (the
    centred coordinates of a whole direction) is far smaller in float64 than float32's own rounding leaves it: the lower edge is
    conservative"""
    lo, hi = window(scale_items(x, p, w_point, w_vert, keep))
    return lo, hi - 1


def old_rank_window(x, p):
    """the k for which the product under the old root, sum w |x|^2 sum w |p|^2 of degree 4, stayed normal"""
    x, p = np.asarray(x, np.float64), np.asarray(p, np.float64)
    prod = ((x - x.mean(0)) ** 2).sum(1).mean() * ((p - p.mean(0)) ** 2).sum(1).mean() * 2.0 * 2.0   # both directions: W = 2
    return window([(prod, 4)])


# ---- B: place ----------------------------------------------------------------------------------------------------------------------
def snapped(a):
    return np.ascontiguousarray(np.round(np.asarray(a, np.float64) / LATTICE) * LATTICE, np.float32)


def place_case(o, trimmed):
    """the blob (trimmed: the partial case) on the lattice, vertices and points shifted by o DIRECTION -> dict(x, p, R, keep, L,
    ulp): every coordinate exact in float32"""
    if trimmed:
        x, p, kp, kv = partial()
        keep = (kp, kv)
    else:
        c = rc.RECOVERY_CASES["cube5_skew15"]
        x, p, keep = c["x"], c["p"], None
    shift = o * DIRECTION
    xs, ps = snapped(x).astype(np.float64) + shift, snapped(p).astype(np.float64) + shift
    x32, p32 = np.ascontiguousarray(xs, np.float32), np.ascontiguousarray(ps, np.float32)
    assert np.array_equal(x32.astype(np.float64), xs) and np.array_equal(p32.astype(np.float64), ps)
    L = np.float32(max(np.abs(x32).max(), np.abs(p32).max()))
    return dict(x=x32, p=p32, R=rc.RECOVERY_CASES["cube5_skew15"]["R"], keep=keep, L=float(L), ulp=float(np.spacing(L)))


_PLACE = {}


def place_reference(o, trimmed):
    """the float64 restatement on the shifted float32 inputs, computed once"""
    if (o, trimmed) not in _PLACE:
        c = place_case(o, trimmed)
        if trimmed:
            _PLACE[o, trimmed] = tc.align(c["x"], c["p"], c["keep"][0], c["keep"][1], None, PLACE_ITERATIONS)
        else:
            _PLACE[o, trimmed] = rc.align(c["x"], c["p"], None, PLACE_ITERATIONS)
    return _PLACE[o, trimmed]


def winner_margin(case, ref):
    """-> (gap, blur).  gap: by how much the restatement's lowest score lies below the lowest score of a start that ended at
    another rotation (more than 1e-3 rad from the winner's).  blur: what a mean of d^2 of that size moves by when every distance
    moves by one ulp(L), 2 sqrt(score) ulp + ulp^2: what float32 at that place cannot tell apart.  `best` and the winner's rotation
    are the restatement's only where gap > blur"""
    b = ref["best"]
    other = [ref["scores"][k] for k in range(len(ref["scores"])) if rc.rotation_angle(ref["R"][k], ref["R"][b]) > 1e-3]
    u = case["ulp"]
    return float(min(other) - ref["scores"][b]), float(2.0 * math.sqrt(ref["scores"][b]) * u + u * u)


# (o, trimmed) of the place cases that are run.  NOT admitted, by winner_margin: the trimmed partial case at o = 1024 and 65536.  Its
# starts 5 and 22 end 3e-3 rad apart at scores 3.0647e-5 and 3.0614e-5 (float64): a gap of 3.3e-8, below the blur of 1.4e-6 at 1024
# and 1.5e-4 at 65536 -- which of the two wins there is rounding, in any float32 implementation (the shim picks 5).  At o = 16 the
# blur is 2.2e-8 and the case is run.  tests/test_rigid_value_forms_cpu.py proves both statements
PLACE_CASES = tuple((o, False) for o in OFFSETS) + ((16, True),)
PLACE_NOT_ADMITTED = ((1024, True), (65536, True))
PLACE_IDS = tuple("%d-%s" % (o, "trimmed" if t else "untrimmed") for o, t in PLACE_CASES)


def split(T):
    T = np.asarray(T, np.float64).reshape(np.shape(T)[:-1] + (3, 4))
    return T[..., :3], T[..., 3]


def place_figures(case, ref, best, best_transform):
    """-> (angle between the rotations, max |z - z_64| in ulp(L)) of a float32 result against the restatement's winner; z is formed
    by the header's float32 chain, as every scan forms it"""
    R, _ = split(best_transform)
    b = ref["best"]
    z = hr.apply(best_transform, case["x"]).astype(np.float64)
    z64 = case["x"].astype(np.float64) @ ref["R"][b].T + ref["t"][b]
    return rc.rotation_angle(R, ref["R"][b]), float(np.abs(z - z64).max() / case["ulp"])


# ---- C: non-finite coordinates ----------------------------------------------------------------------------------------------------
NONFINITE = (("vertex", float("nan")), ("vertex", float("inf")), ("point", float("nan")), ("point", float("inf")))
NONFINITE_IDS = ("vertex-nan", "vertex-inf", "point-nan", "point-inf")
NONFINITE_ITERATIONS = 3


def poisoned(x, p, where, value):
    """(x, p) of a batch with one coordinate of mesh 1 replaced: vertex 70's second, or point 33's third"""
    x, p = x.copy(), p.copy()
    if where == "vertex":
        x[1, 70, 1] = value
    else:
        p[1, 33, 2] = value
    return x, p


def promise_violations(o, V, S, Kc, iterations, trimmed):
    """what of "stay in bounds" one mesh's outputs break (none expected): every index in {-1} u [0, count), every flag 0 or 1, best
    in [0, K), kept_rotation in [0, I], trim_d2 not negative (a NaN is not allowed there either: it is a kept key's d^2, or 0)"""
    bad = []
    if not (np.all(o["vert_nn"] >= -1) and np.all(o["vert_nn"] < S)):
        bad.append("vert_nn")
    if not (np.all(o["point_nn"] >= -1) and np.all(o["point_nn"] < V)):
        bad.append("point_nn")
    if not 0 <= int(o["best"]) < Kc:
        bad.append("best")
    if not (np.all(o["kept_rotation"] >= 0) and np.all(o["kept_rotation"] <= iterations)):
        bad.append("kept_rotation")
    if trimmed:
        for key in ("vert_kept", "point_kept"):
            if not np.all(o[key] <= 1):
                bad.append(key)
        if not np.all(o["trim_d2"] >= 0):
            bad.append("trim_d2")
    return bad


# ---- D: the template ----------------------------------------------------------------------------------------------------------------
TEMPLATE_SHIFT = np.array([0.3, -0.2, 0.1])
TEMPLATE_POSE = "cube13_skew25"
TEMPLATE_ITERATIONS = 30
TEMPLATE_TRIM = (0.8, 0.56)             # trim_point, trim_vert: tc.MODEL_TRIM_POINT / MODEL_TRIM_VERT
TEMPLATE_TRUE_START, TEMPLATE_TRIM_TRUE_START = 13, 9      # the cube rotation under TEMPLATE_POSE, under tc.MODEL_TURN
# rad.  The trimmed case's points are drawn ON the faces of the partial target, not at its vertices: no rigid motion brings the kept
# pairs to distance 0 and the restatement itself ends a sampling error from R* (tests/rigid_trim_cases.py: MODEL_ADMISSION, the same
# rule on the stand-in model).  The device is held to the restatement's own answer under the recovery caps, not to this bound
TEMPLATE_TRIM_ADMISSION = tc.MODEL_ADMISSION


def template_case():
    """-> dict(x (3889,3), p (3889,3), faces, R, t, extent): the template's vertices and themselves moved by TEMPLATE_POSE's
    rotation and TEMPLATE_SHIFT"""
    from tests import template_cases as tpl
    x, faces = tpl.template()
    x = np.ascontiguousarray(x, np.float32)
    R = rc.RECOVERY_CASES[TEMPLATE_POSE]["R"]
    return dict(x=x, p=rc.moved(x, R, TEMPLATE_SHIFT), faces=faces, R=R, t=TEMPLATE_SHIFT, extent=float((x.max(0) - x.min(0)).max()))


def template_partial():
    """-> dict(x, p, keep_point, keep_vert): the template against S = 3889 points drawn on tc.partial_target of it"""
    c = template_case()
    tv, tf, _ = tc.partial_target(c["x"], c["faces"])
    p = tc.draw_points(tv, tf, len(c["x"]), seed=3)
    V, S = len(c["x"]), len(p)
    L = np.float32(max(np.abs(c["x"]).max(), np.abs(p).max()))
    return dict(x=c["x"], p=p, keep_point=ht.keep_count(TEMPLATE_TRIM[0], S), keep_vert=ht.keep_count(TEMPLATE_TRIM[1], V),
                trim_point=TEMPLATE_TRIM[0], trim_vert=TEMPLATE_TRIM[1], R=tc.MODEL_TURN, t=tc.MODEL_SHIFT, extent=c["extent"],
                ulp=float(np.spacing(L)))


_TEMPLATE_REF = {}


def template_reference(trimmed=False):
    """the float64 restatement from the 24 starts with tc.nearest_tree for the scans (the (Q,O,3) table of rc.nearest does not fit
    3889 x 3889), computed once per process (11 to 14 s): tc.align at keep == the count in both directions is the untrimmed call"""
    if trimmed not in _TEMPLATE_REF:
        if trimmed:
            c = template_partial()
            _TEMPLATE_REF[trimmed] = tc.align(c["x"], c["p"], c["keep_point"], c["keep_vert"], None, TEMPLATE_ITERATIONS, nearest=tc.nearest_tree)
        else:
            c = template_case()
            _TEMPLATE_REF[trimmed] = tc.align(c["x"], c["p"], len(c["p"]), len(c["x"]), None, TEMPLATE_ITERATIONS, nearest=tc.nearest_tree)
    return _TEMPLATE_REF[trimmed]


def template_margin(ref, ulp):
    """winner_margin's rule for a template case: -> (gap, blur), the lowest score of a start that ended more than 1e-3 rad from the
    winner's rotation minus the winner's, and what a mean of d^2 of the winner's size moves by when every distance moves by `ulp`"""
    return winner_margin(dict(ulp=ulp), ref)


# ---- E: the host fold ---------------------------------------------------------------------------------------------------------------
def _unit(a):
    a = np.asarray(a, np.float64)
    return a / np.linalg.norm(a)


FOLD_AXES = {"x": _unit([1, 0, 0]), "y": _unit([0, 1, 0]), "z": _unit([0, 0, 1]), "-z": _unit([0, 0, -1]),
             "diag": _unit([1, 1, 1]), "-diag": _unit([-1, -1, -1]), "near_x": _unit([1, 1e-7, 0]), "near_x_2": _unit([1, -1e-4, 2e-9]),
             "near_diag": _unit([1, 1, 1 + 1e-9]), "skew": _unit([0.3, -2, 1])}
PI = math.pi
# 0; tiny; either side of the small-angle branch of log (skew norm 1e-6) and of exp (1e-8); a quarter turn, where log changes from the
# skew part to the quaternion; 1, 3; close to pi from below; pi
FOLD_ANGLES = (0.0, 1e-12, 1e-9, 0.9e-8, 1.1e-8, 0.5e-6, 0.99e-6, 1.01e-6, 2e-6, 1.0, PI / 2 - 1e-9, PI / 2, PI / 2 + 1e-9, 3.0,
               PI - 1e-3, PI - 2e-6, PI - 1.01e-6, PI - 1e-6, PI - 0.99e-6, PI - 5e-7, PI - 1e-9, PI)


def rodrigues(axis, angle):
    """the rotation about a unit axis in float64, written out apart from the code under test"""
    a = np.asarray(axis, np.float64)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * Kx + (2.0 * math.sin(0.5 * angle) ** 2) * (Kx @ Kx)


def projection(R):
    """the rotation nearest to R (SVD): the yardstick of a matrix that is not exactly orthonormal"""
    U, _, Vt = np.linalg.svd(np.asarray(R, np.float64))
    return U @ np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt)) or 1.0]) @ Vt


def fold_matrices():
    """-> [(id, R (3,3) float64)]: every axis at every angle, as float64 and rounded to float32"""
    out = []
    for an, a in FOLD_AXES.items():
        for th in FOLD_ANGLES:
            R = rodrigues(a, th)
            out.append(("%s/%.17g/f64" % (an, th), R))
            out.append(("%s/%.17g/f32" % (an, th), R.astype(np.float32).astype(np.float64)))
    return out
