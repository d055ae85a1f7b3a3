"""The point-to-surface term on the device (mesh3d_surface_near / hit / grad / reduce of kernels_mesh3d.inc behind
MeshObjective.surface and smalfit_fit3d_step_surface; the definition is this project's, include/smalfit.h) (-m gpu):

  shapes        queries in 1, 63, 64, 65, 130 (a topology needs three vertices: 3 stands for 1 in the vertex direction) and
                scanned triangles in scanned_counts(chunk) plus the counts either side of every slice boundary the slice rule
                gives them, in both directions, on soup / ribbon meshes, at N = 1 and on a ragged batch of 3
  distances     |r| against float64 within 89 ulp(L); the returned face's own float64 distance within delta of the least; q
                rebuilt in float64 from the returned (face, barycentrics) within the conditioning rule of
                tests/surface_term_cases.py, the oracle's flagged share asserted first
  assembly      dverts / dtrans against float64 sums formed from the RETURNED correspondences (faces, barycentrics, residuals)
                within (contributions per vertex + 2) 2^-23 x the largest contribution: float32 summation only; rows and losses
                within count 2^-24 relative
  whole         <dverts, u> for three smooth directions against the float64 oracle's central difference of the term: at most 4 x
                what the float32 numpy yardstick deviates by on the same inputs, and at most 3 x what these kernels measured when
                tests/golden/hip_surface_term_measured.json was written (SMALFIT_WRITE_SURFACE_TERM_MEASURED=<path> writes it)
  exact         a mesh against itself; the cube against its shifted copies; ragged = one-mesh calls; two calls; a smaller call
                after a larger; one direction; refusals
  the step      smalfit_fit3d_step == smalfit_fit3d_step_surface(NULL) == both weights 0, bit for bit; fused against unfused
                with the term on; chamfer off and point-surface on
  descent       30 Adam steps on the cube's vertices against the float64 numpy loop of the same recipe
  front end     Stage(loss_weights={"w_point_surface": ...}) and the same key from a YAML file

Every figure is printed before it is judged.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from smalify_amd import _lib                        # noqa: E402
from smalify_amd import engine as eng               # noqa: E402
from tests import host_surface_term as hs           # noqa: E402
from tests import mesh3d_cases as m3                # noqa: E402
from tests import mesh_score_cases as mc            # noqa: E402
from tests import surface_term_cases as sc          # noqa: E402

MEASURED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hip_surface_term_measured.json")
CHUNK = int(hs.load().hst_surface_chunk())
DEV = "cuda"
ULP = 2.0 ** -23


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """a device error ends the session: nothing more is started on a GPU that has just faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:
        pytest.exit("device error, stopping: %s" % exc, returncode=3)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def _surface(fit, faces, targets, points, w_ps=1.0, w_vs=1.0, max_points=130, objective=None, correspondences=True):
    """fit (N,V,3); targets: list of N (verts, faces) or None; points (N,S,3) or None -> (host dict, objective)"""
    N, V = fit.shape[:2]
    obj = objective or eng.MeshObjective(V, faces, N, max_points)
    tg = eng.MeshTargets([t[0] for t in targets], [t[1] for t in targets]) if targets is not None else None
    o = obj.surface(_t(fit), tg, None if points is None else _t(points), w_ps, w_vs, correspondences=correspondences)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}, obj


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same_bits(a, b, what=""):
    assert set(a) == set(b), what
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(_bits(a[k]), _bits(b[k])), (what, k)


def _check_direction(tag, q, sv, sf, face, bary, resid):
    """one mesh, one direction: distances, selection and the closest point against float64"""
    L_ulp = mc.ulp_l(q, sv)
    delta = sc.DELTA_ULP * L_ulp
    o64 = sc.nearest(q, sv, sf, delta=delta)
    d64 = np.sqrt(o64["d2"])
    share = o64["flagged"].mean()
    assert share <= sc.FLAG_CAP, (tag, "the oracle flags too many", share)
    assert ((face >= 0) & (face < len(sf))).all(), tag
    dev = np.abs(np.linalg.norm(resid.astype(np.float64), axis=1) - d64).max() / L_ulp
    own = np.abs(sc.face_dist(q, sv, sf, face) - d64).max() / L_ulp
    q_got = sc.point_from(sv, sf, face, bary)
    off = np.linalg.norm(q_got - o64["q"], axis=1)
    ok = (off <= sc.reach(d64, delta)) | o64["flagged"]
    print("%-34s |r| %6.2f ulp(L)  face's own %6.2f ulp(L)  q off %.2e  flagged %d/%d" % (tag, dev, own, off.max(), o64["flagged"].sum(), len(q)))
    assert dev <= sc.DELTA_ULP and own <= sc.DELTA_ULP, tag
    assert ok.all(), (tag, np.nonzero(~ok)[0][:5])
    assert (bary >= 0).all() and np.abs(bary.astype(np.float64).sum(1) - 1).max() <= 4 * ULP, tag
    # the residual names that point too: the gradient is formed from it, not from the barycentrics
    off_r = np.linalg.norm(np.asarray(q, np.float64) - resid - o64["q"], axis=1)
    assert ((off_r <= sc.reach(d64, delta)) | o64["flagged"]).all(), tag


def _check_call(tag, o, fit, faces, targets, pts, w_ps, w_vs):
    """everything one call returned against float64: per direction the correspondences, then the assembly from them"""
    N, V = fit.shape[:2]
    want = np.zeros((N, V, 3))
    count = np.zeros((N, V))
    largest = 0.0
    rows = np.zeros((N, 2))
    if w_ps > 0:
        S = pts.shape[1]
        for n in range(N):
            _check_direction("%s/mesh%d/points" % (tag, n), pts[n], fit[n], faces, o["point_face"][n], o["point_bary"][n], o["point_residual"][n])
            r = o["point_residual"][n].astype(np.float64)
            rows[n, 0] = (r * r).sum()
            corners = np.asarray(faces)[o["point_face"][n]]
            for i in range(3):
                c = -w_ps * 2.0 / (N * S) * o["point_bary"][n][:, i:i + 1].astype(np.float64) * r
                np.add.at(want[n], corners[:, i], c)
                np.add.at(count[n], corners[:, i], 1)
                largest = max(largest, np.abs(c).max())
    if w_vs > 0:
        for n in range(N):
            _check_direction("%s/mesh%d/verts" % (tag, n), fit[n], targets[n][0], targets[n][1], o["vert_face"][n], o["vert_bary"][n],
                             o["vert_residual"][n])
            r = o["vert_residual"][n].astype(np.float64)
            rows[n, 1] = (r * r).sum()
            c = w_vs * 2.0 / (N * V) * r
            want[n] += c
            count[n] += 1
            largest = max(largest, np.abs(c).max())
    bound = (count + 2)[:, :, None] * ULP * largest
    err = np.abs(o["dverts"] - want)
    print("%-34s dverts off by %.2e of the bound at worst" % (tag, (err / bound).max()))
    assert (err <= bound).all(), tag
    # d trans is the float32 sum of the device's own V gradients of a mesh, 64 to a block and the blocks one after the other:
    # the bound of a float32 sum of that many terms in any order
    own = o["dverts"].astype(np.float64)
    tb = (V + -(-V // 64)) * 2.0 ** -24 * np.abs(own).sum(1)
    assert (np.abs(o["dtrans"] - own.sum(1)) <= tb).all(), (tag, "dtrans")
    # rows: sum d^2 per mesh (d^2 = |r|^2 up to the rounding of a dot product), losses: the means
    for n in range(N):
        for d, cnt in ((0, pts.shape[1] if w_ps > 0 else 0), (1, V if w_vs > 0 else 0)):
            # f8's bound of a float32 sum, count 2^-24 -- of the device's d^2, which are not returned.  The reference here is the
            # sum of |r|^2 of the returned residuals, and a d^2 differs from its |r|^2 in rounding: a segment's is the rounded dot
            # product of r with itself (3 roundings), the plane's h^2 / |n|^2 against |(h / |n|^2) n|^2 (some 8 on either side):
            # 16 x 2^-24 relative per term, hence on the sum
            rel = (cnt + 16) * 2.0 ** -24
            assert abs(o["rows"][n, d] - rows[n, d]) <= rel * rows[n, d] + 1e-45, (tag, n, d, o["rows"][n, d], rows[n, d])
    # losses: the means of the device's own rows -- N terms added, one division; the term: two products and an addition
    dev_rows = o["rows"].astype(np.float64)
    L_ps = dev_rows[:, 0].sum() / (N * pts.shape[1]) if w_ps > 0 else 0.0
    L_vs = dev_rows[:, 1].sum() / (N * V) if w_vs > 0 else 0.0
    rel = (N + 1) * 2.0 ** -24
    assert abs(o["losses"][0] - L_ps) <= rel * L_ps and abs(o["losses"][1] - L_vs) <= rel * L_vs, (tag, o["losses"], L_ps, L_vs)
    term = max(w_ps, 0) * float(o["losses"][0]) + max(w_vs, 0) * float(o["losses"][1])
    assert abs(o["losses"][2] - term) <= 3 * 2.0 ** -24 * term, (tag, o["losses"], term)


# ---- shapes -----------------------------------------------------------------------------------------------------------------
def _counts_around(F0, queries):
    """F0 and the counts either side of every slice boundary the rule gives F0 triangles under `queries` queries, one mesh"""
    z = hs.slices(queries, F0, 1)
    span = -(-F0 // z)
    out = {F0}
    for k in range(1, z + 1):
        out |= {k * span - 1, k * span, k * span + 1}
    return sorted(f for f in out if f >= 1)


def _problem(F, S, seed, N=1, V=None):
    """N ribbons of F faces (V = F + 2 vertices) against N soups of F faces, S points near each soup"""
    V = V or F + 2
    fit = np.stack([mc.ribbon(V, seed=seed + 7 * n)[0] for n in range(N)])
    faces = mc.ribbon(V, seed=0)[1]
    targets = [mc.soup(F, seed=seed + 100 + n) for n in range(N)]
    pts = np.stack([mc.points_near(targets[n][0], targets[n][1], S, seed=seed + 200 + n, sigma=0.05) for n in range(N)])
    return fit, faces, targets, pts


def test_the_cases_reach_every_branch():
    assert set(mc.QUERY_COUNTS) == {1, 63, 64, 65, 130}
    for F0 in mc.scanned_counts(CHUNK):
        z = hs.slices(65, F0, 1)
        assert (z > 1) == (F0 >= 128), (F0, z)
        assert F0 in _counts_around(F0, 65)
    assert len(_counts_around(2 * CHUNK + 3, 65)) > 30 and _counts_around(5, 65) == [4, 5, 6]
    assert hs.slices(65, 2 * CHUNK + 3, 1) * -(-(2 * CHUNK + 3) // hs.slices(65, 2 * CHUNK + 3, 1)) >= 2 * CHUNK + 3
    # (a slice longer than the staged chunk needs queries that fill the chip by themselves: test_a_slice_longer_than_the_chunk)


@pytest.mark.parametrize("direction", ("verts", "points"))
@pytest.mark.parametrize("F0", mc.scanned_counts(CHUNK))
def test_scanned_counts_either_side_of_every_slice_boundary(F0, direction):
    """65 queries (two blocks, one of a single lane) against F scanned triangles: the target soup for the vertices, the fitted
    ribbon for the points"""
    for F in _counts_around(F0, 65):
        if direction == "verts":
            fit, faces = mc.ribbon(65, seed=F)
            targets = [mc.soup(F, seed=F + 100)]
            o, _ = _surface(fit[None], faces, targets, None, 0.0, 0.5, max_points=65)
            _check_call("verts/F%d" % F, o, fit[None], faces, targets, None, 0.0, 0.5)
        else:
            fit, faces = mc.ribbon(F + 2, seed=F)
            assert len(faces) == F
            pts = mc.points_near(fit, faces, 65, seed=F + 200, sigma=0.05)[None]
            o, _ = _surface(fit[None], faces, None, pts, 1.5, 0.0, max_points=65)
            _check_call("points/F%d" % F, o, fit[None], faces, None, pts, 1.5, 0.0)


@pytest.mark.parametrize("Q", mc.QUERY_COUNTS)
def test_query_counts(Q):
    for F in (5, CHUNK + 1):
        V = max(Q, 3)
        fit, faces, targets, pts = _problem(F, Q, seed=10 * Q + F, V=V)
        o, _ = _surface(fit, faces, targets, pts, 0.75, 1.25, max_points=Q)
        _check_call("Q%d_F%d" % (Q, F), o, fit, faces, targets, pts, 0.75, 1.25)


def test_a_slice_longer_than_the_chunk():
    """more than 512 query blocks: the rule gives ONE slice, and a block walks 2 CHUNK + 3 triangles in three staged chunks.
    The queries are 130 positions repeated, so every repeat must carry the bits of the 130-query call (sliced 16 ways, and
    judged against float64 here)"""
    F = 2 * CHUNK + 3
    Q = 513 * 64
    assert hs.slices(Q, F, 1) == 1 and hs.slices(130, F, 1) > 8
    reps = -(-Q // 130)
    # vertices against a target soup of F triangles
    sv, sfaces = mc.ribbon(130, seed=3)
    target = mc.soup(F, seed=4)
    small, _ = _surface(sv[None], sfaces, [target], None, 0.0, 1.0)
    _check_call("long/verts", small, sv[None], sfaces, [target], None, 0.0, 1.0)
    bfaces = mc.ribbon(Q, seed=3)[1]
    big, _ = _surface(np.tile(sv, (reps, 1))[:Q][None], bfaces, [target], None, 0.0, 1.0)
    for k in ("vert_face", "vert_bary", "vert_residual"):
        want = np.tile(small[k][0], (reps,) + (1,) * (small[k][0].ndim - 1))[:Q]
        assert np.array_equal(_bits(big[k][0]), _bits(want)), k
    # points against a fitted ribbon of F triangles
    fv, ffaces = mc.ribbon(F + 2, seed=5)
    pts = mc.points_near(fv, ffaces, 130, seed=6, sigma=0.05)
    small, _ = _surface(fv[None], ffaces, None, pts[None], 1.0, 0.0)
    _check_call("long/points", small, fv[None], ffaces, None, pts[None], 1.0, 0.0)
    big, _ = _surface(fv[None], ffaces, None, np.tile(pts, (reps, 1))[:Q][None], 1.0, 0.0, max_points=Q)
    for k in ("point_face", "point_bary", "point_residual"):
        want = np.tile(small[k][0], (reps,) + (1,) * (small[k][0].ndim - 1))[:Q]
        assert np.array_equal(_bits(big[k][0]), _bits(want)), k
    # the gather of Q points at the F + 2 vertices: against float64 sums of the returned correspondences
    want = np.zeros((F + 2, 3))
    r = big["point_residual"][0].astype(np.float64)
    corners = ffaces[big["point_face"][0]]
    for i in range(3):
        np.add.at(want, corners[:, i], -2.0 / Q * big["point_bary"][0][:, i:i + 1].astype(np.float64) * r)
    # (hundreds of contributions a vertex: the bound of a float32 sum of n terms in any order, n 2^-24 x the sum of magnitudes)
    mag = np.zeros((F + 2, 3))
    count = np.zeros(F + 2)
    for i in range(3):
        np.add.at(mag, corners[:, i], np.abs(2.0 / Q * big["point_bary"][0][:, i:i + 1].astype(np.float64) * r))
        np.add.at(count, corners[:, i], 1)
    assert (np.abs(big["dverts"][0] - want) <= (count + 2)[:, None] * 2.0 ** -24 * mag + 1e-30).all()


RAGGED_FACES = (1, 513, 7)


def _ragged():
    V, S = 130, 70
    fit = np.stack([mc.ribbon(V, seed=40 + n)[0] for n in range(3)])
    faces = mc.ribbon(V, seed=0)[1]
    targets = [mc.soup(F, seed=50 + n) for n, F in enumerate(RAGGED_FACES)]
    pts = np.stack([mc.points_near(targets[n][0], targets[n][1], S, seed=60 + n, sigma=0.05) for n in range(3)])
    return fit, faces, targets, pts


def test_ragged_batch():
    fit, faces, targets, pts = _ragged()
    assert len({len(t[0]) for t in targets}) == 3
    o, _ = _surface(fit, faces, targets, pts, 1.0, 1.0)
    _check_call("ragged", o, fit, faces, targets, pts, 1.0, 1.0)
    # mesh n of the batch is its one-mesh call bit for bit, although that call slices the scan differently
    for n in range(3):
        one, _ = _surface(fit[n:n + 1], faces, targets[n:n + 1], pts[n:n + 1], 1.0, 1.0)
        for k in ("point_face", "point_bary", "point_residual", "vert_face", "vert_bary", "vert_residual", "rows"):
            assert np.array_equal(_bits(o[k][n]), _bits(one[k][0])), (n, k)
    # (the gradient carries 1 / N: the assembly check above has judged every mesh of the batch against its own correspondences)


# ---- the whole gradient ------------------------------------------------------------------------------------------------------
def _record(key, value):
    path = os.environ.get("SMALFIT_WRITE_SURFACE_TERM_MEASURED")
    if path:
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc[key] = value
        json.dump(doc, open(path, "w"), indent=1, sort_keys=True)
    return bool(path)


def _judge(key, device, yardstick):
    """print, record and judge one deviation: 4 x the yardstick's on the same inputs, 3 x the device's own recorded one"""
    rec = json.load(open(MEASURED)) if os.path.exists(MEASURED) else {}
    bar = sc.WHOLE_GRADIENT_FACTOR * yardstick
    print("%-28s device %.3e   float32 yardstick %.3e   bar %.3e   recorded %s" % (key, device, yardstick, bar, rec.get("device/" + key)))
    recording = _record("device/" + key, device)
    _record("yardstick/" + key, yardstick)
    assert np.isfinite(device) and device <= bar, (key, device, bar)
    if recording:
        return
    assert "device/" + key in rec, "tests/golden/hip_surface_term_measured.json has no device/%s: run this file with " \
        "SMALFIT_WRITE_SURFACE_TERM_MEASURED=<path> on a GPU box and commit the result" % key
    assert device <= sc.WHOLE_GRADIENT_RATCHET * rec["device/" + key], (key, device, rec["device/" + key])


def test_whole_gradient_against_central_differences():
    V, F, S = 130, 60, 130
    fit, faces, targets, pts = _problem(F, S, seed=77, V=V)
    w_ps, w_vs = 1.0, 1.0
    o, _ = _surface(fit, faces, targets, pts, w_ps, w_vs, correspondences=False)
    t64 = [(t[0].astype(np.float64), t[1]) for t in targets]
    y = sc.term(fit, faces, targets, pts, w_ps, w_vs, dtype=np.float32)
    dev = yard = 0.0
    for i, u in enumerate(sc.smooth_directions(fit[0], 3, seed=5)):
        want = sc.central_difference(fit.astype(np.float64), faces, t64, pts.astype(np.float64), w_ps, w_vs, u[None])
        got = float((o["dverts"].astype(np.float64) * u[None]).sum())
        y32 = float((y["dverts"].astype(np.float64) * u[None]).sum())
        print("direction %d: device %.9e  yardstick %.9e  central difference %.9e" % (i, got, y32, want))
        dev, yard = max(dev, abs(got - want)), max(yard, abs(y32 - want))
    _judge("whole_gradient", dev, yard)


# ---- exact statements --------------------------------------------------------------------------------------------------------
def test_a_mesh_against_itself_is_exactly_zero():
    rv, rf = mc.ribbon(130, seed=8)
    cv = np.concatenate([mc.CUBE_VERTS * np.float32(0.37) + np.float32(0.11), rv[:122]])
    cf = np.concatenate([mc.CUBE_FACES, mc.ribbon(122, seed=8)[1] + 8]).astype(np.int32)
    for v, f in ((rv, rf), (cv, cf)):
        o, _ = _surface(v[None], f, [(v, f)], v[None], 1.0, 1.0)
        assert (o["losses"] == 0.0).all() and (o["rows"] == 0.0).all()
        assert (o["dverts"] == 0.0).all() and (o["dtrans"] == 0.0).all()
        assert (o["vert_residual"] == 0.0).all() and (o["point_residual"] == 0.0).all()


def test_cube_against_shifted_copies_in_closed_form():
    N = len(mc.CUBE_SHIFTS)
    fit = np.repeat(mc.CUBE_VERTS[None], N, 0)
    targets = [(mc.CUBE_VERTS + s, mc.CUBE_FACES) for s in mc.CUBE_SHIFTS]
    pts = np.stack([t[0] for t in targets])                           # the targets' corners lie on the targets
    o, _ = _surface(fit, mc.CUBE_FACES, targets, pts, 1.0, 1.0, max_points=8)
    for n, s in enumerate(mc.CUBE_SHIFTS):
        L_ulp = mc.ulp_l(fit[n], targets[n][0])
        dv = np.linalg.norm(o["vert_residual"][n].astype(np.float64), axis=1)
        dp = np.linalg.norm(o["point_residual"][n].astype(np.float64), axis=1)
        assert np.abs(dv - mc.box_surface_dist(mc.CUBE_VERTS, s, s + 1.0)).max() <= sc.DELTA_ULP * L_ulp
        assert np.abs(dp - mc.box_surface_dist(targets[n][0], np.zeros(3), np.ones(3))).max() <= sc.DELTA_ULP * L_ulp
    # corner (1,1,0) lies inside the first copy, an eighth above its bottom face: the residual is that eighth along z, exactly
    assert np.array_equal(o["vert_residual"][0][6], np.array([0, 0, 0.125], np.float32))
    # vertices only, one mesh, far outside along one axis: every vertex is pulled along the shift, the sum is d trans
    far = np.array([4.0, 0.0, 0.0], np.float32)
    o, _ = _surface(mc.CUBE_VERTS[None], mc.CUBE_FACES, [(mc.CUBE_VERTS + far, mc.CUBE_FACES)], None, 0.0, 4.0, max_points=8)
    g = o["dverts"][0]
    near = mc.CUBE_VERTS[:, 0] == 1
    assert np.array_equal(g[near], np.tile(np.array([-3.0, 0, 0], np.float32), (4, 1)))       # 2 w / (N V) r = r, r = (-3, 0, 0)
    assert np.array_equal(g[~near], np.tile(np.array([-4.0, 0, 0], np.float32), (4, 1)))
    assert np.array_equal(o["dtrans"][0], np.array([-28.0, 0, 0], np.float32))
    assert o["losses"][1] == np.float32((4 * 9 + 4 * 16) / 8.0) and o["losses"][0] == 0.0 and o["losses"][2] == 4 * o["losses"][1]


def _two_mesh_problem():
    V = 130
    fit = np.stack([mc.ribbon(V, seed=20 + n)[0] for n in range(2)])
    faces = mc.ribbon(V, seed=0)[1]
    targets = [mc.soup(40 + n, seed=30 + n) for n in range(2)]
    return fit, faces, targets


def test_two_calls_the_same_bits_and_nothing_survives_a_larger_call():
    fit, faces, targets = _two_mesh_problem()
    big = np.stack([mc.points_near(*targets[n], 130, seed=80 + n) for n in range(2)])
    small = np.stack([mc.points_near(*targets[n], 70, seed=90 + n) for n in range(2)])
    a, used = _surface(fit, faces, targets, big)
    b, _ = _surface(fit, faces, targets, big, objective=used)
    _same_bits(a, b, "two calls")
    after, _ = _surface(fit, faces, targets, small, objective=used)
    fresh, _ = _surface(fit, faces, targets, small)
    _same_bits(after, fresh, "a smaller call after a larger")
    one_after, _ = _surface(fit[:1], faces, targets[:1], small[:1], objective=used)
    one_fresh, _ = _surface(fit[:1], faces, targets[:1], small[:1])
    _same_bits(one_after, one_fresh, "fewer meshes after more")


def test_one_direction_only():
    fit, faces, targets = _two_mesh_problem()
    pts = np.stack([mc.points_near(*targets[n], 65, seed=95 + n) for n in range(2)])
    both, obj = _surface(fit, faces, targets, pts, 1.0, 1.0)
    ps, _ = _surface(fit, faces, None, pts, 1.0, 0.0, objective=obj)
    vs, _ = _surface(fit, faces, targets, None, 0.0, 1.0, objective=obj)
    vs2, _ = _surface(fit, faces, targets, pts, -1.0, 1.0, objective=obj)
    assert "vert_face" not in ps and "point_face" not in vs
    for k in ("point_face", "point_bary", "point_residual"):
        assert np.array_equal(_bits(ps[k]), _bits(both[k])), k
    for k in ("vert_face", "vert_bary", "vert_residual"):
        assert np.array_equal(_bits(vs[k]), _bits(both[k])) and np.array_equal(_bits(vs2[k]), _bits(both[k])), k
    assert ps["losses"][0] == both["losses"][0] and ps["losses"][1] == 0.0 and ps["losses"][2] == ps["losses"][0]
    assert vs["losses"][1] == both["losses"][1] and vs["losses"][0] == 0.0 and (vs["rows"][:, 0] == 0).all()
    assert np.array_equal(_bits(vs["dverts"]), _bits(vs2["dverts"]))
    # the two one-direction gradients add up to the whole (one rounding per coordinate)
    total = ps["dverts"].astype(np.float64) + vs["dverts"]
    assert np.abs(both["dverts"] - total).max() <= 2 * ULP * np.abs(total).max()
    off, _ = _surface(fit, faces, None, None, 0.0, 0.0, objective=obj)
    assert (off["losses"] == 0).all() and (off["dverts"] == 0).all() and (off["dtrans"] == 0).all() and (off["rows"] == 0).all()


def test_refusals_leave_the_outputs_alone():
    fit, faces, targets = _two_mesh_problem()
    N, V, S = 2, fit.shape[1], 70
    obj = eng.MeshObjective(V, faces, sc.MAX_MESHES, sc.MAX_POINTS)
    tg = eng.MeshTargets([t[0] for t in targets], [t[1] for t in targets])
    tg1 = eng.MeshTargets([targets[0][0]], [targets[0][1]])
    verts, pts = _t(fit), _t(np.stack([mc.points_near(*targets[n], S, seed=n) for n in range(N)]))
    with pytest.raises(eng.SmalfitError, match="1 <= num_points <= max_points points"):
        obj.surface(verts, tg, _t(np.zeros((N, sc.MAX_POINTS + 1, 3))), 1.0, 1.0)
    with pytest.raises(eng.SmalfitError, match="number of target meshes differs"):
        obj.surface(verts, tg1, pts, 1.0, 1.0)
    with pytest.raises(eng.SmalfitError, match="needs the target meshes"):
        obj.surface(verts, None, pts, 1.0, 1.0)
    lib = _lib.load()
    fn = _lib.resolve(lib, "smalfit_mesh_surface_eval")
    f32 = dict(losses=(3,), rows=(N, 2), dverts=(N, V, 3), dtrans=(N, 3), point_bary=(N, S, 3), vert_bary=(N, V, 3),
               point_residual=(N, S, 3), vert_residual=(N, V, 3))
    out = {k: torch.full(s, -7.0, device=DEV) for k, s in f32.items()}
    out["point_face"] = torch.full((N, S), -7, dtype=torch.int32, device=DEV)
    out["vert_face"] = torch.full((N, V), -7, dtype=torch.int32, device=DEV)

    def block():
        a = sc.valid_args(N=N, S=S)
        a.verts, a.points = verts.data_ptr(), pts.data_ptr()
        for k, v in out.items():
            setattr(a, k, v.data_ptr())
        return a
    tried = 0
    for name, step, change, changed, text in sc.REFUSALS:
        if step:
            continue
        a = block()
        change(a)
        t = tg
        if changed.get("targets") is False:
            t = None
        elif changed.get("target_meshes") == 1:
            t = tg1
        elif "target_meshes" in changed:
            continue                                   # (num_meshes above THIS objective's capacity is refused before the targets are read)
        assert fn(obj.handle, t.handle if t else None, eng._stream(), C.byref(a)) != 0, name
        assert lib.smalfit_last_error().decode() == "smalfit_mesh_surface_eval: " + text, name
        tried += 1
    assert tried >= 12
    a = block()
    a.num_meshes = sc.MAX_MESHES + 1
    assert fn(obj.handle, tg.handle, eng._stream(), C.byref(a)) != 0 and b"max_meshes" in lib.smalfit_last_error()
    assert fn(None, tg.handle, eng._stream(), C.byref(block())) != 0 and b"null argument" in lib.smalfit_last_error()
    assert fn(obj.handle, tg.handle, eng._stream(), None) != 0 and b"null argument" in lib.smalfit_last_error()
    torch.cuda.synchronize()
    for k, v in out.items():
        assert (v == -7).all(), k
    assert fn(obj.handle, tg.handle, eng._stream(), C.byref(block())) == 0
    torch.cuda.synchronize()
    for k, v in out.items():
        assert not (v == -7).any(), k


# ---- the step ----------------------------------------------------------------------------------------------------------------
_PARAMS = ("betas", "global_rot", "joint_rot", "trans", "deform_verts")


def _three_steps(how):
    """three iterations of the default scheme through one of the three spellings of 'no surface term'"""
    from smalify_amd.fitter_3d import Stage
    md, fit, targets = m3.fitter_problem(2, seed=6)
    stage = Stage(3, "default", fit, targets, lr=0.02, custom_lrs=m3.DEFAULT_CUSTOM_LRS, seed=11)
    e = fit._engine()
    fn = _lib.resolve(e.lib, "smalfit_fit3d_step_surface")
    sf_losses = torch.full((3,), -7.0, device=DEV)
    losses = []
    for it in range(3):
        a = stage._step_args()
        for name in ("betas", "log_beta_scales") + _PARAMS[1:]:
            setattr(a, name, getattr(fit, name).data_ptr())
        a.weights = (C.c_float * 4)(*stage._weights())
        a.iteration, a.adam_t = it, it + 1
        tg = stage.target_meshes._dev.handle
        if how == "step":
            rc = e.lib.smalfit_fit3d_step(e.handle, stage._objective.handle, tg, eng._stream(), C.byref(a))
        elif how == "null":
            rc = fn(e.handle, stage._objective.handle, tg, eng._stream(), C.byref(a), None)
        else:
            sf = _lib.SurfaceTermArgs()
            sf.num_meshes, sf.w_point_surface, sf.w_vert_surface, sf.losses = 2, 0.0, 0.0 if how == "zero" else -1.0, sf_losses.data_ptr()
            rc = fn(e.handle, stage._objective.handle, tg, eng._stream(), C.byref(a), C.byref(sf))
        assert rc == 0, e.lib.smalfit_last_error()
        losses.append(stage._buffers["losses"].clone())
    torch.cuda.synchronize()
    assert (sf_losses == -7).all()                       # a block with both weights <= 0 is not written either
    state = {k: getattr(fit, k).detach().cpu().numpy().copy() for k in _PARAMS}
    for k, st in stage._adam.items():
        state["m_" + k], state["v_" + k] = st["m"].cpu().numpy().copy(), st["v"].cpu().numpy().copy()
    state["losses"] = torch.stack(losses).cpu().numpy()
    state["points"] = stage._points.cpu().numpy().copy()
    return state


def test_the_step_without_the_term_is_the_step_of_before():
    base = _three_steps("step")
    assert np.abs(base["m_trans"]).max() > 0 and np.isfinite(base["losses"]).all()
    for how in ("null", "zero", "negative"):
        _same_bits(base, _three_steps(how), how)


def _surface_runs(weights, iters=5, scheme="default"):
    from smalify_amd.fitter_3d import Stage
    results = []
    for fused in (True, False):
        md, fit, targets = m3.fitter_problem(2, seed=6)
        stage = Stage(iters, scheme, fit, targets, loss_weights=weights, lr=0.02, custom_lrs=m3.DEFAULT_CUSTOM_LRS, seed=11)
        losses, terms = [], []
        for it in range(iters):
            losses.append((stage.step(it) if fused else stage.step_unfused(it)).clone())
            terms.append(stage.last_surface_terms.clone())
        torch.cuda.synchronize()
        assert stage.last_terms.shape == (5,) and stage.last_surface_terms.shape == (3,)
        results.append((torch.stack(losses).cpu().numpy(), torch.stack(terms).cpu().numpy(),
                        {k: getattr(fit, k).detach().cpu().numpy().copy() for k in _PARAMS}, stage.last_points.cpu().numpy().copy()))
    return results


def test_fused_and_unfused_steps_agree_with_the_term_on():
    (la, ta, pa, xa), (lb, tb, pb, xb) = _surface_runs({"w_point_surface": 2.0, "w_vert_surface": 1.5})
    assert np.array_equal(xa, xb)
    print("fused %s\nunfused %s\nsurface terms %s" % (la, lb, ta[-1]))
    assert (ta[:, 2] > 0).all() and np.abs(ta - tb).max() <= 1e-6 * np.abs(tb).max()
    assert np.abs(la - lb).max() <= 1e-6 * np.abs(lb).max()                 # the bar of the fused-versus-unfused fit3d test
    for k in pa:
        assert m3.rel(pa[k], pb[k]) < 1e-6 or np.array_equal(pa[k], pb[k]), k


def test_chamfer_off_point_surface_on_samples_points_and_trains():
    from smalify_amd.fitter_3d import Stage
    md, fit, targets = m3.fitter_problem(2, seed=6)
    w = dict(w_chamfer=0.0, w_edge=0.0, w_normal=0.0, w_laplacian=0.0, w_point_surface=1.0)
    stage = Stage(12, "init", fit, targets, loss_weights=w, lr=0.02, seed=3)
    stage._sample_buffer().fill_(float("nan"))
    history = [float(stage.step(it)) for it in range(12)]
    pts = stage.last_points.cpu().numpy()
    assert np.isfinite(pts).all() and np.abs(pts).max() <= 1.0 + 1e-6                  # sampled this iteration, on the targets
    want = targets._dev.sample(3000, 3, 11).cpu().numpy()
    assert np.array_equal(pts, want)
    assert float(stage.last_terms[4]) == 0.0 and float(stage.last_terms[0]) == 0.0     # the four terms are off, the total is the term's
    print("point-surface only: %s" % history)
    assert np.isfinite(history).all() and history[-1] < history[0]
    assert float(fit.trans.detach().abs().max()) > 0


def test_deform_scheme_descends_on_the_surface_term_alone():
    """the step's own Adam on deform_verts with nothing but the surface term to descend on"""
    from smalify_amd.fitter_3d import Stage
    md, fit, targets = m3.fitter_problem(2, seed=6)
    w = dict(w_chamfer=0.0, w_edge=0.0, w_normal=0.0, w_laplacian=0.0, w_point_surface=1.0, w_vert_surface=1.0)
    stage = Stage(30, "deform", fit, targets, loss_weights=w, lr=0.002, seed=3)
    before = {k: getattr(fit, k).detach().clone() for k in _PARAMS}
    history, terms = [], []
    for it in range(30):
        history.append(stage.step(it).clone())
        terms.append(stage.last_surface_terms.clone())
    torch.cuda.synchronize()
    history, terms = torch.stack(history).cpu().numpy(), torch.stack(terms).cpu().numpy()
    print("deform only, surface term only: %s" % history)
    assert np.array_equal(history, terms[:, 2])                                    # the four terms are off: the total is the term
    assert np.isfinite(history).all() and history[-1] < history[0]
    assert terms[-1, 0] < terms[0, 0] and terms[-1, 1] < terms[0, 1]                # both directions
    assert float((fit.deform_verts.detach() - before["deform_verts"]).abs().max()) > 0
    for k in ("betas", "global_rot", "joint_rot", "trans"):
        assert torch.equal(getattr(fit, k).detach(), before[k]), k                  # only deform_verts is trained


# ---- descent: the cube towards its shifted copy, vertices only --------------------------------------------------------------
def _numpy_descent(dtype, lr, steps, fit0, faces, targets, pts):
    v = fit0.astype(dtype).copy()
    m, s = np.zeros_like(v), np.zeros_like(v)
    b1, b2, eps = dtype(0.9), dtype(0.999), dtype(1e-8)
    terms = []
    for t in range(1, steps + 1):
        o = sc.term(v, faces, [(targets[0][0].astype(dtype), targets[0][1])], pts.astype(dtype), 1.0, 1.0, dtype=dtype)
        terms.append(float(o["term"]))
        g = o["dverts"]
        m = b1 * m + (dtype(1) - b1) * g
        s = b2 * s + (dtype(1) - b2) * g * g
        step = dtype(lr) / dtype(1 - 0.9 ** t)
        v = v - step * m / (np.sqrt(s) / dtype(np.sqrt(1 - 0.999 ** t)) + eps)
    return np.array(terms)


def test_descent_follows_the_float64_loop():
    steps = 30
    fit0 = mc.CUBE_VERTS[None].copy()
    targets = [(mc.CUBE_VERTS + mc.CUBE_SHIFT, mc.CUBE_FACES)]
    pts = mc.points_near(targets[0][0], targets[0][1], 64, seed=4, sigma=0.0)[None]
    lr = next((c for c in (0.05, 0.02, 0.01, 0.005) if (np.diff(_numpy_descent(np.float64, c, steps, fit0, mc.CUBE_FACES, targets, pts)) < 0).all()), None)
    assert lr is not None, "no candidate learning rate makes the float64 loop decrease"
    t64 = _numpy_descent(np.float64, lr, steps, fit0, mc.CUBE_FACES, targets, pts)
    t32 = _numpy_descent(np.float32, lr, steps, fit0, mc.CUBE_FACES, targets, pts)
    obj = eng.MeshObjective(8, mc.CUBE_FACES, 1, 64)
    tg = eng.MeshTargets([targets[0][0]], [targets[0][1]])
    v, dp = _t(fit0), _t(pts)
    m, s = torch.zeros_like(v), torch.zeros_like(v)
    got = []
    for t in range(1, steps + 1):
        o = obj.surface(v, tg, dp, 1.0, 1.0)
        got.append(o["losses"][2].clone())
        eng.adam_step(v, o["dverts"], m, s, lr, t, beta1=0.9, beta2=0.999, eps=1e-8)
    torch.cuda.synchronize()
    got = torch.stack(got).cpu().numpy().astype(np.float64)
    print("lr %g\nfloat64 %s\ndevice  %s" % (lr, t64, got))
    _judge("descent", float(np.abs(got - t64).max()), float(np.abs(t32 - t64).max()))
    assert got[-1] < got[0]


# ---- front end -------------------------------------------------------------------------------------------------------------
def test_stage_takes_the_surface_weights():
    from smalify_amd.fitter_3d import Stage
    md, fit, targets = m3.fitter_problem(2, seed=6)
    stage = Stage(4, "init", fit, targets, loss_weights={"w_point_surface": 1.0}, lr=0.05, seed=2)
    assert stage.surface_weights == dict(w_point_surface=1.0, w_vert_surface=0.0) and stage.surface_on
    assert sorted(stage.loss_weights) == ["w_chamfer", "w_edge", "w_laplacian", "w_normal"]
    total = stage.step(0)
    torch.cuda.synchronize()
    terms, sterms = stage.last_terms.cpu().numpy(), stage.last_surface_terms.cpu().numpy()
    assert sterms[0] > 0 and sterms[1] == 0 and sterms[2] == sterms[0]
    assert float(total) == np.float32(terms[4] + sterms[2])                # the grand total: the four terms + the surface term
    assert float(stage.step_unfused(1)) == float(np.float32(stage.last_terms.cpu().numpy()[4] + stage.last_surface_terms.cpu().numpy()[2]))
    stage.run(progress=False)
    assert len(stage.losses_to_plot) == 4 and np.isfinite(stage.losses_to_plot).all()
    plain = Stage(1, "init", fit, targets, lr=0.05, seed=2)
    plain.step(0)
    assert plain.last_surface_terms is None and not plain.surface_on


def test_optimise_main_takes_the_surface_weights_from_yaml(tmp_path):
    from smalify_amd.fitter_3d import optimise
    md = m3.synthetic.synthetic_model(seed=0, shape_family_id=-1)
    tv, tf = m3.target_meshes_from_smal(md, 2, seed=9)
    mesh_dir = tmp_path / "meshes"
    mesh_dir.mkdir()
    for name, v in zip(("m0", "m1"), tv):
        with open(mesh_dir / (name + ".obj"), "w") as fh:
            for p in v * 3.0 + 0.5:
                fh.write("v %.7f %.7f %.7f\n" % tuple(p))
            for f in tf:
                fh.write("f %d %d %d\n" % tuple(f + 1))
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("stages:\n  Stage0:\n    scheme: 'init'\n    nits: 15\n    lr: 0.05\n"
                   "    loss_weights:\n      w_point_surface: 1.0\n      w_vert_surface: 0.5\n      w_edge: 0.8\n"
                   "args:\n  results_dir: %s\n  shape_family_id: -1\n" % (tmp_path / "out"))
    args = optimise.build_parser().parse_args(["--mesh_dir", str(mesh_dir), "--yaml_src", str(cfg), "--no_plots"])
    mgr = optimise.main(args, model_data=md, smal_data=m3.synthetic_smal_data())
    st = mgr.stages[0]
    assert st.surface_weights == dict(w_point_surface=1.0, w_vert_surface=0.5) and st.loss_weights["w_edge"] == 0.8
    s = st.last_surface_terms.cpu().numpy()
    assert (s > 0).all() and abs(s[2] - (s[0] + 0.5 * s[1])) <= 4 * ULP * s[2]
    h = st.losses_to_plot
    assert len(h) == 15 and np.isfinite(h).all() and h[-1] < h[0]
    z = np.load(tmp_path / "out" / "Stage0.npz", allow_pickle=True)
    assert np.isfinite(z["verts"]).all()
