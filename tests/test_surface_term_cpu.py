"""The point-to-surface term without a device: mesh3d_math.h's point_scan_tri_closest and the nearest-face scan through the host
shim (tests/host_surface_term_shim.cpp, built without contraction), the float64 oracle of tests/surface_term_cases.py, and
smalfit_plan.h's rules, struct layout, slice count and choice of points.  Every figure is printed before it is judged."""
import ctypes as C

import numpy as np
import pytest

from smalify_amd import _lib
from tests import host_surface_term as hs
from tests import mesh_score_cases as mc
from tests import surface_term_cases as sc

ULP = 2.0 ** -23


# ---- the new function of mesh3d_math.h ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pairs():
    p, a, b, c = mc.accuracy_pairs()
    return (p, a, b, c), hs.closest(p, a, b, c)


def test_d2_is_point_scan_tri_dist2_bit_for_bit(pairs):
    _, o = pairs
    assert np.array_equal(o["d2"].view(np.int32), o["dist2"].view(np.int32))


def test_barycentrics_are_weights(pairs):
    _, o = pairs
    total = o["bary"].astype(np.float64).sum(1)
    print("least weight %g, sum off 1 by at most %.2f ulp" % (o["bary"].min(), np.abs(total - 1.0).max() / ULP))
    assert (o["bary"] >= 0.0).all()
    assert np.abs(total - 1.0).max() <= 4 * ULP


def test_residual_and_barycentrics_name_one_point(pairs):
    """p - r and sum b_i corner_i are the same point up to the rounding of coordinates of size L, and |r|^2 is d^2.
    The quantile, not the maximum: where a sliver's plane wins, its weights s_i / sum are quotients of cancelled cross products,
    relative error ulp / sin(angle) with no bound over all slivers, so the barycentric point has a tail the residual -- formed
    from d - t e or (h / |n|^2) n, and the only one of the two the gradient uses -- does not have.  The residual's own error is
    held to the distance bar without exception (|r| against d below, the stand-in and the device tests against float64)"""
    (p, a, b, c), o = pairs
    q_r = p.astype(np.float64) - o["r"]
    q_b = (o["bary"].astype(np.float64)[:, :, None] * np.stack([a, b, c], 1)).sum(1)
    gap = np.abs(q_r - q_b).max(1) / mc.pair_ulp(p, a, b, c)
    # two float32 roads to one point: all but the slivers' tail within a few ulp(L), the tail within the distance bar
    print("p - r against the barycentric point: worst %.1f ulp(L), 99.9 %% within %.1f" % (gap.max(), np.quantile(gap, 0.999)))
    assert np.quantile(gap, 0.999) <= sc.DELTA_ULP
    r2 = (o["r"].astype(np.float64) ** 2).sum(1)
    assert np.abs(np.sqrt(r2) - np.sqrt(o["d2"].astype(np.float64))).max() <= 4 * mc.pair_ulp(p, a, b, c).max()


def test_the_oracle_agrees_with_another_closest_point(pairs):
    """the float64 oracle shares its candidates and their order with the library; the closest point by Voronoi region is another
    road to the same q.  Distances agree to float64 rounding everywhere; the points wherever the triangle is not so thin that
    float64 itself cannot place a point along it (|n|^2 above 1e-12 of the squared edges)"""
    (p, a, b, c), _ = pairs
    sel = slice(0, 200_000)
    p, a, b, c = (x[sel].astype(np.float64) for x in (p, a, b, c))
    o = sc.closest(p, a, b, c)
    q = sc.region_walk_closest(p, a, b, c)
    dd = np.abs(np.linalg.norm(p - q, axis=1) - np.sqrt(o["d2"]))
    n = np.cross(b - a, c - a)
    edges = np.maximum.reduce([((x - y) ** 2).sum(1) for x, y in ((a, b), (b, c), (c, a))])
    fat = (n * n).sum(1) > 1e-12 * edges * edges
    gap = np.linalg.norm(q - o["q"], axis=1)
    print("oracle against the region walk: distance %.2e, q %.2e over %d of %d pairs" % (dd.max(), gap[fat].max(), fat.sum(), len(fat)))
    # float64 rounding, 2e-16 of coordinates of size 2: nothing amplifies it in a distance; along a triangle whose sine is at
    # least 1e-6 (the `fat` ones) it is amplified by at most 1e6
    assert dd.max() <= 1e-12
    assert fat.mean() > 0.99 and gap[fat].max() <= 1e-9
    b64 = (o["bary"][:, :, None] * np.stack([a, b, c], 1)).sum(1)
    assert np.linalg.norm(b64 - o["q"], axis=1)[fat].max() <= 1e-9                 # the oracle's barycentrics name its q


@pytest.mark.parametrize("order", sc.CORNER_ORDERS)
def test_unit_triangle_regions_in_every_corner_order(order):
    names, q, want = sc.region_queries()
    tri = mc.UNIT_TRIANGLE[list(order)]
    o = hs.closest(q, *(np.repeat(tri[i][None], len(q), 0) for i in range(3)))
    got_r = q.astype(np.float64) - o["r"]
    got_b = (o["bary"].astype(np.float64)[:, :, None] * tri[None].astype(np.float64)).sum(1)
    for i, name in enumerate(names):
        assert np.abs(got_r[i] - want[i]).max() <= 2 * ULP, (name, order, got_r[i], want[i])
        assert np.abs(got_b[i] - want[i]).max() <= 2 * ULP, (name, order, got_b[i], want[i])
    assert np.abs(np.sqrt(o["d2"].astype(np.float64)) - np.linalg.norm(q - want, axis=1)).max() <= 4 * ULP * 2.5


@pytest.mark.parametrize("name,tri,seg", mc.DEGENERATE)
def test_degenerate_triangles_are_their_segment(name, tri, seg):
    q = np.array(mc.DEGENERATE_QUERIES, np.float32)
    tri = np.array(tri, np.float32)
    o = hs.closest(q, *(np.repeat(tri[i][None], len(q), 0) for i in range(3)))
    s0, s1 = (np.array(x, np.float64) for x in seg)
    ev = s1 - s0
    l2 = (ev * ev).sum()
    t = np.clip(((q - s0) * ev).sum(1) / l2, 0, 1) if l2 > 0 else np.zeros(len(q))
    want = s0 + t[:, None] * ev
    got_r = q.astype(np.float64) - o["r"]
    got_b = (o["bary"].astype(np.float64)[:, :, None] * tri[None].astype(np.float64)).sum(1)
    assert np.abs(got_r - want).max() <= 8 * ULP * 3, name
    assert np.abs(got_b - want).max() <= 8 * ULP * 3, name
    assert (o["bary"] >= 0).all() and np.abs(o["bary"].sum(1) - 1).max() <= 4 * ULP


def test_points_on_the_triangle_have_no_residual():
    q = np.array(mc.UNIT_ZEROS, np.float32)
    for order in sc.CORNER_ORDERS:
        tri = mc.UNIT_TRIANGLE[list(order)]
        o = hs.closest(q, *(np.repeat(tri[i][None], len(q), 0) for i in range(3)))
        assert (o["r"] == 0.0).all() and (o["d2"] == 0.0).all(), order
        got = (o["bary"].astype(np.float64)[:, :, None] * tri[None]).sum(1)
        assert np.abs(got - q).max() <= ULP, order


# ---- the float64 oracle's gradient ---------------------------------------------------------------------------------------------
def _generic_problem(seed=3):
    V = 40
    fit, faces = mc.ribbon(V, seed=seed)
    fit = fit.astype(np.float64)[None] + 0.01 * np.random.RandomState(seed).randn(1, V, 3)
    tv, tf = mc.soup(30, seed=seed + 1)
    pts = mc.points_near(tv, tf, 50, seed=seed + 2, sigma=0.05).astype(np.float64)[None]
    return fit, faces, [(tv.astype(np.float64), tf)], pts


@pytest.mark.parametrize("w_ps,w_vs", ((1.0, 0.0), (0.0, 1.0), (0.7, 1.3)))
def test_oracle_gradient_against_central_differences(w_ps, w_vs):
    fit, faces, targets, pts = _generic_problem()
    o = sc.term(fit, faces, targets, pts, w_ps, w_vs)
    rs = np.random.RandomState(9)
    for _ in range(4):
        u = rs.randn(*fit.shape)
        want = sc.central_difference(fit, faces, targets, pts, w_ps, w_vs, u)
        got = (o["dverts"] * u).sum()
        print("w %.1f %.1f: <g, u> %.9e   central difference %.9e   rel %.2e" % (w_ps, w_vs, got, want, abs(got - want) / abs(want)))
        assert abs(got - want) <= 1e-6 * abs(want)
    assert np.allclose(o["dtrans"], o["dverts"].sum(1), rtol=0, atol=1e-15)


def test_oracle_gradient_does_not_depend_on_which_incident_face_wins():
    # two triangles sharing the edge (0, 1), folded upwards; a third sharing only vertex 0.  Dyadic coordinates: the tied
    # distances are equal to the bit in float64 too
    v = np.array([[0, 0, 0], [1, 0, 0], [0.25, 1, 0.5], [0.5, -1, 0.5], [-1, -0.5, 1], [-1, 0.5, 1]], np.float64)[None]
    f = np.array([[0, 1, 2], [1, 0, 3], [0, 4, 5]], np.int64)
    edge_point = np.array([[[0.5, 0.0, -0.75]]])          # below the middle of the shared edge
    vertex_point = np.array([[[-0.25, 0.0, -0.5]]])       # nearest to the shared vertex 0 on all three
    for pts in (edge_point, vertex_point):
        grads, winners = [], []
        for perm in ((0, 1, 2), (1, 0, 2), (2, 1, 0), (2, 0, 1)):
            o = sc.term(v, f[list(perm)], None, pts, 1.0, 0.0)
            grads.append(o["dverts"])
            winners.append(perm[int(o["point"][0]["face"][0])])
        assert len(set(winners)) > 1, winners                       # the tie is real: another face wins in another order
        for g in grads[1:]:
            assert np.abs(g - grads[0]).max() <= 1e-15
        assert np.abs(grads[0]).max() > 0.1


# ---- the conditioning rule on the stand-in mesh ----------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", sc.STANDIN_NOISE)
def test_standin_queries_within_the_conditioning_rule(noise):
    v, f = sc.standin_mesh()
    q = sc.standin_queries(noise)
    L = float(np.abs(v).max())
    delta = sc.DELTA_ULP * ULP * L
    o64 = sc.nearest(q, v, f, delta=delta)
    flagged = o64["flagged"]
    print("noise %.3f L: float64 flags %d of %d queries" % (noise, flagged.sum(), len(q)))
    assert flagged.mean() <= sc.FLAG_CAP                               # the oracle first
    for slices in (1, hs.slices(len(q), len(f), 1)):
        got = hs.nearest(q, v, f, slices)
        d64 = np.sqrt(o64["d2"])
        dev = np.abs(np.sqrt(got["d2"].astype(np.float64)) - d64).max() / (ULP * L)
        own = np.abs(sc.face_dist(q, v, f, got["face"]) - d64).max() / (ULP * L)
        q_got = sc.point_from(v, f, got["face"], got["bary"])
        off = np.linalg.norm(q_got - o64["q"], axis=1)
        ok = off <= sc.reach(d64, delta)
        print("  %d slices: distance %.2f ulp(L), returned face's own %.2f ulp(L), q off by at most %.3g (unflagged), %d beyond reach"
              % (slices, dev, own, off[~flagged].max(), int((~ok & ~flagged).sum())))
        assert dev <= sc.DELTA_ULP and own <= sc.DELTA_ULP
        assert ok[~flagged].all()
        # the residual names the same point
        assert (np.linalg.norm(q.astype(np.float64) - got["r"] - q_got, axis=1) <= delta).all()
    one, many = hs.nearest(q, v, f, 1), hs.nearest(q, v, f, 7)
    for k in one:
        assert np.array_equal(one[k].view(np.int32), many[k].view(np.int32)), k          # the slices change no bit


def test_lowest_face_index_among_equal_distances():
    v, f = mc.CUBE_VERTS, mc.CUBE_FACES
    q = np.array([[0.5, 0.5, -0.25], [1.25, 1.25, 0.5], [0, 0, 0], [1.5, 1.5, 1.5]], np.float32)     # a diagonal, an edge, corners
    got = hs.nearest(q, v, f, 3)
    o64 = sc.nearest(q, v, f)
    assert np.array_equal(got["face"], o64["face"])
    d_all = mc.point_triangle_dist(q[:, None].astype(np.float64), *(v.astype(np.float64)[f[:, i]][None] for i in range(3)))
    assert ((d_all == d_all.min(1, keepdims=True)).sum(1) >= 2).all()                     # every query has a tie


def test_the_gather_is_the_scatter():
    rs = np.random.RandomState(5)
    V, S = 37, 300
    _, faces = mc.ribbon(V, seed=1)
    corners = faces[rs.randint(0, len(faces), S)]
    bary = rs.dirichlet((1, 1, 1), S).astype(np.float32)
    r = rs.randn(S, 3).astype(np.float32)
    got = hs.gather(V, corners, bary, r)
    want = np.zeros((V, 3))
    for i in range(3):
        np.add.at(want, corners[:, i], bary[:, i:i + 1].astype(np.float64) * r)
    count = np.bincount(corners.ravel(), minlength=V).max()
    assert np.abs(got - want).max() <= (count + 2) * ULP * np.abs(bary[:, :, None] * r[:, None, :]).max()


# ---- rules, struct, grids ----------------------------------------------------------------------------------------------------
def _refusal(step, change, changed):
    a = sc.valid_args(step=step)
    change(a)
    return hs.refusal(a, **sc.facts(**dict(dict(step=step), **changed)))


@pytest.mark.parametrize("name,step,change,changed,text", sc.REFUSALS)
def test_every_refusal_rule_with_its_text(name, step, change, changed, text):
    assert _refusal(step, change, changed) == text, name


@pytest.mark.parametrize("name,step,change,changed", sc.ACCEPTED)
def test_accepted_edges(name, step, change, changed):
    assert _refusal(step, change, changed) is None, name


def test_the_rules_apply_in_their_order():
    order = list(dict.fromkeys((r[1], r[4]) for r in sc.REFUSALS))
    for i, (name_i, step_i, change_i, facts_i, text_i) in enumerate(sc.REFUSALS):
        for name_j, step_j, change_j, facts_j, text_j in sc.REFUSALS[i + 1:]:
            if step_i != step_j or text_i == text_j or set(facts_i) & set(facts_j):
                continue
            a = sc.valid_args(step=step_i)
            change_i(a)
            change_j(a)
            got = hs.refusal(a, **sc.facts(**dict(dict(step=step_i), **facts_i, **facts_j)))
            if got != text_i:
                # (a later change may undo an earlier fault -- w_vert_surface = 0 lifts the need for targets; never the reverse)
                assert got == text_j or got is None, (name_i, name_j, got)
                assert order.index((step_i, text_i)) < order.index((step_j, text_j))
    # struct_size comes before everything
    a = sc.valid_args()
    a.struct_size, a.num_meshes, a.losses = 8, 0, None
    assert hs.refusal(a, **sc.facts()) == sc.SIZE_TEXT


def test_struct_layout_matches_the_header():
    lib = hs.load()
    assert lib.hst_sizeof_args() == C.sizeof(_lib.SurfaceTermArgs)
    assert hs.offsets() == [getattr(_lib.SurfaceTermArgs, f).offset for f, _ in _lib.SurfaceTermArgs._fields_]
    assert _lib.SurfaceTermArgs._fields_[0][0] == "struct_size" and _lib.SurfaceTermArgs().struct_size == C.sizeof(_lib.SurfaceTermArgs)
    assert lib.hst_sizeof_fit3d_args() == C.sizeof(_lib.Fit3dArgs)                        # the step's block did not grow
    assert lib.hst_sizeof_hit() == 48
    assert {"smalfit_mesh_surface_eval", "smalfit_fit3d_step_surface"} <= set(_lib.SIGNATURES) & set(_lib.LAZY_SYMBOLS)
    assert _lib.ABI_VERSION == 6


def test_both_weights_off_is_no_term():
    lib = hs.load()
    a = sc.valid_args()
    assert lib.hst_term_on(C.byref(a)) == 1
    a.w_point_surface, a.w_vert_surface = 0.0, -2.0
    assert lib.hst_term_on(C.byref(a)) == 0 and lib.hst_term_on(None) == 0
    a.w_vert_surface = 1e-3
    assert lib.hst_term_on(C.byref(a)) == 1


def test_slice_count_as_numbers():
    lib = hs.load()
    assert lib.hst_target_blocks() >= sc.CUS and lib.hst_min_slice() == 64 and lib.hst_surface_chunk() == mc.QUERIES * 8
    v, f = sc.standin_mesh()
    V, F, S = len(v), len(f), 3000
    for queries in (V, S):
        x, y, z = hs.near_grid(queries, F, 1)
        print("one stand-in mesh, %d queries: grid %d x %d x %d = %d blocks" % (queries, x, y, z, x * y * z))
        assert x == -(-queries // mc.QUERIES) and y == 1 and x * y * z >= sc.CUS
    assert hs.slices(V, F, 32) == 1 and hs.slices(S, F, 32) == 1                          # a batch fills the chip by itself
    assert hs.slices(V, F, 8) == 2
    # tiny inputs: one slice; never an empty slice, never fewer than the floor unless the mesh is smaller
    for queries, faces in ((1, 1), (64, 63), (130, 100), (1, 127), (3889, 12)):
        assert hs.slices(queries, faces, 1) == 1, (queries, faces)
    assert hs.slices(1, 128, 1) == 2 and hs.slices(1, 129, 1) == 2 and 100 <= hs.slices(1, 7774, 1) <= 7774 // 64
    rs = np.random.RandomState(0)
    for _ in range(2000):
        queries, faces, N = int(rs.randint(1, 5000)), int(rs.randint(1, 20000)), int(rs.randint(1, 33))
        z = hs.slices(queries, faces, N)
        span = lib.hst_surface_slice_span(faces, z)
        assert z >= 1 and (z - 1) * span < faces <= z * span, (queries, faces, N, z)      # every slice holds a triangle
        assert z == 1 or span >= 64, (queries, faces, N, z, span)


def test_points_of_a_step_with_the_point_surface_term():
    # unchanged without the term
    assert hs.fit3d_points(0.0) == "None" and hs.fit3d_points(0.0, points=True, points_out=True) == "None"
    assert hs.fit3d_points(1.0) == "SampleToObjective" and hs.fit3d_points(1.0, points_out=True) == "SampleToCaller"
    assert hs.fit3d_points(1.0, points=True) == "Callers" and hs.fit3d_points(1.0, points=True, points_out=True) == "CallersCopied"
    # chamfer off, point-surface on: the points are produced all the same
    assert hs.fit3d_points(0.0, point_surface=True) == "SampleToObjective"
    assert hs.fit3d_points(0.0, points_out=True, point_surface=True) == "SampleToCaller"
    assert hs.fit3d_points(0.0, points=True, point_surface=True) == "Callers"
    assert hs.fit3d_points(0.0, points=True, points_out=True, same=True, point_surface=True) == "Callers"
    assert hs.fit3d_points(0.0, points=True, points_out=True, point_surface=True) == "CallersCopied"
    assert hs.fit3d_points(1.0, point_surface=True) == "SampleToObjective"


# ---- Stage without a device ----------------------------------------------------------------------------------------------------
class _Fitter:
    """as much of a SMAL3DFitter as Stage's constructor touches before it reaches the device"""
    batch_size = 1
    device = "cpu"


def _stage_weights(loss_weights):
    from smalify_amd.fitter_3d import trainer
    st = trainer.Stage.__new__(trainer.Stage)
    try:
        trainer.Stage.__init__(st, 1, "deform", _Fitter(), [None], loss_weights=loss_weights)
    except KeyError:
        raise
    except Exception:
        pass                                            # the constructor goes on to the device; the weights are set before
    return st


def test_stage_keeps_the_surface_weights_apart():
    from smalify_amd.fitter_3d import trainer
    assert trainer.default_weights == dict(w_chamfer=1.0, w_edge=1.0, w_normal=0.01, w_laplacian=0.1)
    assert trainer.default_surface_weights == dict(w_point_surface=0.0, w_vert_surface=0.0)
    st = _stage_weights({"w_point_surface": 1.5, "w_edge": 2.0})
    assert st.loss_weights == dict(w_chamfer=1.0, w_edge=2.0, w_normal=0.01, w_laplacian=0.1)
    assert st.surface_weights == dict(w_point_surface=1.5, w_vert_surface=0.0)
    st = _stage_weights(None)
    assert st.surface_weights == trainer.default_surface_weights and st.loss_weights == trainer.default_weights
    assert trainer.default_surface_weights == dict(w_point_surface=0.0, w_vert_surface=0.0)          # a copy was changed, not this
    with pytest.raises(KeyError, match="w_surface"):
        _stage_weights({"w_surface": 1.0})
