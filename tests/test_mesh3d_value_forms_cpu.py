"""Which regime every case of tests/mesh3d_value_forms.py is in, proved on the host shims (the same mesh3d_math.h the kernels
compile): the windows of A hold every k the GPU test uses and end where the restatement says, the clamped-pair counts of the
normal-term cases, every shifted input of B exact, the designed coincidences of C -- and every equality of A and B already holds
on the shims.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from oracle import mesh3d_oracle as mo
from tests import host_mesh_score as hms
from tests import host_robust as hrb
from tests import host_shim
from tests import host_surface_gate as hsg
from tests import host_surface_term as hst
from tests import mesh3d_cases as m3
from tests import mesh3d_forms as mf
from tests import mesh3d_value_forms as vf
from tests import robust_cases as rc
from tests import surface_gate_cases as sgc


@pytest.fixture(scope="module")
def shim():
    return host_shim.mesh3d()


def _p(a):
    return None if a is None else np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)


def shim_eval(shim, p, weights):
    faces = np.ascontiguousarray(p.faces, np.int32)
    N, V, S = p.N, p.V, p.S
    o = dict(verts=np.zeros((N, V, 3), np.float32), losses=np.zeros(5, np.float32), dverts=np.zeros((N, V, 3), np.float32),
             dtrans=np.zeros((N, 3), np.float32))
    w = np.asarray(weights, np.float32)
    assert shim.hm3_eval(V, len(faces), _p(faces), N, _p(p.lbs), _p(p.trans), _p(p.deform), _p(p.points), S, _p(w), _p(o["verts"]),
                         _p(o["losses"]), _p(o["dverts"]), _p(o["dtrans"])) == 0
    return o


def queries(p, gates=None, sigmas=None):
    """the per-query results of the surface term of problem p on the shims, both directions of every mesh: face, kept, d2, bary, r
    of the (gated) nearest face, rho and w of the robust kernel on it"""
    g = dict(sgc.open_gates(), **(gates or {}))
    v = p.verts
    out = {}
    for n in range(p.N):
        tv, tf = p.targets[n]
        for tag, q, u, sv, sf, tau, mc, sig in (
                ("point", p.points[n], p.point_normals[n], v[n], p.faces, g["max_dist_point"], g["min_cos_point"], "sigma_surface_point"),
                ("vert", v[n], hsg.vertex_normals(v[n], p.faces), tv, tf, g["max_dist_vert"], g["min_cos_vert"], "sigma_surface_vert")):
            if gates is None:
                o = hst.nearest(q, sv, sf)
                o["kept"] = np.ones(len(q), np.uint8)
            else:
                flags = hsg.boundary_flags(len(sv), sf) if g["reject_boundary"] and tag == "vert" else None      # vertex -> target only
                o = hsg.nearest_gated(q, u, sv, sf, min_cos=mc, tau2=sgc.tau2_of(tau), flags=flags)
            if sigmas is not None:
                o["rho"], o["w"] = hrb.gm(o["d2"], hrb.scale_sq(sigmas[sig]))
                rho, w = rc.gm(o["d2"], sigmas[sig])                               # the float64 kernel on the same d^2
                assert np.abs(o["w"] - w).max() <= rc.WEIGHT_BAR and (np.abs(o["rho"] - rho) <= rc.WEIGHT_BAR * rho).all(), (tag, n)
            o["gather"] = hst.gather(len(sv), np.asarray(sf)[o["face"]], o["bary"], o["r"])
            for k, a in o.items():
                out["%s%d/%s" % (tag, n, k)] = a
    return out


def assert_scaled(base, got, degrees, k, what):
    for key, a in base.items():
        deg = degrees[key.split("/")[-1]] if "/" in key else degrees[key]
        assert vf.same_bits(vf.times(a, deg, k), got[key]), (what, key, k)


QUERY_DEGREES = dict(vf.QUERY_DEGREES, gather=1)


# ---- A. scale -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (1, 3))
def test_eval_one_hot_scales_exactly_inside_its_window(shim, N):
    p = vf.ribbon_problem(N)
    lo, hi = vf.eval_window(p)
    print("eval window of %s: %d <= k <= %d" % (p.name, lo, hi))
    assert all(lo <= k <= hi for k in vf.SCALES), (lo, hi)
    for term in ("chamfer", "edge", "laplacian"):
        w, i, dl, dg = vf.ONE_HOT[term]
        base = shim_eval(shim, p, w)
        assert base["losses"][i] > 0
        for k in vf.SCALES + (lo, hi):
            got = shim_eval(shim, vf.scale(p, k), w)
            assert vf.same_bits(vf.times(base["losses"][i], dl, k), got["losses"][i]), (term, k)
            assert vf.same_bits(vf.times(base["dverts"], dg, k), got["dverts"]), (term, k)
            assert vf.same_bits(vf.times(base["dtrans"], dg, k), got["dtrans"]), (term, k)
            assert vf.same_bits(vf.times(base["verts"], 1, k), got["verts"]), (term, k)
    # one k outside: every squared distance underflows to 0, every match falls on index 0
    w, i, dl, dg = vf.ONE_HOT["chamfer"]
    k = vf.OUTSIDE["eval"]
    assert k < lo
    base, out = shim_eval(shim, p, w), shim_eval(shim, vf.scale(p, k), w)
    assert not vf.same_bits(vf.times(base["dverts"], dg, k), out["dverts"])


@pytest.mark.parametrize("name", ("standin", "template"))
def test_normal_term_regimes(shim, name):
    """the three cases by the reference's count, the bit equality between two scales without a clamped pair, and the float64
    reference wherever the set of clamped pairs changes"""
    p = vf.standin_problem() if name == "standin" else vf.template_problem()
    w, i, dl, dg = vf.ONE_HOT["normal"]
    j0, mixed = vf.normal_base_scale(p), vf.normal_mixed_problem(p)
    base_p = vf.scale(p, j0)
    n0, total, _, least = vf.clamped_pairs(base_p.verts, p.faces)
    assert n0 == 0 and least > vf.CLAMP_MARGIN * mf.COS_EPS2
    lo, hi = vf.window(vf.normal_items(base_p.verts, p.faces))
    print("%s: base 2^%d (no pair clamped, min prod %.2e), window of the base %d <= k <= %d" % (name, j0, least, lo, hi))
    base = shim_eval(shim, base_p, w)
    equal = [k for k in vf.SCALES if vf.clamped_pairs(vf.scale(base_p, k).verts, p.faces)[0] == 0]
    assert set(equal) == {3, 10} and all(lo <= k <= hi for k in equal)
    for k in equal:
        got = shim_eval(shim, vf.scale(base_p, k), w)
        assert vf.same_bits(base["losses"][i], got["losses"][i]), k
        assert vf.same_bits(vf.times(base["dverts"], dg, k), got["dverts"]), k
    # outside the window w1 w2 overflows: the term moves
    assert vf.OUTSIDE["normal"] > hi
    out = shim_eval(shim, vf.scale(base_p, vf.OUTSIDE["normal"]), w)
    assert not vf.same_bits(base["losses"][i], out["losses"][i])
    # the regimes by the reference's count
    counts = {}
    for tag, q in (("none", base_p), ("mixed", mixed), ("all", vf.scale(base_p, -12)), ("k=-7", vf.scale(base_p, -7))):
        n, total, margin, _ = vf.clamped_pairs(q.verts, p.faces)
        counts[tag] = n
        if tag != "k=-7":
            assert margin >= vf.CLAMP_MARGIN, (tag, margin)
        o = shim_eval(shim, q, w)
        ref = mf.reference(o["verts"], q.points, p.faces, w)
        assert abs(o["losses"][i] - ref["terms"][i]) <= vf.LOSS_BAR * abs(ref["terms"][i]), (tag, o["losses"][i], ref["terms"][i])
        assert m3.rel(o["dverts"][0], ref["dverts"][0]) < vf.DVERTS_BAR, tag
    print("%s: clamped pairs of %d: %s" % (name, total, counts))
    assert counts["none"] == 0 and 0 < counts["mixed"] < total and counts["all"] == total


@pytest.mark.parametrize("N", (1, 3))
def test_surface_queries_scale_exactly_inside_their_window(N):
    p = vf.ribbon_problem(N)
    lo, hi = vf.window(vf.surface_term_items(p))
    print("surface window of %s: %d <= k <= %d" % (p.name, lo, hi))
    assert all(lo <= k <= hi for k in vf.SCALES), (lo, hi)
    for name, gates, sigmas in vf.SURFACE_VARIANTS:
        base = queries(p, gates, sigmas)
        if name == "plain":
            plain = base
        elif gates is not None:                                                     # the gate decides something: it drops, or picks another face
            kept = np.concatenate([a for key, a in base.items() if key.endswith("/kept")])
            moved = any(not np.array_equal(a, plain[key]) for key, a in base.items() if key.endswith("/face"))
            assert 0 < kept.sum() < len(kept) or moved, name
        for k in vf.SCALES + (lo, hi):
            got = queries(vf.scale(p, k), vf.scaled_gates(gates, k), vf.scaled_sigmas(sigmas, k))
            assert_scaled(base, got, QUERY_DEGREES, k, name)


def test_surface_distance_window_ends_where_the_plane_product_underflows():
    """hms_surface_dist: exact multiples inside the window; outside it h h / |n|^2 has lost its bits"""
    lib = hms.load()
    p = vf.ribbon_problem(1)
    v, (tv, tf) = p.verts[0], p.targets[0]
    lo, hi = vf.window(vf.surface_items(v, tv, tf))
    print("surface distance window: %d <= k <= %d" % (lo, hi))
    base = hms.surface_dist(lib, v, tv, tf)
    for k in vf.SCALES + (lo, hi):
        assert vf.same_bits(vf.times(base, 1, k), hms.surface_dist(lib, vf.ldexp32(v, k), vf.ldexp32(tv, k), tf)), k
    for k in vf.OUTSIDE["surface_dist"]:
        assert not lo <= k <= hi
        assert not vf.same_bits(vf.times(base, 1, k), hms.surface_dist(lib, vf.ldexp32(v, k), vf.ldexp32(tv, k), tf)), k


def test_sampler_scales_exactly(shim):
    p = vf.ribbon_problem(3)
    for n, (tv, tf) in enumerate(p.targets):
        lo, hi = vf.window(vf.sample_items(tv))
        assert all(lo <= k <= hi for k in vf.SCALES)
        base, chosen = vf.shim_sample(shim, tv, tf, 257, 7, 3, n)
        for k in vf.SCALES + (lo, hi):
            got, ch = vf.shim_sample(shim, vf.ldexp32(tv, k), tf, 257, 7, 3, n)
            assert np.array_equal(chosen, ch) and vf.same_bits(vf.times(base, 1, k), got), (n, k)
        k = vf.OUTSIDE["sample"]
        assert k < lo
        assert not vf.same_bits(vf.times(base, 1, k), vf.shim_sample(shim, vf.ldexp32(tv, k), tf, 257, 7, 3, n)[0])


# ---- B. place -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (1, 3))
def test_every_shifted_input_is_exact(N):
    p = vf.ribbon_problem(N, lattice=True)
    assert all(vf.on_lattice(a, 4.0) for a in (p.lbs, p.trans, p.deform, p.points, p.verts)) and all(vf.on_lattice(v, 4.0) for v, _ in p.targets)
    assert 3.5 < p.verts.max() - p.verts.min() <= 8.0
    for o in vf.OFFSETS:
        assert vf.shift_is_exact(p, o), o
    assert not vf.shift_is_exact(p, 1 << 20)                 # (the check can fail: past 2^17 the lattice is finer than float32)


@pytest.mark.parametrize("N", (1, 3))
def test_translation_changes_no_bit_on_the_shims(shim, N):
    p = vf.ribbon_problem(N, lattice=True)
    base = shim_eval(shim, p, mf.GENERAL_WEIGHTS)
    assert all(base["losses"][:4] > 0)
    bq = {name: queries(p, gates, sigmas) for name, gates, sigmas in vf.SURFACE_VARIANTS}
    lib = hms.load()
    bd = [hms.surface_dist(lib, p.verts[n], *p.targets[n]) for n in range(N)]
    for o in vf.OFFSETS:
        q = vf.shift(p, o)
        got = shim_eval(shim, q, mf.GENERAL_WEIGHTS)
        assert np.array_equal(got["verts"], q.verts)
        for key in ("losses", "dverts", "dtrans"):                                  # chamfer, edge, normal, Laplacian and their gradients
            assert vf.same_bits(base[key], got[key]), (o, key)
        for name, gates, sigmas in vf.SURFACE_VARIANTS:
            gq = queries(q, gates, sigmas)
            for key, a in bq[name].items():
                assert vf.same_bits(a, gq[key]), (o, name, key)
        for n in range(N):
            assert vf.same_bits(bd[n], hms.surface_dist(lib, q.verts[n], *q.targets[n])), (o, n)


def test_sampler_far_from_the_origin_against_float64(shim):
    """the sampler interpolates absolute coordinates: no equality, the float64 reference under the YARD rule"""
    p = vf.ribbon_problem(3, lattice=True)
    for o in (0,) + vf.OFFSETS:
        q = vf.shift(p, o) if o else p
        for n, (tv, tf) in enumerate(q.targets):
            got, chosen = vf.shim_sample(shim, tv, tf, 257, 7, 3, n)
            assert np.array_equal(chosen, vf.shim_sample(shim, p.targets[n][0], tf, 257, 7, 3, n)[1])        # areas come from differences
            u, v = vf.sampler_uniforms(shim, 257, 7, 3, n)
            want = vf.sampler_reference(tv, tf, chosen, u, v)
            yard = vf.sampler_deviation(vf.sampler_reference(tv, tf, chosen, u, v, np.float32), want, 4.0)
            err = vf.sampler_deviation(got, want, 4.0)
            print("sampler o=%-6d mesh %d: shim %.2e  (f32 reference %.2e)  bound %.1e" % (o, n, err, yard, vf.bound(vf.SAMPLER_BAR, yard)))
            assert err <= vf.bound(vf.SAMPLER_BAR, yard)


# ---- C. coincidence and collapse -------------------------------------------------------------------------------------------------
def test_a_fit_on_its_target_is_exactly_zero(shim):
    p = vf.coincident_problem()
    assert sorted(map(tuple, p.points[0].tolist())) == sorted(map(tuple, p.verts[0].tolist()))
    o = shim_eval(shim, p, vf.ONE_HOT["chamfer"][0])
    assert o["losses"][0] == 0.0 and vf.same_bits(o["dverts"], np.zeros_like(o["dverts"])) and vf.same_bits(o["dtrans"], np.zeros_like(o["dtrans"]))
    s = vf.self_target_problem()
    for name, gates, sigmas in vf.SURFACE_VARIANTS:
        if name in ("min_cos", "all"):
            continue                                                                # (the self-target problem carries no point normals)
        s2 = vf.replace(s, point_normals=np.zeros_like(s.points))
        q = queries(s2, gates, sigmas)
        for key, a in q.items():
            kind = key.split("/")[-1]
            if kind in ("d2", "r", "rho", "gather"):
                assert not a.any(), (name, key)
            if kind == "w":
                assert (a == 1.0).all(), (name, key)
            if kind == "kept" and name == "max_dist":
                assert a.all(), (name, key)                                         # d = 0 is not beyond max_dist


@pytest.mark.parametrize("name", sorted(vf.COLLAPSES))
def test_collapsed_geometry_is_in_its_regime(shim, name):
    p, same, tie_point = vf.collapsed_problem(name)
    v = p.verts[0].astype(np.float64)
    assert vf.on_lattice(v) and all(np.array_equal(v[same[0]], v[i]) for i in same[1:]) == (name != "face_to_segment")
    pairs = mo.face_pairs(p.faces)
    prod = mf.normal_pair_products(p.verts, pairs)[0]
    assert (prod == 0).any() and "clamped normal pair" in mf.topology_branches(p.case(mf.GENERAL_WEIGHTS))
    o = shim_eval(shim, p, vf.COLLAPSE_WEIGHTS)
    assert all(np.isfinite(a).all() for a in o.values())
    ref = mf.reference(o["verts"], p.points, p.faces, vf.COLLAPSE_WEIGHTS)
    for i in range(4):
        assert abs(o["losses"][i] - ref["terms"][i]) <= vf.LOSS_BAR * abs(ref["terms"][i]), (i, o["losses"], ref["terms"])
    assert m3.rel(o["dverts"][0], ref["dverts"][0]) < vf.DVERTS_BAR
    # a pair with w1 = 0 sits under the clamp with 1 - cos exactly 1
    for z in np.nonzero(prod == 0)[0]:
        one = vf.Problem("pair", vf.PAIR_FACES, p.verts[:, pairs[z]].copy(), np.zeros((1, 3), np.float32), None, p.points, None, None, None)
        assert shim_eval(shim, one, vf.ONE_HOT["normal"][0])["losses"][2] == 1.0
    if name != "face_to_segment":
        # the designed tie: the point's nearest vertices are the coincident ones, the reference's low and high rules part on them
        d2 = mf.sq_dists(p.points[0, tie_point:tie_point + 1], p.verts[0])[0]
        assert all(d2[i] == d2.min() for i in same)
        low, high = ref, mf.reference(o["verts"], p.points, p.faces, mf.GENERAL_WEIGHTS, rule="high")
        assert low["nn_points"][0, tie_point] == same[0] and high["nn_points"][0, tie_point] == same[-1]
        assert m3.rel(o["dverts"][0, same], low["dverts"][0, same]) < vf.DVERTS_BAR <= m3.rel(o["dverts"][0, same], high["dverts"][0, same])


def test_zero_ring_residual_gives_unit_zero(shim):
    v, f = vf.zero_ring_mesh()
    lap, deg = mf.laplacian_residual(v[None], f)
    assert deg[0] == 4 and not lap[0, 0].any()
    p = vf.Problem("fan", f, v[None].copy(), np.zeros((1, 3), np.float32), None, v[None, :2].copy(), None, None, None)
    for o in (0,) + vf.OFFSETS:
        got = shim_eval(shim, vf.shift(p, o) if o else p, vf.ONE_HOT["laplacian"][0])
        ref = mf.reference(got["verts"], None, f, vf.ONE_HOT["laplacian"][0])
        assert abs(got["losses"][3] - ref["terms"][3]) <= vf.LOSS_BAR * ref["terms"][3]
        assert m3.rel(got["dverts"][0], ref["dverts"][0]) < vf.DVERTS_BAR, o


@pytest.mark.parametrize("name", sorted(vf.PAIR_MESHES))
def test_flat_fold_and_coplanar_pair(shim, name):
    v, want = vf.PAIR_MESHES[name]
    pairs = mo.face_pairs(vf.PAIR_FACES)
    assert len(pairs) == 1
    n0, n1 = (np.cross(v[b] - v[a], v[c] - v[a]).astype(np.float64) for a, b, c in vf.PAIR_FACES)
    cos = n0 @ n1 / np.sqrt((n0 @ n0) * (n1 @ n1))
    assert 1.0 - cos == want                                                        # the closed form, exactly, in float64
    p = vf.Problem(name, vf.PAIR_FACES, v[None].copy(), np.zeros((1, 3), np.float32), None, v[None, :2].copy(), None, None, None)
    o = shim_eval(shim, p, vf.ONE_HOT["normal"][0])
    assert abs(o["losses"][2] - want) <= vf.PAIR_EPS and np.isfinite(o["dverts"]).all() and np.isfinite(o["dtrans"]).all()
