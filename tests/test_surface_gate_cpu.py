"""The gated surface term on the host: mesh3d_topology.h's boundary flags and vertex -> face table, mesh3d_math.h's predicate,
boundary rule, closest point with its winner and query normals, smalfit_plan.h's rules for the gate block (all through
tests/host_surface_gate_shim.cpp), the ctypes mirror, Stage's gate dictionary, and the float64 oracle of
tests/surface_gate_cases.py against central differences.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from smalify_amd import _lib
from smalify_amd import engine as eng
from tests import host_surface_gate as hg
from tests import mesh_score_cases as mc
from tests import surface_gate_cases as gc
from tests import surface_term_cases as stc

HEADER_DIR = os.path.join(os.path.dirname(__file__), "..", "include")


# ---- boundary flags by hand ---------------------------------------------------------------------------------------------------
def test_boundary_flags_of_a_single_triangle_are_all_set():
    assert hg.boundary_flags(3, [(0, 1, 2)]).tolist() == [0b111111]


def test_boundary_flags_of_a_closed_tetrahedron_are_all_clear():
    v, f = gc.tetrahedron()
    assert hg.boundary_flags(len(v), f).tolist() == [0, 0, 0, 0]


def test_boundary_flags_of_a_plate_with_its_centre_cell_removed():
    v, f = gc.plate(4, hole=((1, 1),))
    assert len(f) == 16
    got = hg.boundary_flags(len(v), f)
    want, edges, rim = gc.boundary(len(v), f)
    assert np.array_equal(got, want)
    # by hand: the outer rim has 12 edges, the inner one 4; every one of the 16 vertices lies on one of the two
    outer = {tuple(sorted(e)) for e in [(0, 1), (1, 2), (2, 3), (3, 7), (7, 11), (11, 15), (14, 15), (13, 14), (12, 13), (8, 12), (4, 8), (0, 4)]}
    inner = {(5, 6), (6, 10), (9, 10), (5, 9)}
    assert edges == outer | inner and rim == set(range(16))
    set_edges = {tuple(sorted((int(f[i, k]), int(f[i, (k + 1) % 3])))) for i in range(len(f)) for k in range(3) if got[i] >> k & 1}
    assert set_edges == outer | inner
    assert all((got[i] >> 3) == 0b111 for i in range(len(f)))
    # the complete plate: the four inner vertices are no boundary vertices and the inner edges no boundary edges
    v, f = gc.plate(4, hole=())
    got = hg.boundary_flags(len(v), f)
    assert np.array_equal(got, gc.boundary(len(v), f)[0])
    for i in range(len(f)):
        for k in range(3):
            assert bool(got[i] >> (3 + k) & 1) == (int(f[i, k]) not in (5, 6, 9, 10))
            assert bool(got[i] >> k & 1) == (tuple(sorted((int(f[i, k]), int(f[i, (k + 1) % 3])))) in outer)


def test_an_edge_shared_by_three_faces_is_no_boundary():
    v, f = gc.fan_of_three()
    got = hg.boundary_flags(len(v), f)
    assert np.array_equal(got, gc.boundary(len(v), f)[0])
    for i in range(3):
        k = [j for j in range(3) if {int(f[i, j]), int(f[i, (j + 1) % 3])} == {0, 1}][0]
        assert not got[i] >> k & 1
        assert got[i] & 0b111 == 0b111 & ~(1 << k)
    # 0 and 1 still end the other boundary edges
    assert all((got[i] >> 3) == 0b111 for i in range(3))


def test_boundary_flags_of_the_stand_in_pieces():
    for seed in gc.ORACLE_SEEDS:
        sc = gc.oracle_scene(seed)
        tv, tf = sc["targets"][0]
        assert np.array_equal(hg.boundary_flags(len(tv), tf), gc.boundary(len(tv), tf)[0])


# ---- the vertex -> face table -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ("plate", "tetrahedron", "piece"))
def test_vertex_face_table_against_numpy(mesh):
    v, f = {"plate": lambda: gc.plate(4), "tetrahedron": gc.tetrahedron, "piece": lambda: gc.standin_piece(300, 1)}[mesh]()
    off, vf = hg.vertex_faces(len(v), f)
    assert off[0] == 0 and off[-1] == 3 * len(f)
    for vert in range(len(v)):
        want = np.nonzero((f == vert).any(1))[0]
        assert np.array_equal(vf[off[vert]:off[vert + 1]], want), vert


# ---- the predicate --------------------------------------------------------------------------------------------------------------
def test_compatibility_predicate_at_its_edges():
    a, b, c = (0, 0, 0), (1, 0, 0), (0, 1, 0)                       # n = (0, 0, 1)
    up, down, side = (0, 0, 1), (0, 0, -1), (1, 0, 0)
    tilt_in, tilt_out = (np.sqrt(1 - 1e-6), 0, 1e-3), (np.sqrt(1 - 1e-6), 0, -1e-3)

    def ok(u, thr, tri=(a, b, c)):
        return bool(hg.compatible([u], [tri[0]], [tri[1]], [tri[2]], thr)[1][0])
    # c = -1: what smalfit_plan.h calls off; the predicate itself accepts everything at it
    assert ok(up, -1.0) and ok(down, -1.0) and ok(side, -1.0)
    assert not hg.plan(gc.valid_gate().__class__(min_cos_point=-1.0, min_cos_vert=-1.0))["cos_point"]
    # c = 0: either side of perpendicular
    assert ok(tilt_in, 0.0) and not ok(tilt_out, 0.0) and ok(side, 0.0)
    # c = 1: parallel normals pass, anything else does not
    assert ok(up, 1.0) and not ok(tilt_in, 1.0) and not ok(down, 1.0)
    assert ok((0, 0, 1), 1.0, ((0, 0, 0), (3, 0, 0), (0, 0.25, 0)))    # whatever the triangle's size
    # a degenerate face and a zero query normal give 0: compatible exactly when c <= 0
    flat = ((0, 0, 0), (1, 1, 1), (2, 2, 2))
    for u, tri in ((up, flat), ((0, 0, 0), (a, b, c))):
        assert hg.compatible([u], [tri[0]], [tri[1]], [tri[2]], 0.0)[0][0] == 0.0
        assert ok(u, 0.0, tri) and ok(u, -0.5, tri) and not ok(u, 1e-3, tri)
    # a negative threshold: the signed square keeps the order
    back = (np.sqrt(0.75), 0, -0.5)                                  # cosine -0.5
    assert ok(back, -0.6) and not ok(back, -0.4)


# ---- the boundary rule ----------------------------------------------------------------------------------------------------------
def test_boundary_rule_in_every_corner_order():
    for winner in range(3):
        start, end = winner, (winner + 1) % 3
        for flags in range(64):
            edge, s, e = flags >> winner & 1, flags >> (3 + start) & 1, flags >> (3 + end) & 1
            assert hg.boundary_match(flags, winner, 0.0) == bool(edge or s), (winner, flags)
            assert hg.boundary_match(flags, winner, 1.0) == bool(edge or e), (winner, flags)
            for t in (0.5, np.float32(1e-45), np.nextafter(np.float32(1), np.float32(0))):
                assert hg.boundary_match(flags, winner, t) == bool(edge), (winner, flags, t)
    for flags in range(64):
        for t in (0.0, 0.5, 1.0):
            assert not hg.boundary_match(flags, 3, t)                # the plane never matches


def test_boundary_rule_on_the_plate_for_every_corner_order():
    """queries over the hole, over the plate and beyond the outer rim, the faces' corners in all six orders"""
    v, f0 = gc.plate(4, hole=((1, 1),))
    q = np.array([(0.5, 0.5, 0.05), (0.45, 0.52, 0.05), (0.15, 0.2, 0.05), (0.8, 0.9, 0.05), (-0.2, 0.5, 0.05), (1.2, 1.3, 0.0),
                  (1 / 3, 1 / 3 + 0.1, 0.05)], np.float32)
    want_kept = [0, 0, 1, 1, 0, 0, 0]                                # the last sits over an inner rim edge's interior
    for order in stc.CORNER_ORDERS:
        f = f0[:, list(order)]
        o = hg.nearest_gated(q, None, v, f, flags=hg.boundary_flags(len(v), f))
        assert o["kept"].tolist() == want_kept, order
        o = hg.nearest_gated(q, None, v, f, flags=None)
        assert o["kept"].tolist() == [1] * len(q)


# ---- the added outputs change nothing -------------------------------------------------------------------------------------------
def test_closest_point_with_its_winner_keeps_the_bits():
    p, a, b, c = mc.accuracy_pairs()                                 # the pairs the distance's definition was chosen by
    o = hg.closest_where(p, a, b, c)
    for k in ("d2", "bary", "r"):
        assert np.array_equal(o[k].view(np.int32), o[k + "_plain"].view(np.int32)), k
    n = 200000
    ref = stc.closest(p[:n], a[:n], b[:n], c[:n], np.float32)
    agree = o["winner"][:n] == ref["winner"]
    assert agree.mean() > 0.99                                       # (float32 numpy and the shim may break a tie differently)
    t = np.where(o["winner"] == 0, o["bary"][:, 1], np.where(o["winner"] == 1, o["bary"][:, 2], o["bary"][:, 0]))
    seg = o["winner"] < 3
    assert np.array_equal(o["t"][seg], t[seg]) and (o["t"][~seg] == 0).all()
    assert set(np.unique(o["winner"])) == {0, 1, 2, 3}


# ---- the gate block -------------------------------------------------------------------------------------------------------------
def _judge(change_gate, change_term, facts):
    g, a = gc.valid_gate(), stc.valid_args()
    change_gate(g)
    change_term(a)
    return hg.refusal(g, a, **facts)


@pytest.mark.parametrize("case", gc.REFUSALS, ids=[c[0] for c in gc.REFUSALS])
def test_refusals(case):
    _, cg, ct, facts, text = case
    assert _judge(cg, ct, facts) == text


@pytest.mark.parametrize("case", gc.ACCEPTED, ids=[c[0] for c in gc.ACCEPTED])
def test_accepted_edges(case):
    _, cg, ct, facts = case
    assert _judge(cg, ct, facts) is None


def test_refusal_order():
    """a block with every fault at once names the first; mended one at a time it names the next"""
    g, a = gc.valid_gate(), stc.valid_args()
    g.struct_size -= 4
    g.min_cos_point, g.min_cos_vert, g.kept = 2.0, float("nan"), None
    a.w_point_surface = 0.0
    seen = [hg.refusal(g, a, targets=False)]
    g.struct_size += 4
    seen.append(hg.refusal(g, a, targets=False))
    g.min_cos_point = 0.5
    seen.append(hg.refusal(g, a, targets=False))
    g.min_cos_vert = 0.5
    seen.append(hg.refusal(g, a, targets=False))
    g.kept = 0x11000
    seen.append(hg.refusal(g, a, targets=False))
    seen.append(hg.refusal(g, a, targets=True))
    assert seen == [gc.SIZE_TEXT, "min_cos_point must be <= 1 and not NaN", "min_cos_vert must be <= 1 and not NaN", "kept missing",
                    "a vertex gate needs the target meshes", "point_kept given while the point direction is skipped"]


def test_the_plan_of_a_block():
    assert hg.plan(None) == dict(any=False, cos_point=False, cos_vert=False, boundary=False, cc_point=0.0, cc_vert=0.0,
                                 tau2_point=np.inf, tau2_vert=np.inf)
    g = gc.valid_gate()
    p = hg.plan(g)
    assert p["any"] and p["cos_point"] and p["cos_vert"] and p["boundary"]
    assert p["cc_point"] == np.float32(0.25) and p["tau2_vert"] == np.float32(np.float32(0.1) * np.float32(0.1))
    g.min_cos_vert = -0.5
    assert hg.plan(g)["cc_vert"] == np.float32(-0.25)
    # a skipped direction switches nothing on
    p = hg.plan(g, point_dir=False, vert_dir=True)
    assert not p["cos_point"] and p["tau2_point"] == np.inf and p["cos_vert"]
    p = hg.plan(g, point_dir=True, vert_dir=False)
    assert not p["cos_vert"] and not p["boundary"] and p["tau2_vert"] == np.inf
    # every gate off, no mask asked for: nothing gated runs; a mask alone brings the counting kernels in
    off = _lib.SurfaceGateArgs()
    off.kept = 0x1000
    assert not hg.plan(off)["any"]
    off.vert_kept = 0x2000
    assert hg.plan(off)["any"] and not hg.plan(off, vert_dir=False)["any"]
    for tau in (0.0, -1.0, float("inf"), float("nan")):
        off.max_dist_point = tau
        assert hg.plan(off, vert_dir=False)["tau2_point"] == np.inf and not hg.plan(off, vert_dir=False)["any"]


def test_struct_size_and_offsets_against_gcc(tmp_path):
    lib = hg.load()
    assert lib.hsg_sizeof_args() == C.sizeof(_lib.SurfaceGateArgs)
    assert lib.hsg_sizeof_term_args() == C.sizeof(_lib.SurfaceTermArgs)        # no existing struct changed
    assert lib.hsg_sizeof_fit3d_args() == C.sizeof(_lib.Fit3dArgs)
    assert hg.offsets() == [getattr(_lib.SurfaceGateArgs, n).offset for n, _ in _lib.SurfaceGateArgs._fields_]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "smalfit.h"', "int main(void) {",
             'printf("%zu\\n", sizeof(smalfit_surface_gate_args));']
    lines += ['printf("%%zu\\n", offsetof(smalfit_surface_gate_args, %s));' % n for n, _ in _lib.SurfaceGateArgs._fields_]
    (tmp_path / "layout.c").write_text("\n".join(lines + ["return 0; }"]))
    subprocess.run(["gcc", "-I", HEADER_DIR, str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(_lib.SurfaceGateArgs)] + hg.offsets()


def test_the_binding_names_the_new_calls():
    new = {"smalfit_mesh_surface_eval_gated", "smalfit_fit3d_step_gated", "smalfit_mesh_targets_sample_normals"}
    assert new <= set(_lib.SIGNATURES) & set(_lib.LAZY_SYMBOLS)
    g = _lib.SurfaceGateArgs()
    assert g.min_cos_point == -1.0 and g.min_cos_vert == -1.0 and g.reject_boundary == 0 and g.max_dist_point == 0.0


# ---- Stage's gates ----------------------------------------------------------------------------------------------------------------
def test_gate_dictionary():
    assert eng.surface_gates() == gc.open_gates() == eng.surface_gates({})
    g = eng.surface_gates(dict(max_dist_vert=0.25, reject_boundary=1))
    assert g["max_dist_vert"] == 0.25 and g["reject_boundary"] is True and g["min_cos_vert"] == -1.0
    with pytest.raises(KeyError, match="unknown surface gate 'max_dist'"):
        eng.surface_gates(dict(max_dist=0.1))
    b = eng.surface_gate_block(dict(min_cos_point=0.5, max_dist_point=0.125))
    assert (b.min_cos_point, b.max_dist_point, b.min_cos_vert, b.reject_boundary) == (0.5, 0.125, -1.0, 0)
    assert b.struct_size == C.sizeof(_lib.SurfaceGateArgs)


def test_stage_takes_surface_gates_and_refuses_unknown_keys():
    import inspect
    from smalify_amd.fitter_3d import trainer
    assert inspect.signature(trainer.Stage.__init__).parameters["surface_gates"].default is None
    assert trainer.default_weights == dict(w_chamfer=1.0, w_edge=1.0, w_normal=0.01, w_laplacian=0.1)
    assert trainer.default_surface_weights == dict(w_point_surface=0.0, w_vert_surface=0.0)
    st = trainer.Stage.__new__(trainer.Stage)                        # the properties read two dictionaries
    st.surface_weights = dict(w_point_surface=1.0, w_vert_surface=1.0)
    st.surface_gates = eng.surface_gates(None)
    assert st.surface_on and not st.gates_on
    for k, v in (("max_dist_point", 0.1), ("max_dist_vert", 0.1), ("min_cos_point", 0.0), ("min_cos_vert", -0.5), ("reject_boundary", True)):
        st.surface_gates = eng.surface_gates({k: v})
        assert st.gates_on, k
    st.surface_gates = eng.surface_gates(dict(max_dist_point=float("inf"), max_dist_vert=-1.0, min_cos_vert=-1.0))
    assert not st.gates_on


def test_stage_yaml_block_parses_into_the_gates():
    yaml = pytest.importorskip("yaml")
    cfg = yaml.safe_load("stages:\n  fit:\n    scheme: default\n    nits: 3\n    surface_gates:\n      max_dist_vert: 0.2\n"
                         "      reject_boundary: true\n      min_cos_point: 0.25\n")
    kw = cfg["stages"]["fit"]
    assert eng.surface_gates(kw["surface_gates"]) == dict(gc.open_gates(), max_dist_vert=0.2, reject_boundary=True, min_cos_point=0.25)
    with pytest.raises(KeyError):
        eng.surface_gates(dict(kw["surface_gates"], max_dist_points=0.1))


# ---- the oracle -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenes():
    return {seed: gc.oracle_scene(seed) for seed in gc.ORACLE_SEEDS}


def test_cosine_deviation_of_the_shim_and_eps(scenes):
    """|float32 shim - float64| of the signed squared cosine on the oracle scenes' own pairs: what EPS is four times of"""
    worst = 0.0
    for seed, sc in scenes.items():
        tv, tf = sc["targets"][0]
        fit, f = sc["fit"][0], sc["faces"]
        for u32, sv, sf in ((hg.vertex_normals(fit, f), tv, tf), (sc["point_normals"][0], fit, f)):
            want = gc.signed_sq_cos(u32, gc.face_normals(np.asarray(sv, np.float32), sf, np.float64))
            rs = np.random.RandomState(seed)
            qi, fi = rs.randint(0, len(u32), 20000), rs.randint(0, len(sf), 20000)
            tri = np.asarray(sv, np.float32)[sf[fi]]
            got = hg.compatible(u32[qi], tri[:, 0], tri[:, 1], tri[:, 2], 0.0)[0]
            worst = max(worst, float(np.abs(got - want[qi, fi]).max()))
    print("largest deviation of the float32 signed squared cosine: %.3e (recorded %.3e, EPS %.3e)" % (worst, gc.COS_DEVIATION_MEASURED, gc.EPS))
    assert worst <= gc.COS_DEVIATION_MEASURED
    assert gc.EPS == 4 * gc.COS_DEVIATION_MEASURED


def test_the_oracle_alone_stays_under_the_flag_cap(scenes):
    dropped_points = 0
    for seed, sc in scenes.items():
        tv, tf = sc["targets"][0]
        L_ulp = mc.ulp_l(sc["fit"][0], tv)
        for gates in gc.EACH_GATE:
            o = gc.gated_term(sc["fit"], sc["faces"], sc["targets"], sc["points"], sc["point_normals"], 1.0, 1.0, gates,
                              delta=gc.DELTA_ULP * L_ulp)
            for d, name in ((o["point"][0], "points"), (o["vert"][0], "verts")):
                share = d["flagged"].mean()
                print("seed %d %-60s %-6s flagged %.4f kept %d/%d" % (seed, gates, name, share, d["kept"].sum(), len(d["kept"])))
                assert share <= gc.FLAG_CAP, (seed, gates, name)
        # the gates bite: the full set drops some vertices of every scene and keeps most
        assert 0 < o["kept"][0, 0] <= sc["points"].shape[1] and sc["fit"].shape[1] // 2 < o["kept"][0, 1] < sc["fit"].shape[1]
        dropped_points += sc["points"].shape[1] - int(o["kept"][0, 0])
    assert dropped_points > 0


def test_shim_against_the_oracle_on_the_scenes(scenes):
    """the float32 shim's kept masks equal the oracle's at every unflagged query, and its faces are the oracle's or tie with them
    (surface_gate_cases.faces_equivalent)"""
    for seed, sc in scenes.items():
        tv, tf = sc["targets"][0]
        fit, f = sc["fit"][0], sc["faces"]
        delta = gc.DELTA_ULP * mc.ulp_l(fit, tv)
        g = gc.ORACLE_GATES
        o = gc.gated_term(sc["fit"], f, sc["targets"], sc["points"], sc["point_normals"], 1.0, 1.0, g, delta=delta)
        hv = hg.nearest_gated(fit, hg.vertex_normals(fit, f), tv, tf, 3, g["min_cos_vert"], gc.tau2_of(g["max_dist_vert"]),
                              hg.boundary_flags(len(tv), tf))
        hp = hg.nearest_gated(sc["points"][0], sc["point_normals"][0], fit, f, 5, g["min_cos_point"], gc.tau2_of(g["max_dist_point"]))
        for got, want in ((hv, o["vert"][0]), (hp, o["point"][0])):
            ok = ~want["flagged"]
            assert np.array_equal(got["kept"][ok].astype(bool), want["kept"][ok])
            assert ((got["face"] >= 0) == want["kept"])[ok].all()
        assert gc.faces_equivalent(fit, hg.vertex_normals(fit, f), tv, tf, hv["face"], o["vert"][0], g["min_cos_vert"], delta)[~o["vert"][0]["flagged"]].all()
        assert gc.faces_equivalent(sc["points"][0], sc["point_normals"][0], fit, f, hp["face"], o["point"][0], g["min_cos_point"],
                                   delta)[~o["point"][0]["flagged"]].all()
        vn = gc.vertex_normals(fit, f)
        assert np.abs(hg.vertex_normals(fit, f) - vn).max() <= 16 * 2.0 ** -24


def test_fixed_denominators_and_open_gates():
    """with every gate open the gated oracle IS the ungated one; a dropped query leaves the denominators alone"""
    sc = gc.oracle_scene(0, faces_wanted=200, S=40)
    a = gc.gated_term(sc["fit"], sc["faces"], sc["targets"], sc["points"], None, 1.0, 0.5, {})
    b = stc.term(sc["fit"], sc["faces"], sc["targets"], sc["points"], 1.0, 0.5)
    assert a["term"] == b["term"] and np.array_equal(a["dverts"], b["dverts"]) and np.array_equal(a["rows"], b["rows"])
    assert a["kept"].tolist() == [[40, sc["fit"].shape[1]]]
    g = gc.gated_term(sc["fit"], sc["faces"], sc["targets"], sc["points"], None, 1.0, 0.5, dict(max_dist_vert=0.01))
    kept = g["vert"][0]["kept"]
    assert 0 < kept.sum() < len(kept)
    want = (a["vert"][0]["d2"] * kept).sum() / (1 * sc["fit"].shape[1])
    assert abs(g["L_vs"] - want) <= 1e-15 * want


def test_oracle_gradient_against_central_differences():
    """the gates are piecewise constant: away from their edges the oracle's gradient is the derivative of the gated term"""
    sc = gc.oracle_scene(0, faces_wanted=160, S=60)
    g = dict(gc.ORACLE_GATES)
    tv, _ = sc["targets"][0]
    h = 1e-6
    o = gc.gated_term(sc["fit"], sc["faces"], sc["targets"], sc["points"], sc["point_normals"], 1.0, 1.0, g, delta=10 * h, eps=1e-4)
    assert not o["point"][0]["flagged"].any() and not o["vert"][0]["flagged"].any()      # the scene was chosen so
    assert 0 < o["kept"][0, 1] < sc["fit"].shape[1]
    v = sc["fit"].astype(np.float64)
    for i, u in enumerate(stc.smooth_directions(v[0], 3, seed=5)):
        up = gc.gated_term(v + h * u, sc["faces"], sc["targets"], sc["points"], sc["point_normals"], 1.0, 1.0, g)
        dn = gc.gated_term(v - h * u, sc["faces"], sc["targets"], sc["points"], sc["point_normals"], 1.0, 1.0, g)
        assert np.array_equal(up["kept"], dn["kept"])
        cd = (up["term"] - dn["term"]) / (2 * h)
        got = (o["dverts"][0] * u).sum()
        print("direction %d: gradient %.9e central difference %.9e" % (i, got, cd))
        assert abs(got - cd) <= 1e-6 * abs(cd) + 1e-12
