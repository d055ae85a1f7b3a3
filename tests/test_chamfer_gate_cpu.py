"""The gated chamfer term without a GPU: mesh3d_math.h's gated scan and smalfit_plan.h's rules through
tests/host_chamfer_gate_shim.cpp against the float64 brute force of tests/chamfer_gate_cases.py, the gate block's layout, the
binding, Stage's keyword and the oracle's own gradient.  Every figure is printed before it is judged."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from smalify_amd import _lib
from smalify_amd import engine as eng
from tests import chamfer_gate_cases as cc
from tests import host_chamfer_gate as hc
from tests import host_surface_gate as hg
from tests import surface_gate_cases as gc
from tests import surface_term_cases as stc

HEADER_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include")
NO_TAG = 0x7fffffff


# ---- the predicate, the tag and the decision ------------------------------------------------------------------------------------
def test_compatibility_at_c_minus_one_zero_and_one():
    x, y = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)
    a = np.array([x, x, x, (0.6, 0.8, 0.0)], np.float32)
    b = np.array([x, y, (-1.0, 0.0, 0.0), (0.6, 0.8, 0.0)], np.float32)
    dot, _ = hc.compatible(a, b, 0.0)
    assert dot.tolist()[:3] == [1.0, 0.0, -1.0]
    assert hc.compatible(a, b, 1.0)[1].tolist()[:3] == [True, False, False]          # c = 1: the same normal only
    assert hc.compatible(a, b, 0.0)[1].tolist()[:3] == [True, True, False]           # c = 0: the facing half, its edge included
    assert hc.compatible(a, b, -1.0)[1].tolist()[:3] == [True, True, True]           # c = -1: everything (the host switches it off)
    # a threshold one float32 above a dot product refuses it, the dot product itself admits it
    d = dot[3]
    assert hc.compatible(a[3:], b[3:], d)[1][0] and not hc.compatible(a[3:], b[3:], np.nextafter(d, np.float32(2)))[1][0]


def test_zero_normals_and_nan():
    z, x = (0.0, 0.0, 0.0), (1.0, 0.0, 0.0)
    nan = (np.nan, 0.0, 0.0)
    a = np.array([z, x, z, nan, x], np.float32)
    b = np.array([x, z, z, x, nan], np.float32)
    dot, ok0 = hc.compatible(a, b, 0.0)
    assert dot[:3].tolist() == [0.0, 0.0, 0.0] and np.isnan(dot[3:]).all()
    assert ok0.tolist() == [True, True, True, False, False]                      # a zero normal gives 0: compatible exactly when c <= 0
    assert hc.compatible(a, b, 1e-30)[1].tolist() == [False] * 5
    assert hc.compatible(a, b, -1.0)[1].tolist() == [True, True, True, False, False]      # a NaN compares false under every finite c
    assert hc.compatible(a, b, -np.inf)[1].tolist() == [True, True, True, False, False]
    # in the scan: a NaN normal is never matched, a NaN position never wins, and with the test off no normal is read
    q = np.zeros((1, 3), np.float32)
    xs = np.array([(0.1, 0, 0), (0.2, 0, 0), (np.nan, 0, 0)], np.float32)
    xn = np.array([nan, x, x], np.float32)
    o = hc.scan(q, [x], xs, xn, min_cos=0.5)
    assert o["index"].tolist() == [1] and o["kept"].tolist() == [True]
    o = hc.scan(q, None, xs, None)
    assert o["index"].tolist() == [0]
    o = hc.scan(q, [nan], xs, xn, min_cos=-0.9)
    assert o["index"].tolist() == [-1] and o["kept"].tolist() == [False] and np.isinf(o["d2"][0])


def test_tag_and_decision():
    assert hc.tag(0, 0) == 0 and hc.tag(0, 1) == 1 and hc.tag(7, 0) == 14 and hc.tag(7, 255) == 15
    assert hc.tag(2 ** 30 - 1, 1) == NO_TAG - 0 and hc.tag(2 ** 30 - 1, 0) < NO_TAG      # (the last index an objective could hold)
    assert hc.match(np.inf, NO_TAG) == (-1, False)
    assert hc.match(0.25, hc.tag(5, 0)) == (5, True)
    assert hc.match(0.25, hc.tag(5, 1)) == (5, True)                   # the bit is read with reject_boundary only
    assert hc.match(0.25, hc.tag(5, 1), reject=True) == (5, False)     # found, judged, dropped: the index stays
    assert hc.match(0.25, hc.tag(5, 0), reject=True) == (5, True)
    assert hc.match(0.25, hc.tag(5, 0), tau2=0.25) == (5, True) and hc.match(0.25, hc.tag(5, 0), tau2=np.nextafter(np.float32(0.25), np.float32(0))) == (5, False)
    assert hc.match(np.nan, NO_TAG, tau2=1.0) == (-1, False)


def test_truncation_at_d_and_the_floats_beside_it():
    """d^2 = 0.25 exactly; tau^2 is the float32 product the host forms"""
    q = np.zeros((1, 3), np.float32)
    x = np.array([(0.5, 0.0, 0.0)], np.float32)
    half = np.float32(0.5)
    for tau, kept in ((half, True), (np.nextafter(half, np.float32(1)), True), (np.nextafter(half, np.float32(0)), False)):
        g = _lib.ChamferGateArgs()
        g.max_dist_point = g.max_dist_vert = float(tau)
        g.kept = 0x1000
        p = hc.plan(g)
        assert p["tau2_point"] == np.float32(tau * tau) == cc.tau2_of(tau) and p["gated_point"] and p["gated_vert"]
        o = hc.scan(q, None, x, None, tau2=p["tau2_point"])
        assert o["kept"].tolist() == [kept] and o["index"].tolist() == [0] and o["d2"][0] == 0.25
        w = cc.gated_direction(q, None, x, None, None, tau=float(tau), dtype=np.float32)
        assert w["kept"].tolist() == [kept]


@pytest.mark.parametrize("X", (1, 2, 3, 5, 511, 512, 513, 1027))
def test_tie_rule_lowest_index_across_waves_and_chunks(X):
    """equal d^2 at several indices: the lowest compatible one wins wherever the quarter split and the chunks put the others"""
    rs = np.random.RandomState(X)
    x = (rs.rand(X, 3).astype(np.float32) + 2.0)
    q = np.zeros((3, 3), np.float32)
    near = np.array((0.25, 0.5, 0.0), np.float32)
    spots = sorted({0, X // 4, X // 2, X - 1, min(X - 1, 600)})
    for first in range(len(spots)):
        xs = x.copy()
        xs[spots[first:]] = near
        o = hc.scan(q, None, xs, None)
        assert o["index"].tolist() == [spots[first]] * 3 and o["kept"].all()
        # ... and with the lowest made incompatible, the next one
        if first + 1 < len(spots):
            xn = np.tile(np.array((0.0, 0.0, 1.0), np.float32), (X, 1))
            xn[spots[first]] = (0.0, 0.0, -1.0)
            o = hc.scan(q, np.tile(np.array((0.0, 0.0, 1.0), np.float32), (3, 1)), xs, xn, min_cos=0.5)
            assert o["index"].tolist() == [spots[first + 1]] * 3


def test_owner_gather_runs_over_every_record_compatible_or_not():
    rs = np.random.RandomState(4)
    X, Q = 700, 5
    x, q = rs.randn(X, 3).astype(np.float32), rs.randn(Q, 3).astype(np.float32)
    xn = -np.tile(np.array((0.0, 0.0, 1.0), np.float32), (X, 1))
    qn = np.tile(np.array((0.0, 0.0, 1.0), np.float32), (Q, 1))
    owner = rs.randint(-1, Q, X).astype(np.int32)
    o = hc.scan(q, qn, x, xn, owner=owner, min_cos=0.5)
    assert (o["index"] == -1).all() and not o["kept"].any()                      # nothing compatible: nothing found
    for i in range(Q):
        want = (q[i].astype(np.float64) - x[owner == i].astype(np.float64)).sum(0)
        assert np.abs(o["gather"][i] - want).max() <= 64 * 2.0 ** -24 * np.abs(q[i] - x[owner == i]).sum()


# ---- the gate block: rules, order, layout, plan ----------------------------------------------------------------------------------
def _judge(change, facts):
    g = cc.valid_gate()
    change(g)
    return hc.refusal(g, **facts)


@pytest.mark.parametrize("case", cc.REFUSALS, ids=[c[0] for c in cc.REFUSALS])
def test_refusals(case):
    _, change, facts, text = case
    assert _judge(change, facts) == text


@pytest.mark.parametrize("case", cc.ACCEPTED, ids=[c[0] for c in cc.ACCEPTED])
def test_accepted_edges(case):
    _, change, facts = case
    assert _judge(change, facts) is None


def test_refusal_order():
    """a block with every fault at once names the first; mended one at a time it names the next"""
    g = cc.valid_gate()
    g.struct_size -= 4
    g.min_cos_point, g.min_cos_vert, g.kept = 2.0, float("nan"), None
    facts = dict(step=True)                                           # a sampling step, handed normals and bytes
    seen = [hc.refusal(g, **facts)]
    g.struct_size += 4
    seen.append(hc.refusal(g, **facts))
    g.min_cos_point = 0.5
    seen.append(hc.refusal(g, **facts))
    g.min_cos_vert = 0.5
    seen.append(hc.refusal(g, **facts))
    g.kept = 0x11000
    seen.append(hc.refusal(g, **facts))
    g.point_normals = g.point_boundary = None
    seen.append(hc.refusal(g, **facts))
    seen.append(hc.refusal(g))                                        # the caller's points now: the normals are wanted first
    g.point_normals = 0x10000
    seen.append(hc.refusal(g))
    assert seen == [cc.SIZE_TEXT, "min_cos_point must be <= 1 and not NaN", "min_cos_vert must be <= 1 and not NaN", "kept missing",
                    cc.SAMPLED_TEXT, None, "a min_cos gate needs point_normals with the caller's points",
                    "reject_boundary needs point_boundary with the caller's points"]


def test_the_plan_of_a_block():
    inf = np.inf
    off = dict(gated_point=False, gated_vert=False, cos_point=False, cos_vert=False, boundary=False, vert_normals=False,
               point_normals=False, point_boundary=False, c_point=-inf, c_vert=-inf, tau2_point=inf, tau2_vert=inf)
    assert hc.plan(None) == off
    g = cc.valid_gate()
    assert hc.plan(g, chamfer_on=False) == off                         # the term off: the block is ignored
    p = hc.plan(g)
    assert all(p[k] for k in hc.PLAN_FLAGS)
    assert p["c_point"] == 0.5 and p["tau2_vert"] == np.float32(np.float32(0.1) * np.float32(0.1))
    # every gate off, no per-query output: nothing gated runs; an output alone brings its direction's gated kernel in
    g = _lib.ChamferGateArgs()
    g.kept = 0x1000
    assert hc.plan(g) == off
    for field, direction in (("point_kept", "gated_point"), ("point_nn", "gated_point"), ("vert_kept", "gated_vert"), ("vert_nn", "gated_vert")):
        g = _lib.ChamferGateArgs()
        g.kept = 0x1000
        setattr(g, field, 0x2000)
        assert hc.plan(g) == dict(off, **{direction: True}), field
    # one gate at a time: which direction it gates and what it reads
    for field, value, on in (("max_dist_point", 0.1, dict(gated_point=True, tau2_point=np.float32(np.float32(0.1) ** 2))),
                             ("max_dist_vert", 0.1, dict(gated_vert=True, tau2_vert=np.float32(np.float32(0.1) ** 2))),
                             ("min_cos_point", 0.0, dict(gated_point=True, cos_point=True, c_point=0.0, vert_normals=True, point_normals=True)),
                             ("min_cos_vert", -0.5, dict(gated_vert=True, cos_vert=True, c_vert=-0.5, vert_normals=True, point_normals=True)),
                             ("reject_boundary", 1, dict(gated_vert=True, boundary=True, point_boundary=True))):
        g = _lib.ChamferGateArgs()
        g.kept = 0x1000
        setattr(g, field, value)
        assert hc.plan(g) == dict(off, **on), field
    for tau in (0.0, -1.0, float("inf"), float("nan")):
        g = _lib.ChamferGateArgs()
        g.kept, g.max_dist_point, g.max_dist_vert = 0x1000, tau, tau
        assert hc.plan(g) == off
    g.min_cos_point = g.min_cos_vert = -1.0
    assert hc.plan(g) == off


def test_staging_constants():
    k = hc.constants()
    assert k == dict(chunk=cc.CHUNK, record_bytes=32, lds_bytes=512 * 32 + 2048 + 3072, ungated_record_bytes=16)
    assert k["lds_bytes"] <= 32 * 1024 and k["record_bytes"] % 16 == 0
    assert k["chunk"] * k["record_bytes"] == 1024 * k["ungated_record_bytes"]       # the ungated chunk's 16 KB


def test_struct_size_and_offsets_against_gcc(tmp_path):
    lib = hc.load()
    assert lib.hcg_sizeof_args() == C.sizeof(_lib.ChamferGateArgs)
    assert lib.hcg_sizeof_surface_gate_args() == C.sizeof(_lib.SurfaceGateArgs)    # no existing struct changed
    assert lib.hcg_sizeof_term_args() == C.sizeof(_lib.SurfaceTermArgs)
    assert lib.hcg_sizeof_fit3d_args() == C.sizeof(_lib.Fit3dArgs)
    assert hc.offsets() == [getattr(_lib.ChamferGateArgs, n).offset for n, _ in _lib.ChamferGateArgs._fields_]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "smalfit.h"', "int main(void) {",
             'printf("%zu\\n", sizeof(smalfit_chamfer_gate_args));']
    lines += ['printf("%%zu\\n", offsetof(smalfit_chamfer_gate_args, %s));' % n for n, _ in _lib.ChamferGateArgs._fields_]
    (tmp_path / "layout.c").write_text("\n".join(lines + ["return 0; }"]))
    subprocess.run(["gcc", "-I", HEADER_DIR, str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(_lib.ChamferGateArgs)] + hc.offsets()
    assert got[1] == 0                                                 # struct_size first


def test_the_binding_names_the_new_calls():
    new = {"smalfit_mesh_objective_eval_gated", "smalfit_fit3d_step_partial", "smalfit_mesh_targets_sample_attrs"}
    assert new <= set(_lib.SIGNATURES) & set(_lib.LAZY_SYMBOLS)
    g = _lib.ChamferGateArgs()
    assert g.min_cos_point == -1.0 and g.min_cos_vert == -1.0 and g.reject_boundary == 0 and g.max_dist_point == 0.0
    assert len(_lib.SIGNATURES["smalfit_mesh_objective_eval_gated"][1]) == len(_lib.SIGNATURES["smalfit_mesh_objective_eval"][1]) + 2
    assert len(_lib.SIGNATURES["smalfit_fit3d_step_partial"][1]) == len(_lib.SIGNATURES["smalfit_fit3d_step_gated"][1]) + 1


# ---- Stage's gates ----------------------------------------------------------------------------------------------------------------
def test_gate_dictionary():
    assert eng.chamfer_gates() == cc.open_gates() == eng.chamfer_gates({})
    g = eng.chamfer_gates(dict(max_dist_vert=0.25, reject_boundary=1))
    assert g["max_dist_vert"] == 0.25 and g["reject_boundary"] is True and g["min_cos_vert"] == -1.0
    with pytest.raises(KeyError, match="unknown chamfer gate 'max_dist'"):
        eng.chamfer_gates(dict(max_dist=0.1))
    b = eng.chamfer_gate_block(dict(min_cos_point=0.5, max_dist_point=0.125))
    assert (b.min_cos_point, b.max_dist_point, b.min_cos_vert, b.reject_boundary) == (0.5, 0.125, -1.0, 0)
    assert b.struct_size == C.sizeof(_lib.ChamferGateArgs)
    assert not eng.chamfer_gates_on(eng.chamfer_gates())
    for k, v in (("max_dist_point", 0.1), ("max_dist_vert", 0.1), ("min_cos_point", 0.0), ("min_cos_vert", -0.5), ("reject_boundary", True)):
        assert eng.chamfer_gates_on(eng.chamfer_gates({k: v})), k
    assert not eng.chamfer_gates_on(eng.chamfer_gates(dict(max_dist_point=float("inf"), max_dist_vert=-1.0, min_cos_vert=-1.0)))


def test_stage_takes_chamfer_gates():
    import inspect
    from smalify_amd.fitter_3d import trainer
    assert inspect.signature(trainer.Stage.__init__).parameters["chamfer_gates"].default is None
    assert inspect.signature(trainer.Stage.__init__).parameters["surface_gates"].default is None
    st = trainer.Stage.__new__(trainer.Stage)                        # the properties read two dictionaries
    st.loss_weights = dict(trainer.default_weights)
    st.chamfer_gates = eng.chamfer_gates(None)
    assert not st.chamfer_gates_on and not st._chamfer_gated()
    st.chamfer_gates = eng.chamfer_gates(dict(reject_boundary=True))
    assert st.chamfer_gates_on and st._chamfer_gated()
    st.loss_weights["w_chamfer"] = 0.0                               # the term off: the gates are ignored, a step is the plain call
    assert st.chamfer_gates_on and not st._chamfer_gated()
    st._chamfer_kept = None
    assert st.last_chamfer_kept is None


def test_stage_yaml_block_parses_into_the_gates():
    yaml = pytest.importorskip("yaml")
    cfg = yaml.safe_load("stages:\n  fit:\n    scheme: default\n    nits: 3\n    chamfer_gates:\n      max_dist_vert: 0.2\n"
                         "      reject_boundary: true\n      min_cos_point: 0.25\n    surface_gates:\n      max_dist_point: 0.1\n")
    kw = cfg["stages"]["fit"]
    assert eng.chamfer_gates(kw["chamfer_gates"]) == dict(cc.open_gates(), max_dist_vert=0.2, reject_boundary=True, min_cos_point=0.25)
    assert eng.surface_gates(kw["surface_gates"]) == dict(gc.open_gates(), max_dist_point=0.1)
    with pytest.raises(KeyError, match="unknown chamfer gate"):
        eng.chamfer_gates(dict(kw["chamfer_gates"], max_dist_points=0.1))


# ---- the oracle -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenes():
    return {seed: cc.oracle_scene(seed) for seed in cc.ORACLE_SEEDS}


def test_dot_deviation_of_the_shim_and_eps(scenes):
    """|float32 shim - float64| of the dot product on the scenes' own pairs of unit normals: what EPS is four times of"""
    worst = 0.0
    for seed, sc in scenes.items():
        u32 = hg.vertex_normals(sc["fit"][0], sc["faces"])
        m32 = sc["point_normals"][0]
        want = u32.astype(np.float64) @ m32.astype(np.float64).T
        vi, si = np.meshgrid(np.arange(len(u32)), np.arange(len(m32)), indexing="ij")
        got = hc.compatible(u32[vi.ravel()], m32[si.ravel()], 0.0)[0].reshape(want.shape)
        worst = max(worst, float(np.abs(got - want).max()))
    print("largest deviation of the float32 dot product: %.3e (recorded %.3e, EPS %.3e)" % (worst, cc.DOT_DEVIATION_MEASURED, cc.EPS))
    assert worst <= cc.DOT_DEVIATION_MEASURED
    assert cc.EPS == 4 * cc.DOT_DEVIATION_MEASURED


def _oracle(sc, gates, **kw):
    delta = cc.DELTA_ULP * cc.ulp_l(sc["fit"], sc["points"])
    return cc.chamfer_gated(sc["fit"], sc["faces"], sc["points"], sc["point_normals"], sc["point_boundary"], 1.0, gates, delta=delta, **kw)


def test_the_oracle_alone_stays_under_the_flag_cap(scenes):
    """the condition of every exact comparison below and on the device: at most 3 % of the queries of a scene are flagged"""
    for seed, sc in scenes.items():
        S, V = sc["points"].shape[1], sc["fit"].shape[1]
        for gates in cc.EACH_GATE:
            o = _oracle(sc, gates)
            for d, name in ((o["point"][0], "points"), (o["vert"][0], "verts")):
                share = d["flagged"].mean()
                print("seed %d %-60s %-6s flagged %.4f kept %d/%d" % (seed, gates, name, share, d["kept"].sum(), len(d["kept"])))
                assert share <= cc.FLAG_CAP, (seed, gates, name)
        # the full set bites in both directions and keeps a good part
        assert S // 4 < o["kept"][0, 0] < S and V // 10 < o["kept"][0, 1] < V, o["kept"]
        assert sc["point_boundary"].any() and not sc["point_boundary"].all()


@pytest.mark.parametrize("gates", cc.EACH_GATE, ids=[",".join(sorted(g)) for g in cc.EACH_GATE])
def test_shim_against_the_oracle_on_the_scenes(scenes, gates):
    """the float32 shim's kept masks and winners equal the oracle's at every unflagged query, both ways"""
    g = dict(cc.open_gates(), **gates)
    for seed, sc in scenes.items():
        o = _oracle(sc, gates)
        fit, pts, pn, pb = sc["fit"][0], sc["points"][0], sc["point_normals"][0], sc["point_boundary"][0]
        u = hg.vertex_normals(fit, sc["faces"])
        hp = hc.scan(pts, pn, fit, u, min_cos=g["min_cos_point"], tau2=cc.tau2_of(g["max_dist_point"]))
        owner = np.where(hp["kept"], hp["index"], -1).astype(np.int32)
        hv = hc.scan(fit, u, pts, pn, xb=pb if g["reject_boundary"] else None, owner=owner, min_cos=g["min_cos_vert"],
                     tau2=cc.tau2_of(g["max_dist_vert"]))
        for got, want, name in ((hp, o["point"][0], "points"), (hv, o["vert"][0], "verts")):
            ok = ~want["flagged"]
            assert np.array_equal(got["kept"][ok], want["kept"][ok]), (seed, name)
            assert np.array_equal(got["index"][ok], want["index"][ok]), (seed, name)
        # the gathered sums are those of the kept points that chose the vertex
        for v in range(len(fit)):
            mine = owner == v
            want = (fit[v].astype(np.float64) - pts[mine].astype(np.float64)).sum(0)
            assert np.abs(hv["gather"][v] - want).max() <= 16 * 2.0 ** -24 * (np.abs(fit[v] - pts[mine]).sum() + 1e-30)
        # the float32 yardstick (the same numpy code) agrees with the oracle at the unflagged queries too
        y = cc.chamfer_gated(sc["fit"], sc["faces"], sc["points"], sc["point_normals"], sc["point_boundary"], 1.0, gates, dtype=np.float32)
        for got, want in ((y["point"][0], o["point"][0]), (y["vert"][0], o["vert"][0])):
            ok = ~want["flagged"]
            assert np.array_equal(got["kept"][ok], want["kept"][ok]) and np.array_equal(got["index"][ok], want["index"][ok])


def test_fixed_denominators_and_open_gates():
    """with every gate open nothing is dropped and the loss is the plain chamfer; a dropped query leaves the denominators alone"""
    sc = cc.oracle_scene(0, faces_wanted=200, S=40)
    S, V = 40, sc["fit"].shape[1]
    a = cc.chamfer_gated(sc["fit"], sc["faces"], sc["points"], None, None, 1.0, {})
    d2 = cc.pair_d2(sc["points"][0], sc["fit"][0])
    assert a["kept"].tolist() == [[S, V]]
    assert abs(a["chamfer"] - (d2.min(1).mean() + d2.min(0).mean())) <= 1e-15 * a["chamfer"]
    g = cc.chamfer_gated(sc["fit"], sc["faces"], sc["points"], None, None, 1.0, dict(max_dist_vert=0.03))
    kept = g["vert"][0]["kept"]
    assert 0 < kept.sum() < V
    want = d2.min(1).mean() + (d2.min(0) * kept).sum() / V
    assert abs(g["chamfer"] - want) <= 1e-15 * want
    assert cc.chamfer_gated(sc["fit"], sc["faces"], sc["points"], None, None, 0.0, {})["dverts"].any() == False   # noqa: E712


def test_oracle_gradient_against_central_differences():
    """the gates are piecewise constant: away from their edges the oracle's gradient is the derivative of the gated loss"""
    sc = cc.oracle_scene(0, faces_wanted=160, S=60)
    g = dict(cc.ORACLE_GATES)
    h = 1e-6
    args = (sc["faces"], sc["points"], sc["point_normals"], sc["point_boundary"], 1.0, g)
    o = cc.chamfer_gated(sc["fit"], *args, delta=10 * h, eps=1e-4, tie=1e-4)
    assert not o["point"][0]["flagged"].any() and not o["vert"][0]["flagged"].any()      # the scene was chosen so
    S, V = sc["points"].shape[1], sc["fit"].shape[1]
    assert 0 < o["kept"][0, 0] < S and 0 < o["kept"][0, 1] < V
    v = sc["fit"].astype(np.float64)
    for i, u in enumerate(stc.smooth_directions(v[0], 3, seed=5)):
        up = cc.chamfer_gated(v + h * u, *args)
        dn = cc.chamfer_gated(v - h * u, *args)
        assert np.array_equal(up["kept"], dn["kept"])
        for a, b in ((up["point"][0], dn["point"][0]), (up["vert"][0], dn["vert"][0])):
            assert np.array_equal(a["index"], b["index"])
        cd = (up["chamfer"] - dn["chamfer"]) / (2 * h)
        got = (o["dverts"][0] * u).sum()
        print("direction %d: gradient %.9e central difference %.9e" % (i, got, cd))
        assert abs(got - cd) <= 1e-6 * abs(cd) + 1e-12
