"""The robust kernel without a GPU: mesh3d_math.h's robust_gm and weighted gather and smalfit_plan.h's rules and plan through
tests/host_robust_shim.cpp, the struct's layout, the binding's dictionaries, Stage's argument and YAML block, and the oracle
of tests/robust_cases.py on its own scenes.  Every figure is printed before it is judged."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

from smalify_amd import _lib
from smalify_amd import engine as eng
from tests import chamfer_gate_cases as cc
from tests import host_robust as hr
from tests import robust_cases as rc
from tests import surface_gate_cases as gc

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "smalfit.h")
U = 2.0 ** -24


# ---- robust_gm ---------------------------------------------------------------------------------------------------------------------
def test_closed_forms_to_the_bit():
    rho, w = hr.gm([0.25, 0.0, 0.75], 0.25)                           # sigma = 0.5; d = 0.5, 0, sqrt(3) / 2
    assert rho.tolist() == [0.125, 0.0, 0.1875] and w.tolist() == [0.25, 1.0, 0.0625]
    assert hr.scale_sq(0.5) == np.float32(0.25) and rc.s2_of(0.5) == np.float32(0.25)
    rho, w = hr.gm([0.0], 1.1754944e-38)                              # the smallest normal s2: u = s2 / s2 = 1 exactly
    assert rho.tolist() == [0.0] and w.tolist() == [1.0]


def test_gm_against_float64():
    """on a float32 d^2 that is exact here u takes two roundings (one add, one divide); rho = d^2 u a third; w = u u doubles u's two
    and adds one: 5 x 2^-24 relative at the most.  The device's bar (rc.WEIGHT_BAR) holds a fortiori"""
    rs = np.random.RandomState(0)
    worst = 0.0
    for sigma in (1e-3, 0.05, 0.5, 7.0, 1e4):
        s2 = hr.scale_sq(sigma)
        assert s2 == rc.s2_of(sigma)
        d2 = (s2 * np.exp(rs.uniform(-12, 12, 4000))).astype(np.float32)
        rho, w = hr.gm(d2, s2)
        rho64, w64 = rc.gm(d2.astype(np.float64), sigma)
        off = max(float(np.abs(rho / rho64 - 1).max()), float(np.abs(w / w64 - 1).max()))
        worst = max(worst, off)
        # monotone and bounded, up to the two roundings of either neighbour: rho rises with d^2 and stays below s2; w
        # falls from 1
        order = np.argsort(d2)
        assert (np.diff(rho[order]) >= -4 * U * rho[order][1:]).all() and (rho <= s2 * (1 + 2 * U)).all()
        assert (np.diff(w[order]) <= 4 * U * w[order][:-1]).all() and (w <= 1).all()
        # rho >= d^2 (1 - d^2 / s^2): what the large-sigma test of the device relies on
        assert (rho64 >= d2 * (1 - d2.astype(np.float64) / float(s2)) - 1e-300).all()
    print("robust_gm against float64: %.3e relative at worst (bound %.3e)" % (worst, 5 * U))
    assert worst <= 5 * U and worst <= rc.WEIGHT_BAR
    # the largest pull: w d peaks at d = sigma / sqrt 3 with (3 sqrt 3 / 16) sigma
    d = np.linspace(0, 5, 200001)
    _, w = rc.gm(d * d, 1.0)
    assert abs((w * d).max() - rc.W_D_MAX) < 1e-9 and abs(d[np.argmax(w * d)] - 1 / np.sqrt(3)) < 1e-4


def test_scale_rules():
    for sigma, on in ((0.0, False), (-0.0, False), (-1.0, False), (float("inf"), False), (float("nan"), False), (1e-30, True), (0.1, True)):
        assert hr.scale_on(sigma) is on and rc.scale_on(sigma) is on and eng._scale_on(sigma) is on, sigma


# ---- the block's rules --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,change,facts,text", rc.REFUSALS, ids=[r[0] for r in rc.REFUSALS])
def test_every_refusal_and_its_text(name, change, facts, text):
    r = rc.valid_block()
    change(r)
    assert hr.refusal(r, **facts) == text


@pytest.mark.parametrize("name,change,facts", rc.ACCEPTED, ids=[r[0] for r in rc.ACCEPTED])
def test_accepted_edges(name, change, facts):
    r = rc.valid_block()
    change(r)
    assert hr.refusal(r, **facts) is None


def test_the_order_of_the_rules():
    """a block that breaks every rule names the first; mended rule by rule, the next"""
    r = rc.valid_block()
    r.struct_size = 4
    r.sigma_chamfer_point, r.sigma_chamfer_vert, r.sigma_surface_point, r.sigma_surface_vert = 1e-30, 1e30, 1e-30, 1e30
    facts = dict(chamfer_call=False)
    seen = []
    mend = (lambda: setattr(r, "struct_size", C.sizeof(_lib.RobustArgs)), lambda: setattr(r, "sigma_chamfer_point", 0.0),
            lambda: setattr(r, "sigma_chamfer_vert", 0.0), lambda: setattr(r, "sigma_surface_point", 0.0),
            lambda: setattr(r, "sigma_surface_vert", 0.0),
            lambda: [setattr(r, k, None) for k in ("chamfer_weight_sums", "chamfer_point_weights", "chamfer_vert_weights")],
            lambda: setattr(r, "surface_point_weights", None), lambda: setattr(r, "surface_vert_weights", None))
    for fix in mend:
        seen.append(hr.refusal(r, **facts))
        fix()
    assert hr.refusal(r, **facts) is None
    assert seen == [rc.SIZE_TEXT, rc.SQUARE % "sigma_chamfer_point", rc.SQUARE % "sigma_chamfer_vert", rc.SQUARE % "sigma_surface_point",
                    rc.SQUARE % "sigma_surface_vert", rc.NO_CHAMFER, rc.OFF % ("surface_point_weights", "sigma_surface_point"),
                    rc.OFF % ("surface_vert_weights", "sigma_surface_vert")]


def test_the_plans_table():
    for on, facts, (chamfer, sp, sv, s2_on) in rc.PLAN_TABLE:
        r = _lib.RobustArgs()
        sig = (0.5, 0.25, 2.0, 0.125)
        for k, flag, s in zip(rc.KEYS, on, sig):
            setattr(r, k, s if flag else 0.0)
        p = hr.plan(r, **facts)
        assert (p["chamfer"], p["surface_point"], p["surface_vert"]) == (chamfer, sp, sv), (on, facts)
        assert p["any"] == (chamfer or sp or sv)
        assert p["s2"] == tuple(float(np.float32(s) * np.float32(s)) if f else 0.0 for f, s in zip(s2_on, sig)), (on, facts)
    none = hr.plan(None)
    assert not none["any"] and none["s2"] == (0.0, 0.0, 0.0, 0.0)
    # the chamfer term runs both robust instantiations when either scale is on; the one that is off reaches the kernel as s2 = 0
    c = hr.constants()
    assert c["robust_lds_bytes"] == c["gated_lds_bytes"] + 4096 and c["robust_lds_bytes"] <= 32 * 1024


# ---- the struct ---------------------------------------------------------------------------------------------------------------------
def test_struct_layout_matches_the_header(tmp_path):
    cls = _lib.RobustArgs
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "smalfit.h"', "int main(void) {",
             'printf("sizeof %zu\\n", sizeof(smalfit_robust_args));']
    for field, _ in cls._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(smalfit_robust_args, %s));' % (field, field))
    lines += ["return 0; }"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = {a: int(b) for a, b in (ln.split() for ln in out.strip().splitlines())}
    assert got["sizeof"] == C.sizeof(cls) == hr.sizeof_args()
    assert [got[f] for f, _ in cls._fields_] == [getattr(cls, f).offset for f, _ in cls._fields_] == hr.offsets()
    assert [f for f, _ in cls._fields_][1:5] == list(rc.KEYS) == list(eng.ROBUST_KEYS)
    assert _lib.RobustArgs().struct_size == C.sizeof(cls)


def test_entry_points_are_bound_lazily():
    for name in ("smalfit_mesh_objective_eval_robust", "smalfit_mesh_surface_eval_robust", "smalfit_fit3d_step_robust"):
        assert name in _lib.SIGNATURES and name in _lib.LAZY_SYMBOLS
        assert _lib.SIGNATURES[name][1][-1] is not None and _lib.SIGNATURES[name][1][-1]._type_ is _lib.RobustArgs


# ---- the weighted gather of the vertices' scan -------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", (1, 2, 5, 1023, 1024, 1025, 2051))
def test_weighted_gather_of_the_scan(S):
    """the scan's gather with the weights staged beside the records against float64, at the chunk edges; with weights of 1 it is the
    unweighted gather's sum"""
    rs = np.random.RandomState(S)
    x = rs.randn(S, 3).astype(np.float32)
    owner = rs.randint(0, 3, S).astype(np.int32)
    wt = rs.rand(S).astype(np.float32)
    q = np.array([0.1, -0.2, 0.3], np.float32)
    idx, best, g = hr.weighted_gather(q, 1, x, owner, wt)
    d2 = ((q.astype(np.float64) - x) ** 2).sum(1)
    assert idx == int(np.argmin(d2)) and abs(best - d2.min()) <= 8 * U * d2.min()
    mine = owner == 1
    want = (wt[mine, None].astype(np.float64) * (q.astype(np.float64) - x[mine])).sum(0)
    mag = (wt[mine, None].astype(np.float64) * np.abs(q.astype(np.float64) - x[mine])).sum(0)
    assert (np.abs(g - want) <= (mine.sum() + 8) * U * mag + 1e-45).all(), (g, want)
    _, _, ones = hr.weighted_gather(q, 1, x, owner, np.ones(S, np.float32))
    plain = (q.astype(np.float64) - x[mine]).sum(0)
    assert (np.abs(ones - plain) <= (mine.sum() + 8) * U * np.abs(q.astype(np.float64) - x[mine]).sum(0) + 1e-45).all()


# ---- the binding and Stage ----------------------------------------------------------------------------------------------------------
def test_robust_dictionary():
    assert eng.robust() == rc.scales() == eng.robust({})
    r = eng.robust(dict(sigma_chamfer_vert=0.25, sigma_surface_point=1))
    assert r == rc.scales(sigma_chamfer_vert=0.25, sigma_surface_point=1.0) and isinstance(r["sigma_surface_point"], float)
    with pytest.raises(KeyError, match="unknown robust key 'sigma'"):
        eng.robust(dict(sigma=0.1))
    b = eng.robust_block(dict(sigma_chamfer_point=0.5, sigma_surface_vert=0.125))
    assert (b.sigma_chamfer_point, b.sigma_chamfer_vert, b.sigma_surface_point, b.sigma_surface_vert) == (0.5, 0.0, 0.0, 0.125)
    assert b.struct_size == C.sizeof(_lib.RobustArgs) and not b.chamfer_weight_sums and not b.surface_vert_weights
    assert not eng.robust_on(eng.robust())
    for k in rc.KEYS:
        assert eng.robust_on(eng.robust({k: 0.1})), k
    assert not eng.robust_on(eng.robust(dict(sigma_chamfer_point=float("inf"), sigma_chamfer_vert=-1.0, sigma_surface_vert=float("nan"))))


def test_stage_takes_robust():
    from smalify_amd.fitter_3d import trainer
    params = inspect.signature(trainer.Stage.__init__).parameters
    assert params["robust"].default is None and list(params)[-1] == "robust"           # added after the existing parameters
    assert list(params)[-3:-1] == ["surface_gates", "chamfer_gates"]
    st = trainer.Stage.__new__(trainer.Stage)                                           # the properties read three dictionaries
    st.loss_weights = dict(trainer.default_weights)
    st.surface_weights = dict(trainer.default_surface_weights)
    st.robust = eng.robust(None)
    st._robust_weights = None
    assert not st.robust_on and not st._robust_applies() and st.last_robust_weights is None
    st.robust = eng.robust(dict(sigma_chamfer_vert=0.1))
    assert st.robust_on and st._robust_applies() and st._robust_chamfer() and not st._robust_surface()
    st.loss_weights["w_chamfer"] = 0.0                                                  # the term off: its scales are off, a step is the plain call
    assert st.robust_on and not st._robust_applies()
    st.robust = eng.robust(dict(sigma_surface_point=0.1))
    assert not st._robust_applies()                                                     # the surface term is off by default
    st.surface_weights["w_point_surface"] = 1.0
    assert st._robust_applies() and st._robust_surface() and not st._robust_chamfer()
    st.surface_weights.update(w_point_surface=0.0, w_vert_surface=1.0)
    assert not st._robust_applies()                                                     # the scale of a skipped direction is off


def test_stage_yaml_block_parses_into_the_scales():
    yaml = pytest.importorskip("yaml")
    cfg = yaml.safe_load("stages:\n  fit:\n    scheme: default\n    nits: 3\n    robust:\n      sigma_chamfer_vert: 0.2\n"
                         "      sigma_surface_point: 0.05\n    chamfer_gates:\n      max_dist_point: 0.1\n")
    kw = cfg["stages"]["fit"]
    assert eng.robust(kw["robust"]) == rc.scales(sigma_chamfer_vert=0.2, sigma_surface_point=0.05)
    assert eng.chamfer_gates(kw["chamfer_gates"]) == dict(cc.open_gates(), max_dist_point=0.1)
    with pytest.raises(KeyError, match="unknown robust key"):
        eng.robust(dict(kw["robust"], sigma_chamfer=0.1))
    from smalify_amd.fitter_3d import trainer
    assert set(kw) - {"scheme", "nits"} <= set(inspect.signature(trainer.Stage.__init__).parameters)      # optimise.py passes the block on


# ---- the oracle on its scenes -------------------------------------------------------------------------------------------------------
def _flag_share(o):
    flagged = sum(int(d["flagged"].sum()) for side in ("point", "vert") for d in o[side])
    total = sum(len(d["flagged"]) for side in ("point", "vert") for d in o[side])
    return flagged / float(total)


def test_every_scene_flags_at_most_three_percent():
    """the condition on the scenes the device tests run: on the oracle alone, gates off and gates on"""
    shares = {}
    for seed in rc.SCENE_SEEDS:
        s = rc.stray_scene(seed)
        delta = cc.DELTA_ULP * cc.ulp_l(s["fit"], s["points"], s["targets"][0][0])
        for tag, cg, sg in (("off", {}, {}), ("on", dict(max_dist_point=0.3, max_dist_vert=0.3, min_cos_point=0.0, min_cos_vert=0.0),
                                              dict(max_dist_point=0.3, max_dist_vert=0.3, min_cos_point=0.0, min_cos_vert=0.0))):
            o = rc.chamfer_robust(s["fit"], s["faces"], s["points"], s["point_normals"], s["point_boundary"], 1.0, cg, rc.ALL_ON, delta=delta)
            shares["stray %d chamfer gates %s" % (seed, tag)] = _flag_share(o)
            o = rc.surface_robust(s["fit"], s["faces"], s["targets"], s["points"], s["point_normals"], 1.0, 1.0, sg, rc.ALL_ON, delta=delta)
            shares["stray %d surface gates %s" % (seed, tag)] = _flag_share(o)
    assert len(rc.sweep()) == 5 + 2 * 9
    for tag, V, S, seed in rc.sweep():
        fit, faces, pts, nrm, bnd = rc.random_problem(V, S, seed=seed)
        delta = cc.DELTA_ULP * cc.ulp_l(fit, pts)
        o = rc.chamfer_robust(fit, faces, pts, nrm, bnd, 1.0, {}, rc.SWEEP_SIGMA, delta=delta)
        shares[tag] = _flag_share(o)
        assert shares[tag] == 0.0, tag      # the ungated call returns no correspondences: the device test takes the oracle's, every one
        o = rc.chamfer_robust(fit, faces, pts, nrm, bnd, 1.0, rc.SWEEP_GATES, rc.SWEEP_SIGMA, delta=delta)
        shares[tag + " gated"] = _flag_share(o)
    from tests import host_surface_term as hs
    from tests import mesh_score_cases as mc
    for tag, F, Q, V, seed in rc.surface_sweep(lambda q, f: hs.slices(q, f, 1)):
        fit, faces, targets, pts, nrm = rc.soup_problem(F, Q, seed, V=V)
        delta = gc.DELTA_ULP * mc.ulp_l(fit[0], targets[0][0])
        for name, gates in (("", {}), (" gated", rc.SOUP_GATES)):
            o = rc.surface_robust(fit, faces, targets, pts, nrm, 1.0, 1.0, gates, rc.SOUP_SIGMA, delta=delta)
            shares["surface " + tag + name] = _flag_share(o)
    for k, v in shares.items():
        print("%-40s flagged %.4f" % (k, v))
        assert v <= rc.FLAG_CAP, k


def test_the_oracle_itself():
    """scales off: the gated oracles' own values; a stray cluster: its points weigh next to nothing and the loss stays below s2"""
    s = rc.stray_scene(0)
    args = (s["fit"], s["faces"], s["points"], s["point_normals"], s["point_boundary"], 1.0, {})
    base = cc.chamfer_gated(*args)
    off = rc.chamfer_robust(*args, rc.scales())
    assert off["chamfer"] == base["chamfer"] and np.array_equal(off["dverts"], base["dverts"])
    assert off["weight_sums"].tolist() == base["kept"].astype(float).tolist()
    sig = rc.scales(sigma_chamfer_point=rc.STRAY_SIGMA, sigma_chamfer_vert=rc.STRAY_SIGMA)
    on = rc.chamfer_robust(*args, sig)
    assert on["w_point"][0][s["stray"]].max() < 1e-3 and on["w_point"][0][~s["stray"]].min() > 0.5
    assert on["chamfer"] < 2 * float(rc.s2_of(rc.STRAY_SIGMA)) and base["chamfer"] > 10 * on["chamfer"]
    # the float32 yardstick of the same code agrees to float32
    y = rc.chamfer_robust(*args, sig, dtype=np.float32)
    assert abs(float(y["chamfer"]) - on["chamfer"]) <= 1e-5 * on["chamfer"]
    sargs = (s["fit"], s["faces"], s["targets"], s["points"], s["point_normals"], 1.0, 1.0, {})
    sbase = gc.gated_term(*sargs)
    soff = rc.surface_robust(*sargs, rc.scales())
    assert soff["term"] == sbase["term"] and np.array_equal(soff["dverts"], sbase["dverts"])
    son = rc.surface_robust(*sargs, rc.scales(sigma_surface_point=rc.STRAY_SIGMA, sigma_surface_vert=rc.STRAY_SIGMA))
    assert son["w_point"][0][s["stray"]].max() < 1e-3 and son["L_ps"] < float(rc.s2_of(rc.STRAY_SIGMA)) < sbase["L_ps"]
    # central differences of the robust loss on the oracle: w is exactly the derivative of rho
    rs = np.random.RandomState(1)
    direction = rs.randn(*s["fit"].shape)
    h = 1e-6
    f = lambda v: float(rc.chamfer_robust(v, *args[1:], sig)["chamfer"])   # noqa: E731
    fd = (f(s["fit"].astype(np.float64) + h * direction) - f(s["fit"].astype(np.float64) - h * direction)) / (2 * h)
    an = float((on["dverts"] * direction).sum())
    print("central difference %.8e analytic %.8e" % (fd, an))
    assert abs(fd - an) <= 1e-5 * abs(an)
