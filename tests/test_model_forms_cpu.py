"""Which branch each model variant of tests/model_forms.py reaches, proved on the host: the tree walks through the library's
own schedule (smalfit_plan.h: tree_levels, through tests/host_plan_shim.cpp), the skinning forms through skin_form, the
sparsity, valence and shape-direction facts from the variants' arrays, and -- for `valence` -- that a gather which stopped
after the kPre corners held in registers would miss the bars of tests/test_gpu_model_forms.py by a factor of ten."""
import numpy as np
import pytest

from oracle import smal_oracle as so
from tests import host_plan
from tests import lbs_forms as lf
from tests import model_forms as mf
from tests.test_gpu_frame_counts import frame_errors


@pytest.fixture(scope="module")
def plan():
    return host_plan.load()


@pytest.mark.parametrize("name", list(mf.TREES))
def test_tree_takes_the_walk_it_is_named_for(plan, name):
    fast, passes, levels = mf.TREES[name]
    parents = mf.tree_parents(name)
    assert plan.parents_ordered(parents)
    t = plan.tree_levels(parents, tables=True)
    assert (t["max_pass"], t["max_children"]) == (16, 4)
    assert (t["fast"], t["walk_passes"], t["nlev"]) == (fast, passes, levels)
    assert t["npass"] == min(passes, t["max_pass"])
    # the rule itself: the fast walk takes exactly the trees that fit its tables
    assert fast == (passes <= t["max_pass"] and t["most_children"] <= t["max_children"])
    # the flat schedule names every non-root joint once, under its parent, with its children in descending order
    seen = []
    for k in range(t["npass"]):
        for s in range(8):
            j = t["pass_joint"][k][s]
            if j == 255:
                continue
            assert s < 5 and t["pass_parent"][k][s] == parents[j]
            kids = sorted((c for c in range(35) if parents[c] == j), reverse=True)
            assert t["pass_nchild"][k][s] == min(len(kids), t["max_children"])
            assert t["pass_child"][k][s][:len(kids)] == kids[:t["max_children"]]
            seen.append(j)
    if fast:
        assert sorted(seen) == list(range(1, 35))


def test_trees_sit_at_the_limits_they_are_named_for(plan):
    t = {name: plan.tree_levels(mf.tree_parents(name)) for name in mf.TREES}
    assert t["fast_limit"]["npass"] == t["fast_limit"]["max_pass"] and t["fast_limit"]["most_children"] == t["fast_limit"]["max_children"]
    assert t["one_past"]["walk_passes"] == t["one_past"]["max_pass"] + 1 and t["one_past"]["most_children"] == t["one_past"]["max_children"]
    assert t["five_children"]["most_children"] == t["five_children"]["max_children"] + 1 and t["five_children"]["walk_passes"] <= 16
    assert t["star"]["root_children"] == 34 and t["star"]["walk_passes"] == 7          # a level of 34 joints: seven passes of five
    assert t["chain"]["most_children"] == 1
    assert set(mf.DEEP_TREES) == {n for n in t if t[n]["nlev"] > t["smal"]["nlev"]}


@pytest.mark.parametrize("name", list(mf.VERT_COUNTS))
def test_frame_counts_reach_every_skinning_form_at_each_vertex_count(plan, name):
    V = mf.VERT_COUNTS[name]
    md = mf.variant(name)
    assert md.v_template.shape[0] == V and plan.padded_verts(V) == lf.padded_verts(V) == mf.facts(md)["Vp"]
    frames = mf.verts_frames(V)
    assert [plan.skin_form(M, V) for M in frames] == [lf.skin_form(M, V) for M in frames]
    assert {plan.skin_form(M, V) for M in frames} == {"plain", "split", "wide"}
    lo, hi = mf.skin_boundary(V)
    assert lo in frames and hi in frames and hi == lo + 1
    assert plan.skin_form(lo, V) == "split" and plan.skin_form(hi, V) == "wide"
    # the boundary is not the stand-in's
    assert (lo, hi) != mf.skin_boundary(lf.NUM_VERTS) or plan.padded_verts(V) != plan.padded_verts(lf.NUM_VERTS)


def test_vertex_counts():
    f = {n: mf.facts(mf.variant(n)) for n in mf.VERT_COUNTS}
    assert f["v3328"]["Vp"] == f["v3328"]["V"] == 13 * 256                          # no padding lane
    assert f["v3056"]["V"] == mf.MIN_VERTS == max(so.LANDMARKS) + 1 and f["v3056"]["Vp"] == 3072
    assert f["v4100"]["Vp"] == 4352 and f["v4100"]["F"] > mf.facts(mf.base())["F"]
    for n in f:
        assert f[n]["Vp"] != lf.padded_verts() and (f[n]["Kw"], f[n]["Kj"]) == (4, 5)


def test_the_stand_in_is_what_the_variants_leave():
    f = mf.facts(mf.base())
    assert (f["V"], f["F"], f["NB"], f["Kw"], f["Kw_min"], f["Kj"]) == (3889, 7774, 41, 4, 4, 5)
    assert f["valence_max"] == mf.K_PRE and not f["isolated"] and not f["unskinned_joints"] and not f["unregressed_joints"]


def test_valence_facts():
    md = mf.variant("valence")
    f = mf.facts(md)
    hubs, isolated = mf.valence_facts()
    cc = mf.corner_counts(md.faces, f["V"])
    assert [int(cc[h]) for h in hubs] == [n for _, n in mf.HUBS]
    assert {n for _, n in mf.HUBS} == {mf.K_PRE + 1, 16, 17, 40}
    assert f["isolated"] == sorted(isolated) and {0, f["V"] - 1} < set(isolated)
    assert hubs[0] in so.LANDMARKS and set(isolated) & set(so.LANDMARKS) and not set(hubs) & set(isolated)
    assert f["valence_max"] == 40
    # the kernel's corner order is a permutation of the faces, and a hub's first kPre corners stay with it
    order = mf.internal_face_order(md)
    assert sorted(order) == list(range(f["F"]))
    cut = mf.truncated_faces(md, hubs)
    assert [int((cut == h).sum()) for h in hubs] == [mf.K_PRE] * len(hubs)
    assert [int((cut == f["V"] + k).sum()) for k in range(len(hubs))] == [n - mf.K_PRE for _, n in mf.HUBS]
    # the new faces have extent: none is degenerate in the template
    vt = np.asarray(md.v_template, np.float64)
    new = np.asarray(md.faces)[-sum(n for _, n in mf.HUBS):]
    area = np.linalg.norm(np.cross(vt[md.faces[:, 1]] - vt[md.faces[:, 0]], vt[md.faces[:, 2]] - vt[md.faces[:, 0]]), axis=1)
    assert len(new) and area[-20:].min() > np.median(area)


@pytest.mark.parametrize("name,K", (("weights8", 8), ("weights9", 9)))
def test_weight_facts(name, K):
    md = mf.variant(name)
    f = mf.facts(md)
    counts = (np.asarray(md.weights) != 0).sum(1)
    assert f["Kw"] == K and set(counts) == set(range(1, K + 1)) and (K > mf.SKIN_SLOTS) == (name == "weights9")
    assert f["unskinned_joints"] == [mf.EMPTY_JOINT] and mf.EMPTY_JOINT != 0
    assert np.abs(np.asarray(md.weights, np.float64).sum(1) - 1).max() < 1e-6


def test_regressor_facts():
    f, f1 = mf.facts(mf.variant("regressor")), mf.facts(mf.variant("regressor_k1"))
    counts = (np.asarray(mf.variant("regressor").J_regressor) != 0).sum(1)
    assert f["Kj"] == mf.REGRESSOR_ROWS == 12 and set(counts) == set(range(13))
    assert (f1["Kj"], f1["Kj_min"]) == (1, 0)
    for x in (f, f1):
        assert x["unregressed_joints"] == [mf.EMPTY_JOINT]
    for n in ("regressor", "regressor_k1"):
        s = np.asarray(mf.variant(n).J_regressor, np.float64).sum(0)
        assert np.abs(np.delete(s, mf.EMPTY_JOINT) - 1).max() < 1e-5 and s[mf.EMPTY_JOINT] == 0


def test_shape_direction_facts(plan):
    for name, NB in mf.BETA_COUNTS.items():
        md = mf.variant(name)
        assert mf.facts(md)["NB"] == NB and np.isfinite(md.shapedirs).all() and np.abs(md.shapedirs[-1]).max() > 0
    nb = mf.BETA_COUNTS
    assert nb["nb48"] == mf.JS_LDS_BETAS == nb["nb49"] - 1                   # the rest-joint table is staged in LDS | read from memory
    assert nb["nb64"] == mf.MAX_MODEL_BETAS == nb["nb65"] - 1 and nb["nb20"] == mf.FIT_BETAS > nb["nb12"]
    # what the library does with each: only nb65 is refused as a model, only nb12 by the fitter
    for name, NB in nb.items():
        assert (plan.model_dims_refusal(3889, 7774, NB) is not None) == (name == "nb65")
        assert (plan.fit_model_refusal(NB) is not None) == (name == "nb12")
    assert [c for c in mf.lbs_cases() if c[0] == "nb65"] == [] and {c[2] for c in mf.lbs_cases() if c[0] == "nb64"} == {64}


def test_lbs_cases_cover_every_variant_and_form():
    cases = mf.lbs_cases()
    names = set(mf.TREES) | {"valence"} | set(mf.SPARSITY) | set(mf.VERT_COUNTS) | (set(mf.BETA_COUNTS) - {"nb65"})
    assert {c[0] for c in cases} == names and len(set(cases)) == len(cases)
    for name in list(mf.TREES) + ["weights8", "weights9"]:
        assert {lf.skin_form(M) for n, M, _ in cases if n == name} == {"plain", "split", "wide"}
    assert set(mf.FIT_VARIANTS) <= names


def test_a_gather_that_stops_after_kpre_corners_misses_the_bars():
    """the regime proof of `valence`: the oracle's gradients with the hubs' 9th-and-later corners cut off differ from the full
    ones by at least ten times the tolerances the device is held to -- in the per-frame gradients of the fused evaluation and,
    vertex by vertex, in the silhouette's adjoint at every hub with a gradient"""
    md = mf.variant("valence")
    hubs, isolated = mf.valence_facts()
    prob, cur, _ = mf.fit_problem(md)
    _, _, full = mf.oracle_fit(prob, cur)
    with mf.silhouette_truncated_at(hubs, mf.truncated_faces(md, hubs)):
        _, _, cut = mf.oracle_fit(prob, cur)
    worst = {k: float(frame_errors(cut[k], full[k]).max()) for k in mf.PER_FRAME}
    assert max(worst.values()) >= 10 * mf.FIT_GRAD_TOL, worst

    verts, w = mf.render_case(md)
    g, g_cut = mf.oracle_render_grad(md, verts, w), mf.oracle_render_grad(md, verts, w, truncate_at=hubs)
    err = mf.row_errors(g_cut, g)
    assert err[:, list(hubs)].max() >= 10 * mf.RENDER_TOL, err[:, list(hubs)]
    others = np.delete(np.arange(g.shape[1]), list(hubs))
    assert err[:, others].max() < 1e-9                       # (the cut touches the hubs alone)
    assert (g[:, list(isolated)] == 0).all()
