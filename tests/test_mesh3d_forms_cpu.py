"""The cases of tests/test_gpu_mesh3d_forms.py reach every branch of the 3D mesh objective, tests/mesh3d_forms.py still
restates the kernels' tie rule and answers like the host's launch geometry (smalify_amd/csrc/smalfit_plan.h, called through
tests/host_plan_shim.cpp), and its float64 reference agrees with the oracle (no ties) and with the host shim of the kernels'
maths (designed ties, lowest index wins).  No GPU needed."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from oracle import mesh3d_oracle as mo
from tests import host_plan
from tests import host_shim
from tests import mesh3d_cases as mc
from tests import mesh3d_forms as mf

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "smalify_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@pytest.fixture(scope="module")
def shim():
    return host_shim.mesh3d()


def _p(a):
    return None if a is None else np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)


def shim_eval(shim, c):
    faces = np.ascontiguousarray(c.faces, np.int32)
    N, V, S = c.N, c.V, c.S
    verts, losses = np.zeros((N, V, 3), np.float32), np.zeros(5, np.float32)
    dverts, dtrans = np.zeros((N, V, 3), np.float32), np.zeros((N, 3), np.float32)
    w = np.asarray(c.weights, np.float32)
    assert shim.hm3_eval(V, len(faces), _p(faces), N, _p(c.lbs), _p(c.trans), _p(c.deform), _p(c.points), S, _p(w),
                         _p(verts), _p(losses), _p(dverts), _p(dtrans)) == 0
    return verts, losses, dverts, dtrans


# ---- the restatement is the source's -------------------------------------------------------------------------------
def test_the_rules_are_the_kernels():
    k = _src("kernels_mesh3d.inc")
    for name, value in (("kChamQueries", mf.CHAM_QUERIES), ("kChamChunk", mf.CHAM_CHUNK), ("kMeshBlock", mf.MESH_BLOCK)):
        m = re.search(r"constexpr int %s = (\d+);" % name, k)
        assert m and int(m.group(1)) == value, name
    # 256 threads = 4 waves of 64 lanes; every wave holds the same 64 queries, one per lane
    assert "__launch_bounds__(256) void mesh3d_chamfer_kernel(Mesh3dArgs a)" in k
    assert "const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);" in k
    assert "const int qi = blockIdx.x * kChamQueries + lane;" in k
    # one staging loop: the ungated kernel's chunk is kChamChunk, a wave scans quarter_span(w, cnt) of it
    assert "constexpr int kChunk = GATED ? kChamGateChunk : kChamChunk;" in k
    assert re.search(r"for \(int base = 0; base < no; base \+= kChunk\) \{\s*const int cnt = min\(kChunk, no - base\);", k)
    assert len(re.findall(r"for \(int base = 0; base < no;", k)) == 1
    assert "const Span sp = quarter_span(w, cnt);" in k
    m = _src("mesh3d_math.h")
    assert re.search(r"Span quarter_span\(int w, int cnt\) \{\s*const int per = \(cnt \+ 3\) >> 2;\s*"
                     r"const int b = w \* per < cnt \? w \* per : cnt;\s*return Span\{b, b \+ per < cnt \? b \+ per : cnt\};", m)
    assert re.search(r"for \(int s = 1; s < 4; \+\+s\) \{\s*nearest_merge\(best, bidx, sd\[s\]\[lane\], si\[s\]\[lane\]\);", k)
    # the tie rule: strict '<' over ascending indices, lexicographic merge
    assert re.search(r"for \(int j = begin; j < end; \+\+j\) \{.*?if \(d2 < best\) \{\s*best = d2;\s*best_idx = index_base \+ j;", m, re.S)
    assert "if (d2 < best || (d2 == best && idx < best_idx)) {" in m
    assert "lowest index" in m


def test_the_grids_are_the_hosts():
    plan = host_plan.load()
    # the block sizes the host divides by are the kernels' (pinned to kernels_mesh3d.inc above)
    assert (plan.MESH_QUERIES, plan.MESH_THREADS) == (mf.CHAM_QUERIES, mf.MESH_BLOCK)
    # the sizes test_rule_boundaries names and every case's, each with a grid around it
    sizes = {(3889, 3000, 11529), (64, 64, 0), (65, 65, 257)} | {(r["V"], r["S"], r["P"]) for r in mf.coverage_table()}
    for V, S, P in sizes:
        for dv, ds, dp in itertools.product((-1, 0, 1, 63, 64, 255, 256), repeat=3):
            v, s, p = V + dv, max(S + ds, 1), max(P + dp, 0)
            assert plan.mesh_grids(v, s, p) == mf.grids(v, s, p), (v, s, p)
            assert plan.mesh_query_blocks(s) == mf.grids(v, s, p)["bx"]          # an evaluation's own bx follows its num_points
    # the chamfer-off call stands as one query (S = 1, see mf.grids), whatever num_points says
    assert [plan.mesh_points(w, 3000) for w in (1.0, 1e-30, 0.0, -1.0)] == [3000, 3000, 1, 1]
    # negative weights are clamped to 0 on the host, like mf.reference does
    for w in (-2.5, -0.0, 0.0, 1e-30, 0.25, 7.0):
        assert plan.mesh_weight(w) == np.float32(max(w, 0.0))


def test_rule_boundaries():
    assert mf.grids(3889, 3000, 11529) == dict(bx=47, by=61, bv=16, bp=46)
    assert mf.grids(64, 64, 0) == dict(bx=1, by=1, bv=1, bp=0) and mf.grids(65, 65, 257)["by"] == 2
    assert mf.chunk_counts(1024) == [1024] and mf.chunk_counts(2049) == [1024, 1024, 1]
    assert mf.wave_ranges(1) == [(0, 1), (1, 1), (1, 1), (1, 1)]
    assert mf.wave_ranges(5) == [(0, 2), (2, 4), (4, 5), (5, 5)]
    assert mf.wave_ranges(1024) == [(0, 256), (256, 512), (512, 768), (768, 1024)]
    assert mf.chamfer_form(0, 3000, 3889) == (4, 817, 0, "partial")       # the stand-in: what the older tests run
    assert mf.chamfer_form(1, 3889, 3000) == (3, 952, 0, "partial")
    assert mf.wave_of(1024 + 76, 2049) == (1, 0) and mf.wave_of(600, 2049) == (0, 2)


# ---- the cases reach every form ------------------------------------------------------------------------------------
def test_cases_reach_every_form():
    rows = mf.coverage_table()
    print("\n%-24s %2s %5s %5s %5s | %-24s | %-24s | %s" % ("case", "N", "V", "S", "P", "role 0 (S q, V scanned)",
                                                            "role 1 (V q, S scanned)", "topology"))
    for r in rows:
        print("%-24s %2d %5d %5d %5d | %-24s | %-24s | %s" % (r["name"], r["N"], r["V"], r["S"], r["P"], r["role0"],
                                                              r["role1"], ", ".join(r["topology"])))
    for role in ("role0", "role1"):
        forms = [r[role] for r in rows]
        chunks = {f[0] for f in forms}
        assert {1, 2} <= chunks and max(chunks) >= 3, role
        assert {1, 2, 3, 4, 5, 1024} <= {f[1] for f in forms}, role
        assert {1, 2, 3} <= {f[2] for f in forms}, role                      # 3, 2 and 1 waves with nothing to scan
        assert {"partial", "full"} <= {f[3] for f in forms}, role
        nq = [r["S"] if role == "role0" else r["V"] for r in rows]
        assert min(nq) < 64 and 1 in [r["S"] for r in rows], role
    assert {r["N"] for r in rows} >= {1, 3, mf.MAX_MESHES}
    Vs = {r["V"] for r in rows}
    assert {63, 64, 65, 255, 256, 257, 1024, 1025, 1026, 1029, 2049} <= Vs      # by / bv edges and the planar copy
    assert {1, 2, 3, 5, 63, 64, 65, 1024, 1025, 1027, 2048, 2053, 3000} <= {r["S"] for r in rows}
    assert any(r["P"] == 0 for r in rows)
    reached = {b for r in rows for b in r["topology"]}
    assert set(mf.TOPOLOGY_BRANCHES) <= reached, set(mf.TOPOLOGY_BRANCHES) - reached


def test_tie_cases_are_placed_as_designed():
    pts, vts = mf.case("ties_points"), mf.case("ties_verts")
    assert {t.placement for t in pts.ties} == {t.placement for t in vts.ties} == {"one wave", "across waves",
                                                                                  "across chunks"}
    for c in (pts, vts):
        no = c.S if c.ties[0].role == 1 else c.V
        for t in c.ties:
            (ca, wa), (cb, wb) = mf.wave_of(t.a, no), mf.wave_of(t.b, no)
            assert t.a < t.b
            want = {"one wave": (ca == cb and wa == wb), "across waves": (ca == cb and wa != wb),
                    "across chunks": ca != cb}[t.placement]
            assert want, (c.name, t)
            o = c.points[t.mesh] if t.role == 1 else c.verts[t.mesh]
            q = c.verts[t.mesh, t.query] if t.role == 1 else c.points[t.mesh, t.query]
            assert not np.array_equal(o[t.a], o[t.b])                       # distinct positions
            for x in np.concatenate([q, o[t.a], o[t.b]]):                   # dyadic within +-4: exact in float32
                assert abs(x) <= 4 and float(x) * 8 == round(float(x) * 8)
    assert vts.V > mf.CHAM_CHUNK


@pytest.mark.parametrize("name", mf.case_names())
def test_every_case_keeps_its_margins(name):
    assert mf.nn_margin(mf.case(name)) == []


@pytest.mark.parametrize("name", [n for n in mf.case_names() if n not in mf.TIE_CASES])
def test_reference_matches_the_oracle(name):
    c = mf.case(name)
    ref = mf.reference(c.verts, c.points, c.faces, c.weights)
    total, terms, g = mc.oracle_objective(c.verts, c.points, c.faces, c.weights)
    for i, k in enumerate(("chamfer", "edge", "normal", "laplacian")):
        assert abs(ref["terms"][i] - terms[k]) <= 1e-12 * max(abs(terms[k]), 1.0), k
    assert abs(ref["total"] - total) <= 1e-12 * abs(total)
    assert mc.rel(ref["dverts"], g) < 1e-12
    if c.P == 0:
        assert ref["terms"][2] == 0.0


@pytest.mark.parametrize("name", mf.TIE_CASES)
def test_tie_cases_discriminate_and_match_the_shim(shim, name):
    c = mf.case(name)
    low = mf.reference(c.verts, c.points, c.faces, c.weights, rule="low")
    high = mf.reference(c.verts, c.points, c.faces, c.weights, rule="high")
    for t in c.ties:
        nn = low["nn_points"] if t.role == 0 else low["nn_verts"]
        nh = high["nn_points"] if t.role == 0 else high["nn_verts"]
        assert nn[t.mesh, t.query] == t.a and nh[t.mesh, t.query] == t.b, t
        rows = t.rows()
        d = mc.rel(high["dverts"][t.mesh, rows], low["dverts"][t.mesh, rows])
        assert d >= 100 * mf.DVERTS_TOL, (t, d)
    verts, losses, dverts, dtrans = shim_eval(shim, c)
    assert np.array_equal(verts, c.verts)
    assert abs(losses[0] - low["terms"][0]) <= 2e-5 * low["terms"][0]
    for t in c.ties:
        rows = t.rows()
        assert mc.rel(dverts[t.mesh, rows], low["dverts"][t.mesh, rows]) < mf.DVERTS_TOL, t
    for n in range(c.N):
        assert mc.rel(dverts[n], low["dverts"][n]) < mf.DVERTS_TOL


@pytest.mark.parametrize("name", ["hand_%s_S%d_N%d" % h for h in mf.HAND_CASES])
def test_hand_meshes_match_the_shim(shim, name):
    """the topology branches through the shim's gather tables (the GPU test runs them through the kernels)"""
    c = mf.case(name)
    ref = mf.reference(c.verts, c.points, c.faces, c.weights)
    verts, losses, dverts, dtrans = shim_eval(shim, c)
    for i in range(4):
        assert abs(losses[i] - ref["terms"][i]) <= 2e-5 * abs(ref["terms"][i]), i
    for n in range(c.N):
        assert mc.rel(dverts[n], ref["dverts"][n]) < mf.DVERTS_TOL, n


def test_reference_tie_rule_on_a_hand_example():
    """a vertex midway between two points: lowest index wins, the gradient follows it"""
    verts = np.array([[[0.0, 0, 0], [3, 0, 0], [0, 3, 0]]])
    pts = np.array([[[0.5, 0, 0], [-0.5, 0, 0]]])
    faces = np.array([[0, 1, 2]])
    low = mf.reference(verts, pts, faces, (1, 0, 0, 0), "low")
    high = mf.reference(verts, pts, faces, (1, 0, 0, 0), "high")
    assert low["nn_verts"][0, 0] == 0 and high["nn_verts"][0, 0] == 1
    # d/dv0: (2/3) (v0 - p_nn) + (2/2) sum over the points choosing v0 (both) of (v0 - p) = (2/3) (v0 - p_nn)
    assert np.allclose(low["dverts"][0, 0], [-1.0 / 3, 0, 0]) and np.allclose(high["dverts"][0, 0], [1.0 / 3, 0, 0])
    assert mo.unique_edges(faces).shape == (3, 2)
