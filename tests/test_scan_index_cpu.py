"""The scan index without a GPU (smalify_amd/csrc/mesh3d_grid.h through tests/host_scan_index_shim.cpp): the library's builder and a
host walker that takes every decision from the header, against the linear scan over all records -- the 64-bit key (d^2 bits high,
lowest face low) BIT FOR BIT.

  walk      single triangles and pairs (a tie across a cell boundary, both face orders); queries inside the box, outside through
            its 6 faces, 12 edges and 8 corners, on cell boundaries, on target vertices, at 100 x the extent (the fallback), NaN
            and +-inf; flat, degenerate and oversize targets; each ungated, compatible, truncated and both; the sliver recipe,
            200 k queries on 5 k faces, with the premise of the slack asserted on it
  rings     the cells of every ring are exactly the cells at that Chebyshev distance, each once
  builder   the sizing rule as numbers, both caps; the CSR by hand on a 2 x 2 x 1 grid; faces ascending; conservative binning
  front     every refusal with its text; layouts against gcc's; the binding's prototypes
  condition duplication <= 8 and oversize share <= 1 % on the stand-in subdivided once and twice at the shipped cell scale
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from smalify_amd import _lib
from tests import host_scan_index as hsi
from tests import mesh_score_cases as mc
from tests import scan_index_cases as sic

K = hsi.constants()
TARGETS = {"faces%d" % F: (lambda F=F: sic.target(F)) for F in sic.TARGET_FACES}
TARGETS.update(flat=sic.flat_target, degenerate=sic.degenerate_target, oversize=sic.oversize_target,
               pair_swapped=lambda: sic.pair(True))


def _index(name, scale=0.0):
    v, f = TARGETS[name]()
    return hsi.Index(v, f, sic.PAIR_SCALE if name in ("faces2", "pair_swapped") and scale == 0.0 else scale)


def _queries(ix, count=390, seed=0):
    lo, hi = ix.box()
    return sic.placements(ix.verts, ix.faces, lo, hi, ix.cell_edge, count, seed)


def _check_truncated(lin, got, how, tau2):
    """with tau2 finite: a key the walk wrote is the linear scan's; a query it wrote none for is one the hit rule drops"""
    d2 = hsi.key_d2(lin)
    dropped = (lin == hsi.NO_KEY) | (d2 > np.float32(tau2))
    wrote = got != hsi.NO_KEY
    assert np.array_equal(got[wrote], lin[wrote])
    assert dropped[~wrote].all()
    assert (wrote | dropped).all() and not (wrote & dropped).any()          # and it drops exactly those
    early = how // 1000 == 1
    assert dropped[early].all()
    return int(early.sum())


@pytest.mark.parametrize("name", sorted(TARGETS))
def test_walk_is_the_linear_scan(name):
    ix = _index(name)
    q = _queries(ix)
    lin = ix.linear_keys(q)
    got, how = ix.walk_keys(q)
    assert np.array_equal(got, lin), np.nonzero(got != lin)[0][:8]
    assert (lin[-3:] == hsi.NO_KEY).all()                                    # NaN, +inf, -inf: no key
    assert (lin[:-3] != hsi.NO_KEY).all()
    vert_hits = hsi.key_d2(lin[3:-3:6])
    assert (vert_hits == 0).all()                                            # queries ON target vertices: d^2 = 0 exactly
    # compatibility on: random normals against the front-facing half and a tighter cone
    u = sic.unit_normals(len(q), 1)
    for c in (0.0, 0.5):
        cc = np.float32(c) * abs(np.float32(c))
        lin_c = ix.linear_keys(q, u, cc)
        got_c, _ = ix.walk_keys(q, u, cc)
        assert np.array_equal(got_c, lin_c), (c, np.nonzero(got_c != lin_c)[0][:8])
    # truncation on, alone and with compatibility: tau of a cell edge or so, and a tight one
    lo, hi = ix.box()
    stopped = 0
    for tau in (ix.cell_edge, 0.05 * float((hi - lo).max()) + 1e-3):
        tau2 = np.float32(tau) * np.float32(tau)
        g, how_t = ix.walk_keys(q, tau2=tau2)
        stopped += _check_truncated(lin, g, how_t, tau2)
        g, how_t = ix.walk_keys(q, u, 0.0, tau2)
        _check_truncated(ix.linear_keys(q, u, 0.0), g, how_t, tau2)
    print(name, ix.stats(), "fallbacks", int((how // 100 % 10 == 1).sum()), "stopped by tau", stopped)
    if name in ("faces1280", "faces513", "oversize"):
        assert stopped > 0                                                   # far from the box, with tau finite, the walk stops early


def test_fallback_is_reached_and_is_the_linear_scan():
    """queries deep inside the icosphere are more than scan_max_rings(1280) = 6 cells from any face: the walk gives up and scans the mesh; so
    does a query with no compatible face.  (At 100 x the extent the walk often ends BEFORE the fallback: the ring planes bound
    the unseen far side of the target beyond the near side it has found)"""
    v, f = sic.icosphere(3)
    ix = hsi.Index(v, f, 0.5)
    last = hsi.max_rings(len(f))
    assert last == 6 and min(ix.stats()["dims"]) > 6 * last
    rs = np.random.RandomState(2)
    q = np.concatenate([np.zeros((1, 3)), 0.2 * rs.uniform(-1, 1, (63, 3))]).astype(np.float32)
    lin = ix.linear_keys(q)
    got, how = ix.walk_keys(q)
    assert np.array_equal(got, lin) and (how == last + 1 + 100).all()
    # outward normals never face the inside of the sphere from a point outside it on the other side: nothing compatible at c = 1
    qo = sic.placements(v, f, *ix.box(), ix.cell_edge, 60, special=False)
    u = sic.unit_normals(len(qo), 4)
    got, how = ix.walk_keys(qo, u, 1.0)
    assert np.array_equal(got, ix.linear_keys(qo, u, 1.0)) and (got == hsi.NO_KEY).sum() > 30
    assert (how[got == hsi.NO_KEY] // 100 % 10 == 1).all()
    # far away, ungated: the same key, fallback or not
    far = (100.0 * sic.box_directions() * 2.0).astype(np.float32)
    got, how = ix.walk_keys(far)
    assert np.array_equal(got, ix.linear_keys(far))
    print("far queries: rings", how % 100, "fallbacks", int((how // 100 % 10 == 1).sum()))


def test_tie_across_a_cell_boundary_goes_to_the_lower_face():
    for swapped in (False, True):
        v, f = sic.pair(swapped)
        ix = hsi.Index(v, f, sic.PAIR_SCALE)
        assert ix.cell_edge == 1.0 and ix.stats()["dims"] == (2, 1, 1)
        off, face, over = ix.csr()
        # x = 1 belongs to the upper cell: the triangle on [0, 1] is listed in both cells, the one on [1, 2] in the upper only
        assert list(off) == [0, 1, 3] and list(face) == ([1, 0, 1] if swapped else [0, 0, 1]) and len(over) == 0
        z = np.array([0.0, 0.25, -0.5, 2.0, 1e-3], np.float32)
        q = np.stack([np.ones_like(z), np.full_like(z, 0.5), z], 1)
        q = np.concatenate([q, q + np.float32([0, 0.25, 0])])
        lin = ix.linear_keys(q)
        got, _ = ix.walk_keys(q)
        assert np.array_equal(got, lin)
        assert (hsi.key_face(got) == 0).all()
        assert np.array_equal(hsi.key_d2(got), np.concatenate([z * z, z * z]))


def test_one_face_target():
    ix = _index("faces1")
    assert ix.stats()["dims"] == (1, 1, 1) and ix.stats()["entries"] == 1
    q = _queries(ix, 64)
    got, how = ix.walk_keys(q)
    assert np.array_equal(got, ix.linear_keys(q)) and (how[:-3] == 1).all()   # one ring: the block is the whole grid


def test_sliver_recipe_and_the_premise_of_the_slack():
    v, f, q = sic.sliver_scene()
    assert len(f) == 5000 and len(q) == 200_000
    ix = hsi.Index(v, f)
    lin = ix.linear_keys(q)
    got, how = ix.walk_keys(q)
    assert np.array_equal(got, lin), int((got != lin).sum())
    print("sliver scene", ix.stats(), "rings histogram", np.bincount(how % 100), "fallbacks", int((how // 100 % 10 == 1).sum()))
    # the premise: no float32 d^2 undercuts the float64 distance to the same triangle by more than 64 ulp(L)
    face = hsi.key_face(lin)
    a, b, c = (v[f[face, k]] for k in range(3))
    d64 = mc.point_triangle_dist(q, a, b, c)
    lo, hi = ix.box()
    L = np.maximum(np.abs(q.astype(np.float64)).max(1), max(np.abs(lo).max(), np.abs(hi).max()))
    undercut = (d64 - np.sqrt(hsi.key_d2(lin).astype(np.float64))) / (L * 2.0 ** -23)
    print("largest undercut of the float64 distance: %.2f ulp(L) (bar 64, slack %g)" % (undercut.max(), K["slack_ulps"]))
    assert undercut.max() <= 64.0
    assert K["slack_ulps"] == 256.0


def test_rings_are_the_chebyshev_shells():
    ix = _index("faces1280", scale=1.0)
    dims = ix.stats()["dims"]
    assert min(dims) >= 5
    zz, yy, xx = np.meshgrid(*(np.arange(d) for d in dims[::-1]), indexing="ij")
    linear = (zz * dims[1] + yy) * dims[0] + xx
    rs = np.random.RandomState(0)
    cells = [(0, 0, 0), tuple(d - 1 for d in dims), (dims[0] // 2, 0, dims[2] - 1)] + [tuple(rs.randint(0, d) for d in dims) for _ in range(8)]
    for c in cells:
        seen = 0
        for r in range(9):
            cheb = np.maximum(np.maximum(abs(xx - c[0]), abs(yy - c[1])), abs(zz - c[2]))
            got = ix.ring_cells(c, r)
            assert len(set(got.tolist())) == len(got)
            assert sorted(got.tolist()) == sorted(linear[cheb == r].tolist()), (c, r)
            seen += len(got)
        assert seen == int((np.maximum(np.maximum(abs(xx - c[0]), abs(yy - c[1])), abs(zz - c[2])) <= 8).sum())
    # the cell of a coordinate: the border cells for everything outside, monotone in between
    lo, hi = ix.box()
    assert tuple(ix.query_cell(lo - 5.0)) == (0, 0, 0) and tuple(ix.query_cell(hi + 5.0)) == tuple(d - 1 for d in dims)
    assert tuple(ix.query_cell(np.float32([3e38, -3e38, 0.0])))[:2] == (dims[0] - 1, 0)
    xs = np.linspace(lo[0] - 0.1, hi[0] + 0.1, 4001).astype(np.float32)
    cx = np.array([ix.query_cell(np.float32([x, 0, 0]))[0] for x in xs])
    assert (np.diff(cx) >= 0).all() and cx[0] == 0 and cx[-1] == dims[0] - 1


def test_sizing_rule_as_numbers():
    s = K["cell_scale"]
    assert s == 2.0
    # h = scale sqrt(area / F); dims = ceil(extent / h)
    h, dims = hsi.grid_dims((1.0, 2.0, 0.5), area=4.0, faces=1600, scale=2.0)
    assert h == np.float32(0.1) and dims == (10, 20, 5)
    h, dims = hsi.grid_dims((1.0, 2.0, 0.0), area=4.0, faces=1600, scale=2.0)
    assert dims == (10, 20, 1)                                               # a zero extent: one cell
    h, dims = hsi.grid_dims((0.0, 0.0, 0.0), area=0.0, faces=3, scale=2.0)
    assert dims == (1, 1, 1) and h == 1.0                                    # no area, no extent
    h, dims = hsi.grid_dims((0.5, 0.0, 0.0), area=0.0, faces=3, scale=2.0)
    assert dims == (1, 1, 1) and h == 0.5                                    # no area: the largest extent
    # the cap on cells per axis: h grows to extent / kScanMaxDim
    h, dims = hsi.grid_dims((1.0, 1e-3, 1e-3), area=1e-6, faces=100, scale=2.0)
    assert dims[0] == K["max_dim"] and h == np.float32(1.0 / K["max_dim"])
    # the cap on cells per mesh: h grows until the product fits
    base = 2.0 * (6.0 / 6e6) ** 0.5
    h, dims = hsi.grid_dims((1.0, 1.0, 1.0), area=6.0, faces=6_000_000, scale=2.0)
    assert dims[0] * dims[1] * dims[2] <= K["max_cells"] and h > base
    assert all(d == int(np.ceil(1.0 / h - 1e-6)) for d in dims) and max(dims) <= K["max_dim"]
    assert (dims[0] + 12) ** 3 > K["max_cells"]                              # ... and no further than a step of the growth
    # the last ring before the fallback: the largest block of at most 2 x faces cells, 48 at most
    assert K["max_rings"] == 48
    assert [hsi.max_rings(n) for n in (1, 13, 14, 513, 7774, 124384, 497536, 10 ** 8)] == [0, 0, 1, 4, 11, 30, 48, 48]
    # the launch: one wave per query, four queries a block
    assert K["grid_queries"] == 4
    assert hsi.launch_grids(3889, 8) == ((973, 8), (973, 8)) and hsi.launch_grids(4, 1)[0] == (1, 1) and hsi.launch_grids(5, 1)[0] == (2, 1)


def test_stats_by_hand_on_a_2_2_1_grid():
    # four unit squares of the plane z = 0, two triangles each; h = 1 exactly: scale sqrt(4 / 8) = 1
    v = np.array([[x, y, 0] for y in (0, 1, 2) for x in (0, 1, 2)], np.float32)
    f = []
    for j in range(2):
        for i in range(2):
            o = 3 * j + i
            f += [[o, o + 1, o + 4], [o, o + 4, o + 3]]
    ix = hsi.Index(v, np.array(f, np.int32), cell_scale=sic.PAIR_SCALE)
    assert ix.cell_edge == 1.0
    s = ix.stats()
    # every triangle's box is a unit square [i, i + 1] x [j, j + 1]: a coordinate ON a cell plane belongs to the upper cell, the
    # box's far side at 2 is clamped into the last cell -- so the squares of column / row 0 overlap two cells along that axis
    counts = {(0, 0): 2, (1, 0): 4, (0, 1): 4, (1, 1): 8}
    off, face, over = ix.csr()
    assert s["dims"] == (2, 2, 1) and s["cells"] == 4 and s["occupied_cells"] == 4 and s["oversize"] == 0
    assert [off[k + 1] - off[k] for k in range(4)] == [counts[(0, 0)], counts[(1, 0)], counts[(0, 1)], counts[(1, 1)]]
    assert s["entries"] == 18 and s["largest_cell"] == 8
    assert s["bytes"] == hsi.load().hsi_sizeof_grid() + 4 * (5 + 18 + 0)
    assert list(face[off[0]:off[1]]) == [0, 1] and list(face[off[3]:off[4]]) == list(range(8))
    for k in range(4):
        assert (np.diff(face[off[k]:off[k + 1]]) > 0).all()                  # faces ascending inside a cell


def test_binning_is_conservative_and_the_oversize_list_holds_the_rest():
    v, f = sic.oversize_target()
    ix = hsi.Index(v, f)
    s = ix.stats()
    off, face, over = ix.csr()
    assert list(over) == [500] and s["oversize"] == 1
    assert s["entries"] <= 8 * len(f)                                        # the one huge triangle did not blow the count up
    # every triangle is listed in the cell of each of its corners and of its centroid
    dims = s["dims"]
    for t in range(0, 500, 7):
        pts = list(v[f[t]]) + [v[f[t]].mean(0)]
        for p in pts:
            c = ix.query_cell(p)
            k = (c[2] * dims[1] + c[1]) * dims[0] + c[0]
            assert t in face[off[k]:off[k + 1]]


def test_every_refusal_and_its_text():
    a = _lib.ScanIndexArgs()
    ok = np.zeros((4, 3), np.float32)
    assert hsi.args_refusal(a, ok) is None
    a.cell_scale = 3.0
    assert hsi.args_refusal(a, ok) is None
    a.struct_size += 4
    assert hsi.args_refusal(a, ok) == "smalfit_scan_index_args.struct_size does not match this library (built against another smalfit.h?)"
    a = _lib.ScanIndexArgs()
    for bad in (-1.0, float("nan"), float("inf")):
        a.cell_scale = bad
        assert hsi.args_refusal(a, ok) == "cell_scale must be finite and >= 0 (0: the library's own)"
    a = _lib.ScanIndexArgs()
    for bad in (np.nan, np.inf, -np.inf):
        v = ok.copy()
        v[2, 1] = bad
        assert hsi.args_refusal(a, v) == "scan index needs finite target vertices"
    s = _lib.ScanIndexStats()
    assert hsi.stats_refusal(s, True, 0, 1) is None
    assert hsi.stats_refusal(None, True, 0, 1) == "null argument"
    assert hsi.stats_refusal(s, False, 0, 1) == "the targets have no scan index (smalfit_mesh_targets_build_index)"
    assert hsi.stats_refusal(s, True, 1, 1) == "mesh out of range" and hsi.stats_refusal(s, True, -1, 1) == "mesh out of range"
    s.struct_size = 8
    assert hsi.stats_refusal(s, True, 0, 1) == "smalfit_scan_index_stats.struct_size does not match this library (built against another smalfit.h?)"


def test_struct_layouts_and_the_binding(tmp_path):
    lib = hsi.load()
    assert lib.hsi_sizeof_args() == C.sizeof(_lib.ScanIndexArgs) == 8
    assert lib.hsi_sizeof_stats() == C.sizeof(_lib.ScanIndexStats) == 48
    assert lib.hsi_sizeof_grid() == 64
    mirror = [getattr(_lib.ScanIndexArgs, n).offset for n, _ in _lib.ScanIndexArgs._fields_] + \
             [getattr(_lib.ScanIndexStats, n).offset for n, _ in _lib.ScanIndexStats._fields_]
    assert hsi.offsets() == mirror
    # ... and gcc's, from include/smalfit.h as C
    header = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include")
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "smalfit.h"', "int main(void) {"]
    for cname, cls in (("smalfit_scan_index_args", _lib.ScanIndexArgs), ("smalfit_scan_index_stats", _lib.ScanIndexStats)):
        lines.append('printf("%%zu\\n", sizeof(%s));' % cname)
        lines += ['printf("%%zu\\n", offsetof(%s, %s));' % (cname, n) for n, _ in cls._fields_]
    (tmp_path / "layout.c").write_text("\n".join(lines + ["return 0; }"]))
    subprocess.run(["gcc", "-I", header, str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [8] + mirror[:2] + [48] + mirror[2:]
    for name in ("smalfit_mesh_targets_build_index", "smalfit_mesh_targets_index_stats"):
        assert name in _lib.SIGNATURES and name in _lib.LAZY_SYMBOLS
    if not _lib.needs_rebuild():
        built = _lib.load()
        assert hasattr(built, "smalfit_mesh_targets_build_index") and hasattr(built, "smalfit_mesh_targets_index_stats")


@pytest.mark.parametrize("subdiv", [1, 2])
def test_condition_on_the_subdivided_stand_in(subdiv):
    """a cell scale that breaks either bound is wrong whatever it times"""
    v, f = sic.standin(subdiv)
    assert len(f) == 7774 * 4 ** subdiv
    s = hsi.Index(v, f).stats()
    dup, share = s["entries"] / len(f), s["oversize"] / len(f)
    print("stand-in x 4^%d: %s, duplication %.2f, oversize share %.4f, entries per occupied cell %.2f"
          % (subdiv, s, dup, share, s["entries"] / s["occupied_cells"]))
    assert dup <= 8.0 and share <= 0.01
    for scale in (1.0, 1.5, 3.0, 4.0):
        t = hsi.Index(v, f, scale).stats()
        print("  cell_scale %.1f: dims %s, duplication %.2f, per occupied cell %.2f, largest %d, oversize %d, %.1f MB"
              % (scale, t["dims"], t["entries"] / len(f), t["entries"] / t["occupied_cells"], t["largest_cell"], t["oversize"], t["bytes"] / 1e6))


def test_fitter_front_end_arguments():
    """Stage(scan_index=), load_meshes(scan_index=), optimise.py --scan_index and TargetMeshes.build_index exist and default to off"""
    import inspect
    from smalify_amd.fitter_3d import optimise, trainer, utils
    assert inspect.signature(trainer.Stage.__init__).parameters["scan_index"].default is False
    assert inspect.signature(utils.load_meshes).parameters["scan_index"].default is False
    assert optimise.build_parser().parse_args([]).scan_index is False
    assert optimise.build_parser().parse_args(["--scan_index"]).scan_index is True
    t = utils.TargetMeshes([np.zeros((3, 3), np.float32)], [np.array([[0, 1, 2]], np.int32)])
    assert t.has_index is False and callable(t.build_index)
    v, f = utils.subdivide_mesh(*sic.target(1), times=2)
    assert len(f) == 16 and len(v) == 15
