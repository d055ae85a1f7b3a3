"""The 3-D mesh kernels at the edges of their value range (-m gpu): mesh3d_chamfer, ring, gather, surface_near / hit / grad, the
grid variants, sample, surface_dist and score_reduce behind eng.MeshObjective.eval / .surface / .score and eng.MeshTargets, on the
cases of tests/mesh3d_value_forms.py (tests/test_mesh3d_value_forms_cpu.py proves on the host which regime each is in).

  A  scale   every output at scale 2^k, k in (-12, -7, 3, 10), is the scale-1 output of the same device times the exact power of
             two: tobytes() equalities.  The normal term: bit-equal between two scales without a clamped pair, the float64
             reference (2e-5 on the term, 2e-4 rel-L2 on d/d verts) where the set of clamped pairs changes.
  B  place   shifted by o (1, -1, 0.5), o in (16, 1024, 65536), on the 2^-7 lattice: chamfer, edge, normal, Laplacian, the surface
             term plain, gated and robust, with and without the index, the score and all their gradients keep their bits.  The
             sampler is held to float64: the larger of 1e-6 and YARD = 2 x the float32 reference's own deviation, and RATCHET = 3 x
             what these kernels measured when tests/golden/hip_mesh3d_value_forms_measured.json was written (floor 1e-6);
             SMALFIT_WRITE_MESH3D_VALUE_MEASURED=<path> writes it.  Every figure is printed next to the yardstick.
  C  coincidence and collapse   closed forms and the existing bars; no NaN in any output."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import mesh3d_oracle as mo  # noqa: E402
from smalify_amd import engine as eng  # noqa: E402
from tests import host_shim  # noqa: E402
from tests import mesh3d_cases as m3  # noqa: E402
from tests import mesh3d_forms as mf  # noqa: E402
from tests import mesh3d_value_forms as vf  # noqa: E402
from tests import robust_cases as rc  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
MEASURED = os.path.join(HERE, "golden", "hip_mesh3d_value_forms_measured.json")
SEED, ITERATION, SAMPLES = 7, 3, 257


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """a device error ends the session: nothing more is started on a GPU that has just faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:
        pytest.exit("device error, stopping: %s" % exc, returncode=3)


def dev(x, dtype=torch.float32):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).cuda()


def host(o):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in o.items()}


def objective(p):
    return eng.MeshObjective(p.V, p.faces, p.N, p.S)


def targets_of(p, index=False):
    t = eng.MeshTargets([v for v, _ in p.targets], [f for _, f in p.targets])
    return t.build_index() if index else t


def run_eval(obj, p, weights, gates=None, sigmas=None):
    return host(obj.eval(dev(p.lbs), dev(p.trans), dev(p.deform), dev(p.points), weights, chamfer_gates=gates, robust=sigmas))


def run_surface(obj, p, tg, gates=None, sigmas=None):
    normals = dev(p.point_normals) if gates is not None and gates.get("min_cos_point", -1.0) > -1.0 else None
    return host(obj.surface(dev(p.verts), tg, dev(p.points), 1.0, 0.5, correspondences=True, gates=gates, point_normals=normals,
                            robust=sigmas))


def run_score(obj, p, tg, thresholds):
    return host(obj.score(dev(p.verts), tg, dev(p.points), thresholds))


def no_nan(o):
    return all(np.isfinite(a).all() for a in o.values() if a.dtype.kind == "f")


def assert_scaled(base, got, degrees, k, what):
    assert set(base) == set(got), what
    for key, a in base.items():
        assert vf.same_bits(vf.times(a, degrees[key], k), got[key]), (what, key, k)


def check_robust_sums(p, o, gates, sigmas):
    """rows and surface_weight_sums against the float64 kernel (robust_cases.gm) on the device's own residuals and kept flags.  The
    bars are float32's: a sum of cnt terms (cnt 2^-24), d^2 against |r|^2 (16 roundings, tests/test_gpu_surface_term.py), the
    kernel's own 3 (rho) or 4 (w, whose sensitivity to d^2 is at most twice rho's) roundings"""
    for n in range(p.N):
        for d, (tag, sig, cnt) in enumerate((("point", "sigma_surface_point", p.S), ("vert", "sigma_surface_vert", p.V))):
            d2 = (o[tag + "_residual"][n].astype(np.float64) ** 2).sum(-1)
            kept = o[tag + "_kept"][n] != 0 if gates is not None else np.ones(cnt, bool)
            rho, w = rc.gm(d2, sigmas[sig])
            assert abs(o["rows"][n, d] - rho[kept].sum()) <= (cnt + 19) * 2.0 ** -24 * rho[kept].sum(), (n, tag, "rho")
            assert abs(o["surface_weight_sums"][n, d] - w[kept].sum()) <= (cnt + 36) * 2.0 ** -24 * w[kept].sum(), (n, tag, "w")
            if kept.any():
                assert np.abs(o[tag + "_weights"][n][kept] - w[kept]).max() <= 36 * 2.0 ** -24, (n, tag)


def assert_same(base, got, what):
    assert set(base) == set(got), what
    for key, a in base.items():
        assert vf.same_bits(a, got[key]), (what, key)


# ---- A. scale -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (1, 3))
def test_eval_one_hot_is_an_exact_power_of_two_of_itself(N):
    p = vf.ribbon_problem(N)
    obj = objective(p)
    scaled = {k: vf.scale(p, k) for k in vf.SCALES}
    for term in ("chamfer", "edge", "laplacian"):
        w, i, dl, dg = vf.ONE_HOT[term]
        base = run_eval(obj, p, w)
        assert base["losses"][i] > 0 and base["losses"][4] == base["losses"][i] and no_nan(base)
        for k, q in scaled.items():
            got = run_eval(obj, q, w)
            for key, deg in (("verts", 1), ("dverts", dg), ("dtrans", dg)):
                assert vf.same_bits(vf.times(base[key], deg, k), got[key]), (term, key, k)
            for j in (i, 4):
                assert vf.same_bits(vf.times(base["losses"][j], dl, k), got["losses"][j]), (term, "losses", j, k)
    # the matches themselves, and the gated and robust kernels of the same scan
    w = vf.ONE_HOT["chamfer"][0]
    base = run_eval(obj, p, w, vf.CHAMFER_GATES, vf.SIGMAS)
    assert 0 < base["point_kept"].sum() < base["point_kept"].size and 0 < base["vert_kept"].sum() < base["vert_kept"].size
    plain = mf.reference(p.verts, p.points, p.faces, w)
    assert np.array_equal(np.where(base["point_kept"] != 0, base["point_nn"], -1), np.where(base["point_kept"] != 0, plain["nn_points"], -1))
    for k, q in scaled.items():
        got = run_eval(obj, q, w, vf.scaled_gates(vf.CHAMFER_GATES, k), vf.scaled_sigmas(vf.SIGMAS, k))
        for key, deg in vf.GATED_EVAL_DEGREES.items():
            a, b = (base[key][[0, 4]], got[key][[0, 4]]) if key == "losses" else (base[key], got[key])
            assert vf.same_bits(vf.times(a, deg, k), b), ("gated and robust", key, k)


@pytest.mark.parametrize("name", ("standin", "template"))
def test_normal_term_between_scales_and_across_the_clamp(name):
    p = vf.standin_problem() if name == "standin" else vf.template_problem()
    w, i, _, dg = vf.ONE_HOT["normal"]
    obj = objective(p)
    base_p = vf.scale(p, vf.normal_base_scale(p))
    base = run_eval(obj, base_p, w)
    for k in (3, 10):                                              # no clamped pair at either scale: the same bits
        got = run_eval(obj, vf.scale(base_p, k), w)
        assert vf.same_bits(base["losses"][i], got["losses"][i]), k
        assert vf.same_bits(vf.times(base["dverts"], dg, k), got["dverts"]), k
    # none, a mix, all under the clamp, and k = -7: the float64 reference with the clamp restated
    for tag, q in (("none", base_p), ("mixed", vf.normal_mixed_problem(p)), ("all", vf.scale(base_p, -12)), ("k=-7", vf.scale(base_p, -7))):
        o = run_eval(obj, q, w)
        assert no_nan(o), tag
        ref = mf.reference(o["verts"], q.points, p.faces, w)
        err, gerr = abs(o["losses"][i] - ref["terms"][i]) / abs(ref["terms"][i]), m3.rel(o["dverts"][0], ref["dverts"][0])
        print("normal term %-9s %-6s clamped %5d of %d: term %.2e (bar %.0e)  dverts %.2e (bar %.0e)"
              % (name, tag, vf.clamped_pairs(q.verts, p.faces)[0], obj.num_face_pairs, err, vf.LOSS_BAR, gerr, vf.DVERTS_BAR))
        assert err <= vf.LOSS_BAR and gerr < vf.DVERTS_BAR, (tag, err, gerr)


@pytest.mark.parametrize("index", (False, True), ids=("linear", "index"))
@pytest.mark.parametrize("variant", vf.SURFACE_VARIANTS, ids=[v[0] for v in vf.SURFACE_VARIANTS])
@pytest.mark.parametrize("N", (1, 3))
def test_surface_term_is_an_exact_power_of_two_of_itself(N, variant, index):
    name, gates, sigmas = variant
    p = vf.ribbon_problem(N)
    obj = objective(p)
    tg = targets_of(p, index)
    base = run_surface(obj, p, tg, gates, sigmas)
    assert no_nan(base) and base["losses"][2] > 0
    if sigmas is not None:
        check_robust_sums(p, base, gates, sigmas)
    stats = tg.index_stats() if index else None
    for k in vf.SCALES:
        q = vf.scale(p, k)
        tq = targets_of(q, index)
        got = run_surface(obj, q, tq, vf.scaled_gates(gates, k), vf.scaled_sigmas(sigmas, k))
        assert_scaled(base, got, vf.SURFACE_DEGREES, k, name)
        if sigmas is not None:
            check_robust_sums(q, got, gates, vf.scaled_sigmas(sigmas, k))
        if index:
            assert [(s["dims"], s["entries"]) for s in tq.index_stats()] == [(s["dims"], s["entries"]) for s in stats], k


@pytest.mark.parametrize("index", (False, True), ids=("linear", "index"))
@pytest.mark.parametrize("N", (1, 3))
def test_score_is_an_exact_power_of_two_of_itself(N, index):
    p = vf.ribbon_problem(N)
    obj = objective(p)
    base = run_score(obj, p, targets_of(p, index), vf.THRESHOLDS)
    assert no_nan(base) and base["within"].min() < base["within"].max()      # the thresholds part the queries
    for k in vf.SCALES:
        q = vf.scale(p, k)
        got = run_score(obj, q, targets_of(q, index), [float(vf.ldexp32(t, k)) for t in vf.THRESHOLDS])
        assert_scaled(base, got, vf.SCORE_DEGREES, k, "score")


def _sample(tg):
    pts, normals, boundary = tg.sample_attrs(SAMPLES, SEED, ITERATION)
    plain = tg.sample(SAMPLES, SEED, ITERATION)
    return host(dict(points=pts, normals=normals, boundary=boundary, plain=plain))


def test_sampler_is_an_exact_power_of_two_of_itself():
    p = vf.ribbon_problem(3)
    base = _sample(targets_of(p))
    assert vf.same_bits(base["points"], base["plain"]) and no_nan(base)
    for k in vf.SCALES:
        got = _sample(targets_of(vf.scale(p, k)))
        assert_scaled(base, got, dict(points=1, plain=1, normals=None, boundary=None), k, "sample")


# ---- B. place -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (1, 3))
def test_translation_changes_no_bit(N):
    p = vf.ribbon_problem(N, lattice=True)
    obj = objective(p)
    w = mf.GENERAL_WEIGHTS

    def everything(q):
        out = {"eval": run_eval(obj, q, w), "eval gated robust": run_eval(obj, q, w, vf.CHAMFER_GATES, vf.SIGMAS)}
        for index in (False, True):
            tg = targets_of(q, index)
            for name, gates, sigmas in vf.SURFACE_VARIANTS:
                out["surface %s %s" % (name, index)] = run_surface(obj, q, tg, gates, sigmas)
            out["score %s" % index] = run_score(obj, q, tg, vf.THRESHOLDS)
        return out

    base = everything(p)
    assert all(no_nan(o) for o in base.values()) and (base["eval"]["losses"] > 0).all()
    for name, gates, sigmas in vf.SURFACE_VARIANTS:                # (the index changes no bit: its own promise, kept on the lattice too)
        assert_same(base["surface %s False" % name], base["surface %s True" % name], name)
    for o in vf.OFFSETS:
        q = vf.shift(p, o)
        got = everything(q)
        assert np.array_equal(got["eval"]["verts"], q.verts)
        for call, b in base.items():
            for key, a in b.items():
                if key != "verts":
                    assert vf.same_bits(a, got[call][key]), (o, call, key)


class Table:
    """the printed figures of one test, the YARD bound, the ratchet and the record of what was measured"""

    def __init__(self):
        self.lines, self.bad, self.measured = [], [], {}
        self.recorded = json.load(open(MEASURED)) if os.path.exists(MEASURED) else {}

    def add(self, key, err, yard, bar, floor):
        limit = vf.bound(bar, yard)
        line = "%-28s hip %.2e  (f32 reference %.2e)  bound %.1e" % (key, err, yard, limit)
        self.lines.append(line)
        self.measured[key] = max(self.measured.get(key, 0.0), float(err))
        if not err <= limit:
            self.bad.append(line)
        if key in self.recorded and err > max(vf.RATCHET * self.recorded[key], floor):
            self.bad.append(line + "   [ratchet: the recorded %.2e]" % self.recorded[key])

    def close(self, capsys):
        with capsys.disabled():
            print("\n" + "\n".join(self.lines))
        path = os.environ.get("SMALFIT_WRITE_MESH3D_VALUE_MEASURED")
        if path:
            doc = json.load(open(path)) if os.path.exists(path) else {}
            doc.update(self.measured)
            json.dump(doc, open(path, "w"), indent=1, sort_keys=True)
        assert not self.bad, "\n".join(self.bad)
        assert self.recorded, "tests/golden/hip_mesh3d_value_forms_measured.json is missing: run this file with SMALFIT_WRITE_MESH3D_VALUE_MEASURED=<path> on a GPU and commit the result"


def test_sampler_far_from_the_origin_against_float64(capsys):
    """the sampler interpolates absolute coordinates: it loses the digits of the offset, as any float32 evaluation does"""
    shim = host_shim.mesh3d()
    p = vf.ribbon_problem(3, lattice=True)
    table = Table()
    for o in (0,) + vf.OFFSETS:
        q = vf.shift(p, o) if o else p
        got = _sample(targets_of(q))
        for n, (tv, tf) in enumerate(q.targets):
            _, chosen = vf.shim_sample(shim, tv, tf, SAMPLES, SEED, ITERATION, n)
            u, v = vf.sampler_uniforms(shim, SAMPLES, SEED, ITERATION, n)
            want = vf.sampler_reference(tv, tf, chosen, u, v)
            yard = vf.sampler_deviation(vf.sampler_reference(tv, tf, chosen, u, v, np.float32), want, 4.0)
            table.add("sampler/o=%d/mesh%d" % (o, n), vf.sampler_deviation(got["points"][n], want, 4.0), yard, vf.SAMPLER_BAR, vf.FLOOR_VALUE)
    table.close(capsys)


# ---- C. coincidence and collapse ---------------------------------------------------------------------------------------------------
def test_points_on_the_vertices_give_a_chamfer_term_of_exactly_zero():
    p = vf.coincident_problem()
    o = run_eval(objective(p), p, vf.ONE_HOT["chamfer"][0])
    assert o["losses"][0] == 0.0 and o["losses"][4] == 0.0
    assert vf.same_bits(o["dverts"], np.zeros_like(o["dverts"])) and vf.same_bits(o["dtrans"], np.zeros_like(o["dtrans"]))


@pytest.mark.parametrize("variant", [v for v in vf.SURFACE_VARIANTS if v[0] not in ("min_cos", "all")], ids=lambda v: v[0])
def test_a_mesh_against_itself_gives_a_surface_term_of_zero(variant):
    name, gates, sigmas = variant
    p = vf.self_target_problem()
    o = run_surface(objective(p), p, targets_of(p), gates, sigmas)
    assert no_nan(o)
    for key in ("losses", "rows", "dverts", "dtrans", "point_residual", "vert_residual"):
        assert not o[key].any(), (name, key)
    if sigmas is not None:
        assert (o["point_weights"] == 1.0).all() and (o["vert_weights"] == 1.0).all()
        assert np.array_equal(o["surface_weight_sums"], [[p.S, p.V]])
    if name == "max_dist":                                         # "dropped when d^2 > tau^2": d = 0 is kept
        assert o["point_kept"].all() and o["vert_kept"].all() and np.array_equal(o["kept"], [[p.S, p.V]])


def check_against_reference(p, o, weights):
    assert no_nan(o) and np.array_equal(o["verts"], p.verts)
    ref = mf.reference(o["verts"], p.points, p.faces, weights)
    for i in range(4):
        if weights[i] > 0:
            assert abs(o["losses"][i] - ref["terms"][i]) <= vf.LOSS_BAR * abs(ref["terms"][i]), (i, o["losses"], ref["terms"])
    assert abs(o["losses"][4] - ref["total"]) <= vf.LOSS_BAR * abs(ref["total"])
    for n in range(p.N):
        assert m3.rel(o["dverts"][n], ref["dverts"][n]) < vf.DVERTS_BAR, n
    assert np.abs(o["dtrans"] - ref["dtrans"]).max() <= 2e-4 * np.abs(ref["dtrans"]).max() + 1e-7
    return ref


@pytest.mark.parametrize("name", sorted(vf.COLLAPSES))
def test_collapsed_fitted_geometry(name):
    p, same, tie_point = vf.collapsed_problem(name)
    obj = objective(p)
    check_against_reference(p, run_eval(obj, p, vf.COLLAPSE_WEIGHTS), vf.COLLAPSE_WEIGHTS)
    # every pair with a zero normal: under the clamp, 1 - cos exactly 1
    pairs = mo.face_pairs(p.faces)
    zero = np.nonzero(mf.normal_pair_products(p.verts, pairs)[0] == 0)[0]
    assert len(zero)
    pair_obj = eng.MeshObjective(4, vf.PAIR_FACES, 1, p.S)
    for z in zero:
        one = vf.Problem("pair", vf.PAIR_FACES, p.verts[:, pairs[z]].copy(), np.zeros((1, 3), np.float32), None, p.points, None, None, None)
        o = run_eval(pair_obj, one, vf.ONE_HOT["normal"][0])
        assert o["losses"][2] == 1.0 and no_nan(o), z
    if name != "face_to_segment":                                  # the designed tie resolves to the lowest index
        t = run_eval(obj, p, mf.TIE_WEIGHTS, dict(max_dist_point=64.0, max_dist_vert=64.0))
        assert t["point_nn"][0, tie_point] == same[0] and t["point_kept"].all()
        low, high = (mf.reference(t["verts"], p.points, p.faces, mf.TIE_WEIGHTS, rule=r) for r in ("low", "high"))
        assert m3.rel(t["dverts"][0, same], low["dverts"][0, same]) < vf.DVERTS_BAR <= m3.rel(t["dverts"][0, same], high["dverts"][0, same])


def test_a_vertex_on_the_mean_of_its_ring_has_unit_zero():
    v, f = vf.zero_ring_mesh()
    p = vf.Problem("fan", f, v[None].copy(), np.zeros((1, 3), np.float32), None, v[None, :2].copy(), None, None, None)
    obj = objective(p)
    w = vf.ONE_HOT["laplacian"][0]
    base = run_eval(obj, p, w)
    check_against_reference(p, base, w)
    for o in vf.OFFSETS:                                           # ... wherever the mesh stands
        got = run_eval(obj, vf.shift(p, o), w)
        for key in ("losses", "dverts", "dtrans"):
            assert vf.same_bits(base[key], got[key]), (o, key)


@pytest.mark.parametrize("name", sorted(vf.PAIR_MESHES))
def test_flat_fold_and_coplanar_pair(name):
    v, want = vf.PAIR_MESHES[name]
    p = vf.Problem(name, vf.PAIR_FACES, v[None].copy(), np.zeros((1, 3), np.float32), None, v[None, :2].copy(), None, None, None)
    o = run_eval(objective(p), p, vf.ONE_HOT["normal"][0])
    assert abs(o["losses"][2] - want) <= vf.PAIR_EPS and no_nan(o)
