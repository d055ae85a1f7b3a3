"""Every engine entry point after every other on ONE engine (-m gpu): the acts of tests/entry_order_cases.py.

The engine is built on state one call leaves for the next -- the per-pixel depth bounds, accumulators "cleared by whoever reads
them last", queue and arrival counters, candidate lists, the staging slots of the folded loop, a projection workspace several
entry points borrow, the graph replay key, options and joint limits -- and different entry points run different subsets of the
chain that is meant to leave it clean.

  a  fresh     every act twice, each time on a brand-new engine: bit for bit (the act is reproducible); one result is fresh[B]
  b  reset     for every B, on one long-lived engine shared by the module: for every A in table order, A, reset_raster_cache(), B;
               B == fresh[B] byte for byte on every output, status() included
  c  foreign   for the B that are single evaluations or renders, A then B with NO reset: the depth bounds B finds are those of
     cache     another image (scenes X and Y overlap with an IoU of 0.14 .. 0.18).  Silhouettes within SIL_TOL = 2e-4 per pixel of
               the float64 oracle's render of the vertices B rendered; the sum of the nine loss terms within 2e-6 relative and every
               gradient tensor within 2e-5 rel-L2 of fresh[B] (the bars of test_raster_cache_never_changes_results); rows of
               per-frame / per-window tables within the same absolute budgets (2e-6 x the total, 2e-5 x the norm of the whole
               gradient: a row is a partial sum of the same pixels); integer outputs, the projections and the vertices equal exactly
  d  walk      150 acts drawn with RandomState(5) on one engine, a reset with probability 1/2 before each: (b) or (c) accordingly
  e  two       two engines over one DeviceModel take the acts alternately on one stream: each equals fresh[B]

tests/golden/hip_entry_order_measured.json records the largest foreign-cache deviation per B (written under
SMALFIT_WRITE_ENTRY_ORDER_MEASURED=<path>); with the file present a deviation also stays within RATCHET = 3 x its recorded value
(or the floor: a tenth of the bar, below which it is float32 noise whose draw changes with any reordering of a sum)."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import entry_order_cases as oc      # noqa: E402
from tests import parity_cases as pc           # noqa: E402

SIL_TOL = 2e-4
LOSS_TOL = 2e-6
GRAD_TOL = 2e-5
RATCHET = 3.0
MEASURED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hip_entry_order_measured.json")
WALK_LENGTH = 150

_FRESH = {}
_SHARED = {}
_ORACLE_SIL = {}
_MEASURED = {}


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """a device error ends the session: nothing more is started on a GPU that has just faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:
        pytest.exit("device error, stopping: %s" % exc, returncode=3)


def _differing(a, b):
    """the first key whose bytes differ (or that only one has), or None"""
    if set(a) != set(b):
        return "keys %s" % sorted(set(a) ^ set(b))
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            return k
    return None


def _describe(a, b, k):
    if k is None or k.startswith("keys") or a[k].shape != b[k].shape:
        return str(k)
    x, y = a[k].astype(np.float64).ravel(), b[k].astype(np.float64).ravel()
    bad = np.flatnonzero(~((x == y) | (np.isnan(x) & np.isnan(y))))
    return "%s: %d of %d differ, first at %d: %r != %r, largest |difference| %.3e" % (
        k, len(bad), x.size, bad[0] if len(bad) else -1, x[bad[0]] if len(bad) else None, y[bad[0]] if len(bad) else None,
        float(np.nanmax(np.abs(x - y))))


def _fresh(name):
    """the result of act `name` on a brand-new engine (made twice, on two engines: the act itself is reproducible)"""
    if name not in _FRESH:
        results = []
        for _ in range(2):
            e = oc.new_engine()
            results.append(oc.ACTS[name].fn(e))
            del e
        k = _differing(results[0], results[1])
        assert k is None, "act %r is not reproducible on fresh engines: %s" % (name, _describe(results[0], results[1], k))
        _FRESH[name] = results[0]
    return _FRESH[name]


def _shared_engine():
    """the module's one long-lived engine and the history of the acts it ran"""
    if not _SHARED:
        _SHARED["engine"], _SHARED["history"] = oc.new_engine(), []
    return _SHARED["engine"], _SHARED["history"]


def _run(e, history, name, reset):
    if reset:
        e.reset_raster_cache()
    history.append(("reset + " if reset else "") + name)
    return oc.ACTS[name].fn(e)


def _assert_fresh_bits(got, name, after, history):
    k = _differing(got, _fresh(name))
    assert k is None, "%r after %r and a reset differs from a fresh engine's: %s\nlast acts: %s" % (
        name, after, _describe(got, _fresh(name), k), history[-5:])


def _oracle_sil(verts):
    """the float64 oracle's silhouettes of these float32 vertices (computed once per set of vertices)"""
    from oracle import smal_oracle as so
    key = hashlib.sha256(np.ascontiguousarray(verts).tobytes()).hexdigest()
    if key not in _ORACLE_SIL:
        _, om = pc.get_oracle_model()
        with torch.no_grad():
            _ORACLE_SIL[key] = so.soft_silhouette(torch.from_numpy(verts).double(), om.faces, oc.S).numpy()
    return _ORACLE_SIL[key]


def _rel(a, b, norm=None):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b) if norm is None else norm, 1e-30))


EXACT = ("proj_out", "verts_out", "verts_in", "proj", "status", "refused")


def _foreign_cache_deviations(got, name):
    """-> ({quantity: deviation}, [keys that had to be equal exactly and are not]) of act `name` run on a foreign cache"""
    ref = _fresh(name)
    assert set(got) == set(ref), (name, sorted(set(got) ^ set(ref)))
    dev, unequal = {}, []
    total = float(ref["losses"].astype(np.float64).sum()) if "losses" in ref else None
    gnorm = float(np.sqrt(sum(np.sum(ref[k].astype(np.float64) ** 2) for k in ref if k.startswith("g_"))))
    for k in ref:
        if k == "face_list_lengths":
            continue                                # diagnostics: the form of a list may follow the bounds, results never do
        if k in ("sil_out", "sil"):
            orc = _oracle_sil(ref["verts_out" if k == "sil_out" else "verts_in"])
            dev["sil"] = float(np.abs(got[k].astype(np.float64) - orc).max())
            dev["sil_fresh"] = float(np.abs(ref[k].astype(np.float64) - orc).max())
        elif k == "losses":
            dev["loss"] = abs(float(got[k].astype(np.float64).sum()) - total) / abs(total)
        elif k in ("losses_per_frame", "window_losses"):
            rows = np.abs(got[k].astype(np.float64).sum(1) - ref[k].astype(np.float64).sum(1)).max()
            dev["loss_rows"] = float(rows) / abs(total)
        elif k.startswith("window_g_"):
            dev["grad_rows"] = max(dev.get("grad_rows", 0.0), _rel(got[k], ref[k], norm=gnorm))
        elif k.startswith("g_"):
            dev["grad"] = max(dev.get("grad", 0.0), _rel(got[k], ref[k]))
        elif k in EXACT or not np.issubdtype(ref[k].dtype, np.floating):
            if got[k].tobytes() != ref[k].tobytes():
                unequal.append(k)
        else:
            raise AssertionError("no rule for output %r of act %r" % (k, name))
    return dev, unequal


BARS = {"sil": SIL_TOL, "loss": LOSS_TOL, "loss_rows": LOSS_TOL, "grad": GRAD_TOL, "grad_rows": GRAD_TOL}


def _assert_foreign_cache(got, name, after, history, record=True):
    """record: the pair belongs to (c)'s table -- its deviations are recorded and held to the ratchet"""
    dev, unequal = _foreign_cache_deviations(got, name)
    recorded = json.load(open(MEASURED)) if record and os.path.exists(MEASURED) else {}
    bad = ["%s must be equal exactly" % k for k in unequal]
    for q, bar in BARS.items():
        if q not in dev:
            continue
        key = "%s/%s" % (name, q)
        if record:
            _MEASURED[key] = max(_MEASURED.get(key, 0.0), dev[q])
        if not dev[q] <= bar:
            bad.append("%s %.3e exceeds %.1e%s" % (q, dev[q], bar, " (a fresh render: %.3e)" % dev["sil_fresh"] if q == "sil" else ""))
        elif key in recorded and dev[q] > max(RATCHET * recorded[key], 0.1 * bar):
            bad.append("%s %.3e is more than %.0f x the recorded %.3e" % (q, dev[q], RATCHET, recorded[key]))
    assert not bad, "%r after %r without a reset: %s\nlast acts: %s" % (name, after, "; ".join(bad), history[-5:])
    return dev


# ---- a ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", oc.NAMES)
def test_a_fresh_engines_agree(name):
    r = _fresh(name)
    assert r["status"][0] == 0, (name, r["status"])
    if oc.ACTS[name].kind == "refusal":
        assert r["refused"][0] == 1
        for k, v in r.items():                      # nothing was launched: every output buffer still holds the sentinel
            if v.dtype == np.float32:
                assert (v == np.float32(oc.SENTINEL)).all(), (name, k)
    else:
        for k, v in r.items():                      # ... and an act that ran wrote every float it hands out
            if v.dtype == np.float32:
                assert not (v == np.float32(oc.SENTINEL)).any(), (name, k)
    if name == "render Y3" or name == "eval Y8":
        assert (r["face_list_lengths"] > 0).any()


def test_a_the_acts_reach_what_the_table_says():
    """the acts reach what the table says they reach: the optimiser moved, the limit term and the option changed a result"""
    assert not np.array_equal(_fresh("run 3")["flat"], _fresh("run 1")["flat"])
    assert not np.array_equal(_fresh("run 4")["flat"], _fresh("run 3")["flat"])
    assert np.count_nonzero(_fresh("run graph")["exp_avg"]) > _fresh("run graph")["exp_avg"].size // 2
    assert _differing(_fresh("run graph"), _fresh("run 3")) is None             # the replay ends in the folded loop's bits
    assert _fresh("joint limits")["losses"][8] > 0 and _fresh("eval X4")["losses"][8] == 0
    assert not np.array_equal(_fresh("option unclamped")["g_trans"], _fresh("eval X4")["g_trans"])
    assert np.array_equal(_fresh("option unclamped")["sil_out"], _fresh("eval X4")["sil_out"])
    assert np.array_equal(_fresh("eval u8")["losses"], _fresh("eval X4")["losses"])
    assert _fresh("eval stage 0")["losses"][4] == 0 and _fresh("eval X4")["losses"][4] > 0
    assert _fresh("fit metrics")["sil_counts"].min() > 0


# ---- b ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", oc.NAMES)
def test_b_after_any_act_and_a_reset_the_bits_are_a_fresh_engines(name):
    e, history = _shared_engine()
    _fresh(name)
    for after in oc.NAMES:
        _run(e, history, after, reset=False)
        _assert_fresh_bits(_run(e, history, name, reset=True), name, after, history)


# ---- c ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", oc.CACHED)
def test_c_a_foreign_depth_cache_never_changes_results(name, capsys):
    e, history = _shared_engine()
    _fresh(name)
    worst = {}
    for after in oc.NAMES:
        _run(e, history, after, reset=False)
        dev = _assert_foreign_cache(_run(e, history, name, reset=False), name, after, history)
        for q, v in dev.items():
            if v >= worst.get(q, (-1.0, ""))[0]:
                worst[q] = (v, after)
    with capsys.disabled():
        print("\n[foreign cache %-24s %s]" % (name, "  ".join("%s %.2e (after %s)" % (q, v, a) for q, (v, a) in sorted(worst.items()))))


def test_c_measured_values_are_recorded():
    """the record of (c): written on request, and complete"""
    if not _MEASURED:
        for name in oc.CACHED:                      # this test alone: one foreign act in front of every B
            e, history = _shared_engine()
            _run(e, history, "eval Y8" if name != "eval Y8" else "eval X4", reset=False)
            _assert_foreign_cache(_run(e, history, name, reset=False), name, history[-2], history)
    path = os.environ.get("SMALFIT_WRITE_ENTRY_ORDER_MEASURED")
    if path:
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc.update(_MEASURED)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        json.dump(doc, open(path, "w"), indent=1, sort_keys=True)
    assert os.path.exists(MEASURED), ("tests/golden/hip_entry_order_measured.json is missing: run this file with "
                                      "SMALFIT_WRITE_ENTRY_ORDER_MEASURED=<path> on a GPU box and commit the result")
    recorded = json.load(open(MEASURED))
    missing = [k for k in _MEASURED if k not in recorded]
    assert not missing, "not in tests/golden/hip_entry_order_measured.json: %s" % missing


# ---- d ---------------------------------------------------------------------------------------------------------------------------
def test_d_a_seeded_walk():
    rs = np.random.RandomState(5)
    e, history = oc.new_engine(), []
    for step in range(WALK_LENGTH):
        name = oc.NAMES[rs.randint(len(oc.NAMES))]
        reset = bool(rs.rand() < 0.5)
        after = history[-1] if history else "nothing"
        got = _run(e, history, name, reset)
        try:
            if reset:
                _assert_fresh_bits(got, name, after, history)
            elif name in oc.CACHED or oc.ACTS[name].kind == "setting":
                _assert_foreign_cache(got, name, after, history, record=False)
            elif oc.ACTS[name].kind != "run":       # no silhouette, or a refusal: nothing of it may depend on the cache
                _assert_fresh_bits(got, name, after, history)
            else:                                   # a run on stale bounds: float noise compounds through Adam
                assert got["status"][0] == 0 and np.isfinite(got["flat"]).all()
        except AssertionError:
            print("the walk up to step %d:\n  %s" % (step, "\n  ".join(history)))
            raise


# ---- e ---------------------------------------------------------------------------------------------------------------------------
def test_e_two_engines_interleaved_share_nothing():
    dm = pc.get_model()[2]
    e1, e2 = oc.new_engine(dm), oc.new_engine(dm)
    h1, h2 = [], []
    n = len(oc.NAMES)
    for i, name in enumerate(oc.NAMES):
        other = oc.NAMES[(n - 1 - i + n // 2) % n]  # the second engine goes through the table from elsewhere, backwards
        a = _run(e1, h1, name, reset=True)
        b = _run(e2, h2, other, reset=True)
        _assert_fresh_bits(a, name, "%r on the other engine" % (h2[-2] if len(h2) > 1 else "nothing"), h1)
        _assert_fresh_bits(b, other, "%r on the other engine" % name, h2)
