"""CPU: the trimmed rigid pre-alignment's host side -- the float64 restatement (tests/rigid_trim_cases.py) and what it buys on a
side scan with a floor (the untrimmed restatement ends more than 1 rad off, the trimmed one recovers R*), the shim's selection
against numpy.lexsort, smalfit_plan.h's refusals in their order, the block's layout against gcc, the grids and launch counts, the
fraction -> count rule at its edges, and the binding.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from smalify_amd import _lib
from smalify_amd import engine as eng
from tests import host_rigid_align as hr
from tests import host_rigid_trim as ht
from tests import rigid_align_cases as rc
from tests import rigid_trim_cases as tc

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "smalfit.h")
EPS32 = float(np.finfo(np.float32).eps)


# ---- the restatement and what trimming buys -------------------------------------------------------------------------------------
def test_full_keeps_restate_the_untrimmed_call():
    c = rc.RECOVERY_CASES["cube5_skew15"]
    x, p = c["x"], c["p"][:100]
    a = tc.align(x, p, len(p), len(x), iterations=3)
    b = rc.align(x, p, None, 3)
    assert np.array_equal(a["R"], b["R"]) and np.array_equal(a["t"], b["t"]) and np.array_equal(a["scores"], b["scores"])


@pytest.mark.parametrize("name", tc.POSES)
def test_partial_case_is_admitted_and_the_untrimmed_call_misses_it(name):
    """the side scan of the lopsided blob (96 of 161 vertices seen) with 40 floor points: the trimmed float64 restatement alone
    recovers R*; the untrimmed one, both ways and with w_vert = 0, ends more than 1 rad off"""
    c = tc.PARTIAL_CASES[name]
    assert c["p"].shape == (136, 3) and c["x"].shape == (161, 3) and (c["keep_point"], c["keep_vert"]) == (87, 77)
    ref = tc.reference(name)
    b = ref["best"]
    angle = rc.rotation_angle(ref["R"][b], c["R"])
    print(name, "trimmed: best", b, "angle", angle, "score", ref["scores"][b])
    assert angle <= rc.RECOVERY_ADMISSION
    assert np.abs(ref["t"][b] - c["t"]).max() <= rc.RECOVERY_ADMISSION * (1.0 + c["extent"])
    assert ref["kept"].sum() == 0
    others = [k for k in range(tc.TRIM_STARTS) if rc.rotation_angle(ref["R"][k], c["R"]) > 1e-3]
    assert ref["scores"][b] <= 1e-12 and others and min(ref["scores"][k] for k in others) > 1e-3
    for variant in ("untrimmed", "untrimmed_points"):
        u = tc.reference(name, variant)
        off = rc.rotation_angle(u["R"][u["best"]], c["R"])
        print(name, variant, "ends", off, "rad off")
        assert off > tc.UNTRIMMED_FLOOR


def test_restated_selection_keeps_the_lowest_index_among_equal_keys():
    d2 = np.array([0.5, 0.0, 0.5, 0.0, 0.25, 0.5])
    assert list(np.flatnonzero(tc.select(d2, 1))) == [1]
    assert list(np.flatnonzero(tc.select(d2, 4))) == [0, 1, 3, 4]
    assert list(np.flatnonzero(tc.select(d2, 5))) == [0, 1, 2, 3, 4]
    assert tc.select(d2, 6).all()


# ---- the shim's selection against numpy.lexsort -----------------------------------------------------------------------------------
def _key_sets(count):
    rs = np.random.RandomState(count)
    straddle = np.sort(rs.rand(count).astype(np.float32))
    lo, hi = count // 3, max(count // 3 + 1, (2 * count) // 3)
    straddle[lo:hi] = straddle[lo]                       # a run of bit-equal d^2 across the middle third
    straddle = straddle[rs.permutation(count)]
    return dict(random=rs.rand(count).astype(np.float32) ** 2, equal=np.full(count, 0.37, np.float32),
                zero=np.zeros(count, np.float32), straddle=straddle)


@pytest.mark.parametrize("count", (1, 64, 65, 161, 1025))
def test_shim_selection_against_lexsort(count):
    for kind, d2 in _key_sets(count).items():
        for keep in sorted({1, 63, 64, 65, count - 1, count}):
            if not 1 <= keep <= count:
                continue
            kept, tbits, tq = ht.select(d2, keep)
            order = np.lexsort((np.arange(count), d2.view(np.uint32)))
            want = np.zeros(count, np.uint8)
            want[order[:keep]] = 1
            assert np.array_equal(kept, want), (kind, count, keep)
            assert tq == order[keep - 1] and tbits == int(d2.view(np.uint32)[tq]), (kind, count, keep)
            assert int(kept.sum()) == keep
    # a query without a match has no key: never kept, and fewer keys than keep keeps them all
    d2 = np.array([0.3, 0.1, 0.2, 0.0], np.float32)
    idx = np.array([5, -1, 2, -1], np.int32)
    kept, tbits, tq = ht.select(d2, 3, idx)
    assert list(kept) == [1, 0, 1, 0] and tq == 0 and tbits == ht.key_bits(0.3)
    kept, tbits, tq = ht.select(d2, 1, idx)
    assert list(kept) == [0, 0, 1, 0] and tq == 2
    kept, tbits, tq = ht.select(d2, 2, np.full(4, -1, np.int32))
    assert not kept.any() and (tbits, tq) == (0, -1)


def test_key_order():
    vals = np.array([0.0, 1e-45, 1e-38, 1e-20, 0.5, 1.0, 3e38], np.float32)
    bits = [ht.key_bits(v) for v in vals]
    assert bits == sorted(bits) and len(set(bits)) == len(bits) and bits[0] == 0
    assert bits == [int(b) for b in vals.view(np.uint32)]
    assert ht.key_kept(5, 9, 6, 0) and ht.key_kept(6, 3, 6, 3) and not ht.key_kept(6, 4, 6, 3) and not ht.key_kept(7, 0, 6, 3)
    assert not ht.key_kept(0, 0, 0, -1)


def test_one_trimmed_float32_iteration_is_the_definition():
    c = tc.PARTIAL_CASES["cube5_skew15"]
    x, p = c["x"], c["p"]
    R0, t0 = rc.start_transform(rc.cube_rotations()[5], x.astype(np.float64), p.astype(np.float64))
    T0 = np.concatenate([R0, t0[:, None]], 1).astype(np.float32)
    o = ht.iterate(x, p, T0, c["keep_point"], c["keep_vert"])
    x64, p64 = x.astype(np.float64), p.astype(np.float64)
    R64, t64, cost64, kept64 = tc.iterate(x64, p64, T0[:, :3].astype(np.float64), T0[:, 3].astype(np.float64), 1.0, 1.0, c["keep_point"],
                                          c["keep_vert"])
    assert o["kept"] == kept64 == 0
    assert int(o["kept_v"].sum()) == c["keep_vert"] and int(o["kept_p"].sum()) == c["keep_point"]
    assert abs(float(o["cost"]) - cost64) <= 64 * EPS32 * cost64
    Tn = o["T"].reshape(3, 4)
    assert rc.rotation_angle(Tn[:, :3], R64) <= 1e-5 and np.abs(Tn[:, 3] - t64).max() <= 1e-5
    # full keeps: the untrimmed shim's iteration, bit for bit
    full = ht.iterate(x, p, T0, len(p), len(x))
    plain = hr.iterate(x, p, T0)
    assert np.array_equal(full["T"], plain["T"]) and full["cost"] == plain["cost"] and full["kept_v"].all() and full["kept_p"].all()
    # a skipped direction: no mask, threshold 0
    one = ht.iterate(x, p, T0, c["keep_point"], 1, w_vert=0.0)
    assert np.all(one["kept_v"] == 255) and one["trim_d2"][0] == 0.0 and one["trim_d2"][1] > 0.0


# ---- the rules ------------------------------------------------------------------------------------------------------------------
def test_every_refusal_in_its_order():
    t = _lib.RigidTrimArgs()
    t.keep_vert, t.keep_point = 50, 45
    assert ht.refusal(t) is None and ht.trim_on(t)
    t.struct_size += 4
    t.keep_vert, t.keep_point = 0, 91
    steps = [
        ("smalfit_rigid_trim_args.struct_size does not match", lambda: setattr(t, "struct_size", C.sizeof(_lib.RigidTrimArgs))),
        ("keep_vert must be 1 .. num_verts", lambda: setattr(t, "keep_vert", 100)),
        ("keep_point must be 1 .. num_points", lambda: setattr(t, "keep_point", 90)),
    ]
    for text, mend in steps:
        msg = ht.refusal(t)
        assert msg is not None and text in msg, (text, msg)
        mend()
    assert ht.refusal(t) is None
    assert not ht.trim_on(t) and not ht.trim_on(None)           # both keeps at their counts: off
    t.keep_vert = 101
    assert ht.refusal(t) == "keep_vert must be 1 .. num_verts"
    # a keep of a direction of weight 0 is accepted and ignored
    assert ht.refusal(t, vert_dir=False) is None and not ht.trim_on(t, vert_dir=False)
    t.keep_vert, t.keep_point = 100, -3
    assert ht.refusal(t) == "keep_point must be 1 .. num_points"
    assert ht.refusal(t, point_dir=False) is None and not ht.trim_on(t, point_dir=False)
    t.keep_vert, t.keep_point = 99, 90
    assert ht.trim_on(t) and not ht.trim_on(t, vert_dir=False)
    t.keep_vert, t.keep_point = 1, 1
    assert ht.refusal(t, V=1, S=1) is None and not ht.trim_on(t, V=1, S=1)


def test_grids_and_launches():
    g = ht.grids(True, True, 24, 1, 30)
    assert g["trim"] == (2, 24, 1)
    # the init, I + 1 rounds of (two scans, the selection, the solve), the pick: one launch a round more than untrimmed
    assert g["launches"] == 1 + 31 * 4 + 1 and g["untrimmed_launches"] == 1 + 31 * 3 + 1
    g = ht.grids(False, True, 3, 70, 0)
    assert g["trim"] == (1, 3, 70) and g["launches"] == 1 + 3 + 1
    g = ht.grids(True, False, 64, 32, 5)
    assert g["trim"] == (1, 64, 32) and g["launches"] == 1 + 6 * 3 + 1


def test_fraction_to_count_rule_at_its_edges():
    for count in (1, 3, 136, 161, 3000, 3889):
        assert ht.keep_count(1.0, count) == eng.keep_count(1.0, count) == count
        assert ht.keep_count(1e-300, count) == eng.keep_count(1e-300, count) == 1
        for k in sorted({1, count // 3, count // 2, count - 1} - {0}):
            exact = k / count
            above = float(np.nextafter(exact, 2.0))              # one double ulp above k / count
            for f in (exact, above, float(np.nextafter(exact, 0.0))):
                want = int(min(count, max(1, np.ceil(np.float64(f) * np.float64(count)))))
                assert ht.keep_count(f, count) == eng.keep_count(f, count) == want, (count, k, f)
            if k < count and above * count > k:
                assert ht.keep_count(above, count) == k + 1, (count, k)
    assert ht.keep_count(87 / 136, 136) in (87, 88) and ht.keep_count(0.5, 161) == 81
    assert 1 <= ht.keep_count(0.6, 3000) <= 3000


# ---- the block, the binding, the header -----------------------------------------------------------------------------------------
def test_struct_layout_matches_the_header(tmp_path):
    cls = _lib.RigidTrimArgs
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "smalfit.h"', "int main(void) {",
             'printf("sizeof %zu\\n", sizeof(smalfit_rigid_trim_args));']
    for field, _ in cls._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(smalfit_rigid_trim_args, %s));' % (field, field))
    lines += ["return 0; }"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = {a: int(b) for a, b in (ln.split() for ln in out.strip().splitlines())}
    assert got["sizeof"] == C.sizeof(cls) == ht.sizeof_args()
    assert [got[f] for f, _ in cls._fields_] == [getattr(cls, f).offset for f, _ in cls._fields_] == ht.offsets()
    assert _lib.RigidTrimArgs().struct_size == C.sizeof(cls)
    # the untrimmed block is what it was
    assert C.sizeof(_lib.RigidAlignArgs) == hr.sizeof_args()


def test_entry_point_is_bound_lazily_under_abi_version_6():
    text = open(HEADER).read()
    name = "smalfit_trimmed_rigid_align"
    assert _lib.ABI_VERSION == 6 and re.search(r"#define SMALFIT_ABI_VERSION 6\b", text)
    assert name in _lib.SIGNATURES and name in _lib.LAZY_SYMBOLS
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int and args[2]._type_ is _lib.RigidAlignArgs and args[3]._type_ is _lib.RigidTrimArgs
    assert _lib.SIGNATURES["smalfit_rigid_align"] == (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(_lib.RigidAlignArgs)])
    declared = set(re.findall(r"\b(smalfit_[a-z_0-9]+)\s*\(", text))
    # the untrimmed call's three entry points are still exactly three under their prefix; the trimmed call stands beside them
    assert name in declared and not name.startswith("smalfit_rigid_")
    assert {n for n in declared if n.startswith("smalfit_rigid_")} == {
        "smalfit_rigid_aligner_create", "smalfit_rigid_aligner_destroy", "smalfit_rigid_align"}
    assert "trimming or robust weights" not in text           # f14's "Not here" line no longer lists trimming
    lib_path = _lib.LIB_PATH
    if os.path.exists(lib_path):
        out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
        assert re.search(r" T %s$" % name, out, re.M)


def test_python_fractions_are_checked_before_anything_else():
    class NoHandle(eng.RigidAligner):
        def __init__(self):
            pass
    al = NoHandle()
    for bad in (0.0, -0.1, 1.0000001, float("nan"), float("inf")):
        with pytest.raises(eng.SmalfitError, match="trim_point must be in \\(0, 1\\]"):
            al.align(None, None, trim_point=bad)
        with pytest.raises(eng.SmalfitError, match="trim_vert must be in \\(0, 1\\]"):
            al.align(None, None, trim_vert=bad)


# ---- the stand-in model's partial target ------------------------------------------------------------------------------------------
def test_model_cut_is_admitted():
    """the cut tests/test_gpu_rigid_trim.py uses on the stand-in model: the float64 restatement on the oracle's vertices for the
    fitter's parameters and on points drawn on the cut target (numpy's draw here, the device sampler's there) lands within
    MODEL_ADMISSION of R*, and every start that ends elsewhere scores worse"""
    import torch
    from oracle import smal_oracle as so
    from smalify_amd import synthetic
    md = synthetic.synthetic_model(seed=0, shape_family_id=-1)
    g, j, b = tc.model_parameters()
    theta = np.concatenate([g[:, None, :], j], 1)
    v = so.smal_forward(so.OracleModel(md), torch.from_numpy(b), torch.from_numpy(theta), torch.zeros(1, 6, dtype=torch.float64))[0].numpy()[0]
    tv, tf, seen = tc.partial_target(v, md.faces)
    assert 0.6 < seen.mean() < 0.8
    p = tc.draw_points(tv, tf, tc.MODEL_POINTS, seed=0)
    V = len(v)
    r = tc.align(v.astype(np.float32), p, eng.keep_count(tc.MODEL_TRIM_POINT, tc.MODEL_POINTS), eng.keep_count(tc.MODEL_TRIM_VERT, V),
                 nearest=tc.nearest_tree)
    angles = [rc.rotation_angle(r["R"][k], tc.MODEL_TURN) for k in range(24)]
    best = r["best"]
    others = [r["scores"][k] for k in range(24) if angles[k] > 0.3]
    print("model cut: angle", angles[best], "score", r["scores"][best], "next distinct", min(others))
    assert angles[best] <= tc.MODEL_ADMISSION
    assert others and min(others) > 1.5 * r["scores"][best]
