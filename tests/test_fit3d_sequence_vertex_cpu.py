"""The temporal terms on posed vertices without a GPU (include/smalfit.h, "scan sequences", the vertex terms):
fit3d_sequence_vertex_math.h and smalfit_plan.h through the host shim against a float64 restatement and against torch autograd, the
dyadic case bit for bit, clip boundaries, uniform motion, short clips, every refusal in its order, the plan and the grid, the struct
layout, the header's rules, the Python surface, and why the terms exist: a pose a full turn away in axis-angle."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from smalify_amd import _lib, engine as eng
from tests import host_sequence_vertex as hv
from tests import sequence_vertex_cases as vc

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "smalfit.h")
NEW_EXPORTS = ("smalfit_scan_sequence_vertex_term", "smalfit_scan_sequence_vertex_step")


# ---- the arithmetic ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", vc.VERTS)
@pytest.mark.parametrize("clips", vc.CLIPS, ids=vc.clip_id)
def test_shim_matches_both_restatements(clips, V):
    bar = vc.bars()
    x = vc.verts(clips, V)
    for weights in vc.WEIGHT_SETS:
        got = hv.term(clips, x, weights)
        for name, ref in (("float64", vc.reference64(clips, x, weights)), ("autograd", vc.reference_torch(clips, x, weights))):
            w = vc.worst([(got, ref)])
            print(clips, V, weights, name, w)
            assert w["grad"] <= bar["grad"] and w["dtrans"] <= bar["dtrans"] and w["loss"] <= bar["loss"], (name, weights, w)
        assert (got["losses"][0] > 0) == (weights[0] > 0 and max(clips) >= 2)
        assert (got["losses"][1] > 0) == (weights[1] > 0 and max(clips) >= 3)


def test_the_bar_is_three_times_the_float32_restatement():
    shim = vc.worst((hv.term(c, vc.verts(c, V), w), vc.reference64(c, vc.verts(c, V), w)) for c, V, w in vc.all_cases())
    print("host shim against float64:", shim)
    vc.record_float32_restatement(shim)                 # (only with SMALFIT_WRITE_SEQUENCE_VERTEX_MEASURED set)
    m = vc.measured()
    rec = m["float32_restatement_deviation"]
    assert m["ratchet"] == vc.RATCHET == 3.0
    for k in ("loss", "dtrans", "grad"):
        assert m["bar"][k] == pytest.approx(3.0 * rec[k], rel=1e-12), k
    now = vc.float32_restatement_deviation()
    print("float32 torch restatement against float64 now:", now, "recorded:", rec)
    for k in ("loss", "dtrans", "grad"):
        assert 0 < now[k] <= vc.bars()[k], k


@pytest.mark.parametrize("V", vc.DYADIC_VERTS)
def test_dyadic_case_equals_the_closed_form_bit_for_bit(V):
    want = vc.dyadic_closed_form(V)
    got = hv.term(vc.DYADIC_CLIPS, vc.dyadic_verts(V), vc.dyadic_weights(V))
    for k in ("dverts", "dtrans", "losses"):
        assert np.array_equal(vc.bits(got[k]), vc.bits(want[k])), k
    assert want["losses"].all() and want["dverts"][1:].any() and not want["dverts"][0].any()      # mesh 0 is alone in its clip
    for i, only in enumerate(((1, 0), (0, 1))):                                  # each term alone: an absent part contributes nothing
        w = tuple(a * b for a, b in zip(vc.dyadic_weights(V), only))
        one, ref = hv.term(vc.DYADIC_CLIPS, vc.dyadic_verts(V), w), vc.dyadic_closed_form(V, weights=w)
        for k in ("dverts", "dtrans", "losses"):
            assert np.array_equal(vc.bits(one[k]), vc.bits(ref[k])), (only, k)
        assert one["losses"][1 - i] == 0 and vc.bits(one["losses"][2]) == vc.bits(one["losses"][i])


def test_no_gradient_crosses_a_clip_boundary():
    clips, V = (2, 5, 2), 7
    x = vc.verts(clips, V)
    base = hv.term(clips, x, vc.WEIGHTS)
    moved = x.copy()
    moved[4] += np.float32(0.25)                                                  # the middle mesh of the middle clip
    got = hv.term(clips, moved, vc.WEIGHTS)
    for k in ("dverts", "dtrans"):
        for n in (0, 1, 7, 8):                                                   # the other clips keep their bits
            assert np.array_equal(vc.bits(got[k][n]), vc.bits(base[k][n])), (k, n)
        for n in (2, 3, 4, 5, 6):                                                # the five-frame stencil reaches both ends of the clip
            assert not np.array_equal(vc.bits(got[k][n]), vc.bits(base[k][n])), (k, n)
    only_vel = (vc.WEIGHTS[0], 0.0)
    a, b = hv.term(clips, x, only_vel), hv.term(clips, moved, only_vel)
    for n in range(9):                                                           # the velocity stencil reaches one neighbour
        assert np.array_equal(vc.bits(a["dverts"][n]), vc.bits(b["dverts"][n])) == (n not in (3, 4, 5)), n


@pytest.mark.parametrize("clips", [(5,), (3, 4)], ids=vc.clip_id)
def test_uniform_motion_has_no_acceleration(clips):
    x = vc.uniform_motion(clips, 9)
    acc = hv.term(clips, x, (0.0, 1.9))
    assert not acc["losses"].any() and not acc["dverts"].any() and not acc["dtrans"].any()      # exactly 0
    vel = hv.term(clips, x, (0.7, 0.0))
    assert vel["losses"][0] > 0 and vel["dverts"].any()
    both = hv.term(clips, x, (0.7, 1.9))
    assert vc.bits(both["losses"][2]) == vc.bits(vel["losses"][0]) and both["losses"][1] == 0


@pytest.mark.parametrize("clips", [(1,), (2,), (1, 2, 1), (2, 2)], ids=vc.clip_id)
def test_short_clips_leave_the_acceleration_term_zero(clips):
    x = vc.verts(clips, 6)
    acc = hv.term(clips, x, (0.0, 1.9))
    assert not acc["losses"].any() and not acc["dverts"].any() and not acc["dtrans"].any()
    both, vel = hv.term(clips, x, vc.WEIGHTS), hv.term(clips, x, (vc.WEIGHTS[0], 0.0))
    for k in ("dverts", "dtrans", "losses"):
        assert np.array_equal(vc.bits(both[k]), vc.bits(vel[k])), k


def test_outputs_are_optional_and_the_total_form():
    clips, x = (4,), vc.verts((4,), 5)
    full = hv.term(clips, x, vc.WEIGHTS)
    for dv, dt in ((False, True), (True, False), (False, False)):
        part = hv.term(clips, x, vc.WEIGHTS, want_dverts=dv, want_dtrans=dt)
        assert np.array_equal(vc.bits(part["losses"]), vc.bits(full["losses"]))
        assert (part["dverts"] is None) == (not dv) and (part["dtrans"] is None) == (not dt)
        assert dv is False or np.array_equal(vc.bits(part["dverts"]), vc.bits(full["dverts"]))
        assert dt is False or np.array_equal(vc.bits(part["dtrans"]), vc.bits(full["dtrans"]))
    f = np.float32
    base, par, ver = f(1.37), f(0.21), f(0.043)
    assert vc.bits(hv.step_total(base, par, ver)) == vc.bits(f(f(base + par) + ver))


# ---- refusals, the plan, the grid ---------------------------------------------------------------------------------------------------
def test_every_refusal_text_in_order():
    losses, total = np.zeros(3, np.float32), np.zeros(1, np.float32)
    nan, inf = float("nan"), float("inf")
    wrong = dict(step=False, num_verts=0, verts=False, handle_meshes=3)
    assert hv.refusal(hv.block((0.5, 0.5), losses.ctypes.data)) is None
    assert hv.refusal(hv.block((0.5, 0.5), losses.ctypes.data, total.ctypes.data)) is None
    assert hv.refusal(hv.block((-1.0, 0.0), losses.ctypes.data)) is None                       # a weight <= 0 is "skipped", not refused
    # every defect at once, then one repaired after the other: the order of the list in smalfit_plan.h
    assert hv.refusal(None, **wrong) == "the vertex block is NULL"
    assert hv.refusal(hv.block((nan, inf), None, total.ctypes.data), **wrong) == "losses is NULL"
    assert hv.refusal(hv.block((nan, inf), losses.ctypes.data, total.ctypes.data), **wrong) == "w_temp_vert_vel is not finite"
    assert hv.refusal(hv.block((0.5, inf), losses.ctypes.data, total.ctypes.data), **wrong) == "w_temp_vert_acc is not finite"
    assert hv.refusal(hv.block((0.5, 0.5), losses.ctypes.data, total.ctypes.data), **wrong) == "step_total given outside a step"
    assert hv.refusal(hv.block((0.5, 0.5), losses.ctypes.data), **wrong) == "num_verts must be positive"
    wrong["num_verts"] = 1
    assert hv.refusal(hv.block((0.5, 0.5), losses.ctypes.data), **wrong) == "verts is NULL"
    wrong["verts"] = True
    assert hv.refusal(hv.block((0.5, 0.5), losses.ctypes.data), **wrong) == "the sequence handle was built for another num_meshes"
    wrong["handle_meshes"] = 4
    assert hv.refusal(hv.block((0.5, 0.5), losses.ctypes.data), **wrong) is None
    for i, name in enumerate(hv.WEIGHT_KEYS):
        for bad in (nan, inf, -inf):
            w = [0.5, 0.5]
            w[i] = bad
            assert hv.refusal(hv.block(w, losses.ctypes.data)) == name + " is not finite"
    assert hv.refusal(hv.block((0.5, 0.5), losses.ctypes.data), num_verts=-3) == "num_verts must be positive"


def test_plan_launches_nothing_when_no_term_applies_and_the_grid():
    off = dict(launch=False, vel=False, acc=False, grid=(0, 0), partials=0)
    both = hv.block((0.5, 2.0))
    assert hv.plan(None) == off
    assert hv.plan(hv.block((0.0, 0.0))) == off
    assert hv.plan(hv.block((-1.0, 0.0))) == off
    assert hv.plan(both, longest=1) == off                                                  # every clip of length 1
    assert hv.plan(hv.block((0.0, 2.0)), longest=2) == off                                  # no clip holds a triple
    p = hv.plan(both, longest=2, num_verts=3889, num_meshes=32)
    assert p == dict(launch=True, vel=True, acc=False, grid=(16, 32), partials=5 * 32 * 16)
    p = hv.plan(hv.block((0.0, 2.0)), longest=3, num_verts=256, num_meshes=3)
    assert p == dict(launch=True, vel=False, acc=True, grid=(1, 3), partials=15)
    for V, blocks in ((1, 1), (255, 1), (256, 1), (257, 2), (512, 2), (513, 3)):
        assert hv.plan(both, longest=5, num_verts=V, num_meshes=7)["grid"] == (blocks, 7), V


# ---- the header and the binding --------------------------------------------------------------------------------------------------
def test_struct_layout_matches_the_header_and_the_shim(tmp_path):
    cls, cname = _lib.SequenceVertexArgs, "smalfit_sequence_vertex_args"
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "smalfit.h"', "int main(void) {",
             'printf("sizeof %%zu\\n", sizeof(%s));' % cname, 'printf("sequence %zu\\n", sizeof(smalfit_sequence_args));']
    lines += ['printf("%s %%zu\\n", offsetof(%s, %s));' % (f, cname, f) for f, _ in cls._fields_]
    lines += ["return 0; }"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)     # the header compiles as C
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines())
    assert int(got["sizeof"]) == C.sizeof(cls) == hv.sizeof_args() == 24
    assert [int(got[f]) for f, _ in cls._fields_] == [getattr(cls, f).offset for f, _ in cls._fields_] == hv.offsets() == [0, 4, 8, 16]
    assert int(got["sequence"]) == C.sizeof(_lib.SequenceArgs) == hv.sizeof_sequence_args() == 32      # the sequence block keeps its layout


def test_header_rules_for_the_new_exports():
    text = open(HEADER).read()
    assert re.search(r"#define SMALFIT_ABI_VERSION 6\b", text) and _lib.ABI_VERSION == 6
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in NEW_EXPORTS:
        assert name in _lib.SIGNATURES and name in _lib.LAZY_SYMBOLS, name
        # the sequence handle is the FIRST argument: the entry-order matrix keys on engine / objective handles in that place
        assert re.search(r"\b%s\s*\(\s*smalfit_scan_sequence\s*\*" % name, code), name
    declared = set(re.findall(r"\b(smalfit_[a-z_0-9]+)\s*\(", text))
    assert set(NEW_EXPORTS) <= declared and declared == set(_lib.SIGNATURES)
    comment = text[text.index("scan sequences: one shape per clip"):text.index("typedef struct smalfit_scan_sequence ")]
    assert "VERTEX TERMS" in comment
    not_here = comment[comment.rindex("Not here:"):]
    assert "a temporal term on posed vertices" not in not_here and "acceleration" not in not_here


# ---- Python ------------------------------------------------------------------------------------------------------------------------
def test_binding_helpers():
    assert eng.temporal_vertex_weights() == dict(w_temp_vert_vel=0.0, w_temp_vert_acc=0.0)
    assert eng.temporal_vertex_weights(dict(w_temp_vert_acc=2))["w_temp_vert_acc"] == 2.0
    with pytest.raises(KeyError, match="unknown temporal vertex weight"):
        eng.temporal_vertex_weights(dict(w_temp_joint=1.0))
    assert eng.temporal_weights() == dict(w_temp_joint=0.0, w_temp_global=0.0, w_temp_trans=0.0)      # stays as it is
    with pytest.raises(KeyError):
        eng.temporal_weights(dict(w_temp_vert_vel=1.0))
    assert not eng.temporal_vertex_on(eng.temporal_vertex_weights()) and eng.temporal_vertex_on(eng.temporal_vertex_weights(dict(w_temp_vert_vel=1)))
    assert all(hasattr(eng.ScanSequence, k) for k in ("vertex_block", "vertex_term"))


def test_stage_signature_and_yaml():
    from smalify_amd.fitter_3d import trainer
    params = inspect.signature(trainer.Stage.__init__).parameters
    names = list(params)
    assert names[-3:] == ["surface_gates", "chamfer_gates", "robust"]
    assert names[names.index("temporal") + 1] == "temporal_verts" and params["temporal_verts"].default is None
    assert isinstance(trainer.Stage.last_temporal_vertex_losses, property)
    yaml = pytest.importorskip("yaml")
    cfg = yaml.safe_load("stages:\n  fit:\n    scheme: default\n    nits: 3\n    temporal:\n      w_temp_joint: 0.5\n"
                         "    temporal_verts:\n      w_temp_vert_vel: 0.5\n      w_temp_vert_acc: 4.0\n")
    kw = cfg["stages"]["fit"]
    assert set(kw) - {"scheme", "nits"} <= set(params)                           # optimise.py passes the block on as it stands
    assert eng.temporal_vertex_weights(kw["temporal_verts"]) == dict(w_temp_vert_vel=0.5, w_temp_vert_acc=4.0)
    src = inspect.getsource(trainer.Stage.__init__)
    assert "give clip_lengths with it" in src                                     # temporal_verts without clip_lengths raises


# ---- why: a pose a full turn away --------------------------------------------------------------------------------------------------
def test_a_full_turn_in_axis_angle_moves_no_vertex():
    """r and r (1 + 2 pi / |r|) are one rotation: the vertex terms see the surface stand still where the parameter term on
    joint_rot sees the pose jump by 2 pi.  float64, the oracle's LBS."""
    from oracle import smal_oracle as so
    from smalify_amd import synthetic
    om = so.OracleModel(synthetic.synthetic_model(seed=0, shape_family_id=-1))
    rng = np.random.default_rng(4)
    theta = torch.from_numpy(0.2 * rng.standard_normal((1, 35, 3))).repeat(2, 1, 1)
    r = theta[1, 9].clone()
    theta[1, 9] = r * (1.0 + 2.0 * np.pi / float(r.norm()))
    beta = torch.from_numpy(0.3 * rng.standard_normal((1, 20))).repeat(2, 1)
    x = so.smal_forward(om, beta, theta, torch.zeros(2, 6, dtype=torch.float64))[0].numpy()
    assert float(np.abs(x[1] - x[0]).max()) < 1e-6 * float(np.abs(x[0]).max())                  # unchanged to rounding
    vertex = vc.reference64((2,), x, (1.0, 1.0))["losses"]
    d = (theta[1, 1:] - theta[0, 1:]).reshape(-1).numpy()
    joint = float((d * d).sum()) / 102.0                                                      # the joint term at weight 1
    print("vertex terms", vertex, "joint term", joint)
    assert vertex[2] < 1e-12 and joint == pytest.approx((2.0 * np.pi) ** 2 / 102.0, rel=1e-9) and joint > 0.38
