"""The scan-sequence block without a GPU (include/smalfit.h, "scan sequences"): fit3d_sequence_math.h and smalfit_plan.h through the
host shim against a float64 restatement and against the reference's get_temporal form, the dyadic case bit for bit, clip
boundaries, every refusal, the plan, the struct layout, the header's rules, tie_shapes, the command line and the YAML."""
import ctypes as C
import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from smalify_amd import _lib, engine as eng
from tests import host_sequence as hs
from tests import sequence_cases as sc

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "smalfit.h")
NEW_EXPORTS = ("smalfit_scan_sequence_create", "smalfit_scan_sequence_destroy", "smalfit_scan_sequence_couple", "smalfit_scan_sequence_step")


# ---- the arithmetic ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clips", sc.CLIPS, ids=sc.clip_id)
def test_shim_matches_the_float64_restatement(clips):
    st, bar = sc.state(clips), sc.bars()
    got = hs.couple(clips, st, True, sc.WEIGHTS)
    ref = sc.reference64(clips, st, True, sc.WEIGHTS)
    for k in ("g_betas", "g_theta", "g_trans"):
        dev = sc.deviation(got[k], ref[k])
        print(clips, k, dev)
        assert dev <= bar["grad"], (k, dev)
    for t in range(4):
        dev = sc.deviation(got["losses"][t], ref["losses"][t])
        print(clips, "loss", t, dev)
        assert dev <= bar["loss"], (t, dev)
    if sum(clips) == len(clips):                       # nothing is coupled: the gradients keep their bits, the losses read 0
        assert all(np.array_equal(sc.bits(got[k]), sc.bits(st[k])) for k in ("g_betas", "g_theta", "g_trans"))
        assert not got["losses"].any()


@pytest.mark.parametrize("clips", sc.CLIPS, ids=sc.clip_id)
def test_shim_matches_get_temporal_with_autograd(clips):
    """the definition, not only the arithmetic: F.mse_loss(x[n], x[n+1]) * w over the pairs of every clip, in float64"""
    st, bar = sc.state(clips), sc.bars()
    got = hs.couple(clips, st, False, sc.WEIGHTS)
    ref = sc.reference_torch(clips, st, sc.WEIGHTS)
    assert sc.deviation(got["g_theta"], ref["g_theta"]) <= bar["grad"] and sc.deviation(got["g_trans"], ref["g_trans"]) <= bar["grad"]
    for t in range(4):
        assert sc.deviation(got["losses"][t], ref["losses"][t]) <= bar["loss"], t
    assert np.array_equal(sc.bits(got["g_betas"]), sc.bits(st["g_betas"]))          # share_shape off: the rows keep their bits


def test_the_bar_is_three_times_the_float32_restatement():
    m = sc.measured()
    rec = m["float32_restatement_deviation"]
    assert m["ratchet"] == sc.RATCHET == 3.0
    assert m["bar"]["loss"] == pytest.approx(3.0 * rec["loss"], rel=1e-12) and m["bar"]["grad"] == pytest.approx(3.0 * rec["grad"], rel=1e-12)
    now = sc.float32_restatement_deviation()
    print("float32 torch restatement against float64 now:", now, "recorded:", rec)
    assert 0 < now["loss"] <= sc.bars()["loss"] and 0 < now["grad"] <= sc.bars()["grad"]


def test_dyadic_case_equals_the_closed_form_bit_for_bit():
    st, want = sc.dyadic_state(), sc.dyadic_closed_form()
    got = hs.couple(sc.DYADIC_CLIPS, st, True, sc.DYADIC_WEIGHTS)
    for k in ("g_betas", "g_theta", "g_trans", "losses"):
        assert np.array_equal(sc.bits(got[k]), sc.bits(want[k])), k
    assert want["losses"][:3].all() and want["g_theta"][1:].any() and not want["g_theta"][0].any()      # mesh 0 is alone in its clip


def test_no_gradient_crosses_a_clip_boundary():
    clips = (1, 3, 1)
    st = sc.state(clips)
    base = hs.couple(clips, st, True, sc.WEIGHTS)
    moved = {k: v.copy() for k, v in st.items()}
    for k in ("global_rot", "joint_rot", "trans", "g_betas"):
        moved[k][3] += np.float32(0.25)
    got = hs.couple(clips, moved, True, sc.WEIGHTS)
    for k in ("g_betas", "g_theta", "g_trans"):
        for n in (0, 4):
            assert np.array_equal(sc.bits(got[k][n]), sc.bits(base[k][n])), (k, n)
            assert np.array_equal(sc.bits(got[k][n]), sc.bits(st[k][n])), (k, n)      # ... which are the incoming bits
        assert not np.array_equal(sc.bits(got[k][2]), sc.bits(base[k][2])), k          # mesh 2 is mesh 3's neighbour
    assert not np.array_equal(sc.bits(got["losses"]), sc.bits(base["losses"]))


def test_shape_sum_order_and_length_one():
    g = sc.state((5,))["g_betas"]
    for col in (0, 7, 19):
        for n in range(5):
            assert sc.bits(hs.row_sum(g, col, n, 1)) == sc.bits(g[n, col])             # a clip of one: the row's own bits
        s = g[1, col]
        for r in (2, 3):
            s = np.float32(s + g[r, col])
        assert sc.bits(hs.row_sum(g, col, 1, 3)) == sc.bits(s)                         # ascending n, one addition per further row
    got = hs.couple((2, 3), sc.state((5,)), True, (0, 0, 0))
    assert np.array_equal(sc.bits(got["g_betas"][0]), sc.bits(got["g_betas"][1]))
    assert np.array_equal(sc.bits(got["g_betas"][2]), sc.bits(got["g_betas"][4]))
    assert not np.array_equal(sc.bits(got["g_betas"][1]), sc.bits(got["g_betas"][2]))


def test_gradient_operand_order_and_loss_form():
    f = np.float32
    g, w, L, x, p, n = f(0.125), f(0.7), 102, f(0.3), f(-0.2), f(0.45)
    c = f(f(2) * w) / f(L)
    fma = lambda a, b, acc: f(np.float64(a) * np.float64(b) + np.float64(acc))     # one rounding (the operands here keep the sum exact in float64)
    assert sc.bits(hs.grad(g, w, L, x, p, n, 1, 1)) == sc.bits(fma(c, f(f(x - p) + f(x - n)), g))
    assert sc.bits(hs.grad(g, w, L, x, p, n, 1, 0)) == sc.bits(fma(c, f(x - p), g))
    assert sc.bits(hs.grad(g, w, L, x, p, n, 0, 1)) == sc.bits(fma(c, f(x - n), g))
    assert sc.bits(hs.grad(g, w, L, x, p, n, 0, 0)) == sc.bits(g)
    assert sc.bits(hs.loss(w, f(1.7), 3)) == sc.bits(w * f(f(1.7) / f(3)))


# ---- refusals and the plan -----------------------------------------------------------------------------------------------------
def test_every_refusal_text():
    losses = np.zeros(4, np.float32)
    ok = lambda **kw: hs.block(True, (0.5, 0.5, 0.5), losses.ctypes.data, **kw)
    assert hs.refusal(ok()) is None
    assert hs.refusal(ok(), handle_meshes=3) == "the sequence handle was built for another num_meshes"
    assert hs.refusal(ok(), lengths_sum=5) == "clip_lengths do not sum to num_meshes"
    for i, name in enumerate(hs.WEIGHT_KEYS):
        for bad in (float("nan"), float("inf"), -float("inf")):
            w = [0.5, 0.5, 0.5]
            w[i] = bad
            assert hs.refusal(hs.block(True, w, losses.ctypes.data)) == name + " is not finite"
    assert hs.refusal(hs.block(True, (0.5, 0.5, 0.5), None)) == "losses is NULL"
    total = np.zeros(1, np.float32)
    assert hs.refusal(ok(step_total=total.ctypes.data)) is None
    assert hs.refusal(ok(step_total=total.ctypes.data), step=False) == "step_total given outside a step"
    assert hs.refusal(ok(), joint_rot=False) == "w_temp_joint > 0 but joint_rot is missing"
    assert hs.refusal(ok(), global_rot=False) == "w_temp_global > 0 but global_rot is missing"
    assert hs.refusal(ok(), trans=False) == "w_temp_trans > 0 but trans is missing"
    assert hs.refusal(hs.block(True, (0, -1.0, 0), losses.ctypes.data), joint_rot=False, global_rot=False, trans=False) is None
    # the handle's own
    assert hs.create_refusal(4, (1, 3)) is None
    assert hs.create_refusal(4, (1, 3), given=False) == "null argument"
    assert hs.create_refusal(0, (1,)) == "num_meshes and num_clips must be positive"
    assert hs.create_refusal(4, ()) == "num_meshes and num_clips must be positive"
    assert hs.create_refusal(4, (4, 0)) == "every clip length must be positive"
    assert hs.create_refusal(4, (5, -1)) == "every clip length must be positive"
    assert hs.create_refusal(4, (1, 2)) == "clip_lengths do not sum to num_meshes"
    assert hs.create_refusal(4, (3, 2)) == "clip_lengths do not sum to num_meshes"


def test_plan_launches_nothing_when_nothing_is_coupled():
    off = dict(launch=False, share=False, joint=False, trans=False, blocks=0, **{"global": False})
    on = hs.block(True, (0.5, 0.0, 2.0))
    assert hs.plan(None) == off
    assert hs.plan(on, any_long=False) == off                                             # every clip of length 1, any weights
    assert hs.plan(hs.block(False, (0, 0, 0))) == off                                     # nothing switched on
    assert hs.plan(hs.block(True, (0, -1, 0)), betas_given=False) == off                  # the shape is shared only while betas is trained
    assert hs.plan(hs.block(False, (0, 0, -3.0))) == off
    p = hs.plan(on, num_meshes=5, num_clips=3, num_betas=20)
    assert p == dict(launch=True, share=True, joint=True, trans=True, blocks=1 + (3 * 20 + 5 * 108 + 255) // 256, **{"global": False})
    p = hs.plan(hs.block(True, (0, 0, 0)), num_meshes=5, num_clips=3, num_betas=20)
    assert p["launch"] and p["share"] and p["blocks"] == 2                                # the loss block and 60 shape sums
    p = hs.plan(on, betas_given=False, num_meshes=32, num_clips=1, num_betas=20)
    assert p["launch"] and not p["share"] and p["blocks"] == 1 + (32 * 108 + 255) // 256


# ---- the header and the binding --------------------------------------------------------------------------------------------------
def test_struct_layout_matches_the_header_and_the_shim(tmp_path):
    cls, cname = _lib.SequenceArgs, "smalfit_sequence_args"
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "smalfit.h"', "int main(void) {",
             'printf("sizeof %%zu\\n", sizeof(%s));' % cname]
    lines += ['printf("%s %%zu\\n", offsetof(%s, %s));' % (f, cname, f) for f, _ in cls._fields_]
    lines += ["return 0; }"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)     # the header compiles as C
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines())
    assert int(got["sizeof"]) == C.sizeof(cls) == hs.sizeof_args()
    assert [int(got[f]) for f, _ in cls._fields_] == [getattr(cls, f).offset for f, _ in cls._fields_] == hs.offsets()


def test_header_rules_for_the_new_exports():
    text = open(HEADER).read()
    assert re.search(r"#define SMALFIT_ABI_VERSION 6\b", text) and _lib.ABI_VERSION == 6
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in NEW_EXPORTS:
        assert name in _lib.SIGNATURES and name in _lib.LAZY_SYMBOLS, name
        if name.endswith("_create"):
            continue
        # the sequence handle is the FIRST argument: the entry-order matrix keys on engine / objective handles in that place
        assert re.search(r"\b%s\s*\(\s*smalfit_scan_sequence\s*\*" % name, code), name
    declared = set(re.findall(r"\b(smalfit_[a-z_0-9]+)\s*\(", text))            # comments included, as tests/test_cabi_exports.py reads it
    assert set(NEW_EXPORTS) <= declared and declared == set(_lib.SIGNATURES)


# ---- Python: tie_shapes, the command line, the YAML -------------------------------------------------------------------------------
def _stand_in(N=5, nb=6):
    rng = np.random.default_rng(3)
    return types.SimpleNamespace(batch_size=N, betas=torch.nn.Parameter(torch.from_numpy(rng.standard_normal((N, nb)).astype(np.float32))),
                                 log_beta_scales=torch.nn.Parameter(torch.zeros(N, 6), requires_grad=False))


def test_tie_shapes_writes_one_row_per_clip():
    from smalify_amd.fitter_3d import trainer
    fit = _stand_in()
    before = fit.betas.detach().clone()
    assert not trainer._clip_rows_tied(before.numpy(), (1, 3, 1))
    trainer.tie_shapes(fit, (1, 3, 1))
    after = fit.betas.detach()
    assert torch.equal(after[0], before[0]) and torch.equal(after[4], before[4])
    assert all(torch.equal(after[n], before[1]) for n in (1, 2, 3))
    assert trainer._clip_rows_tied(after.numpy(), (1, 3, 1)) and not trainer._clip_rows_tied(after.numpy(), (5,))
    fit = _stand_in()
    trainer.tie_shapes(fit, (2, 3), how="mean")
    assert torch.equal(fit.betas.detach()[2], before[2:5].mean(dim=0)) and torch.equal(fit.betas.detach()[3], fit.betas.detach()[4])
    assert torch.equal(fit.betas.detach()[0], before[0:2].mean(dim=0))
    with pytest.raises(ValueError, match="sum 5"):
        trainer.tie_shapes(fit, (2, 2))
    with pytest.raises(ValueError, match="how must be"):
        trainer.tie_shapes(fit, (5,), how="median")
    fit.log_beta_scales.data[1, 0] = 0.5
    with pytest.raises(ValueError, match="log_beta_scales"):
        trainer.tie_shapes(fit, (5,))
    trainer.tie_shapes(fit, (1, 1, 3))                                            # mesh 1 is alone in its clip
    with pytest.raises(ValueError, match="tie_shapes"):
        trainer._require_tied_shapes(_stand_in(), (5,))


def test_binding_helpers():
    assert eng.temporal_weights() == dict(w_temp_joint=0.0, w_temp_global=0.0, w_temp_trans=0.0)
    assert eng.temporal_weights(dict(w_temp_trans=2))["w_temp_trans"] == 2.0
    with pytest.raises(KeyError, match="unknown temporal weight"):
        eng.temporal_weights(dict(w_temp=1.0))
    assert eng.check_clip_lengths((2, 1), 3) == [2, 1]
    for bad in ((), (2, 2), (3, 0), (4, -1)):
        with pytest.raises(ValueError):
            eng.check_clip_lengths(bad, 3)


def test_command_line_and_yaml():
    from smalify_amd.fitter_3d import optimise, trainer
    p = optimise.build_parser()
    plain = p.parse_args([])
    assert plain.sequence is False and plain.clip_lengths is None and optimise.sequence_clip_lengths(plain, 4) is None
    assert optimise.sequence_clip_lengths(p.parse_args(["--sequence"]), 7) == [7]
    assert optimise.sequence_clip_lengths(p.parse_args(["--clip_lengths", "2", "1", "4"]), 7) == [2, 1, 4]
    with pytest.raises(ValueError):
        optimise.sequence_clip_lengths(p.parse_args(["--clip_lengths", "2", "1"]), 7)
    with pytest.raises(ValueError):
        optimise.sequence_clip_lengths(p.parse_args(["--clip_lengths", "8", "-1"]), 7)
    with pytest.raises(ValueError):
        optimise.sequence_clip_lengths(p.parse_args(["--sequence", "--clip_lengths", "3", "4"]), 7)
    yaml = pytest.importorskip("yaml")
    cfg = yaml.safe_load("args:\n  sequence: true\nstages:\n  fit:\n    scheme: default\n    nits: 3\n    share_shape: false\n"
                         "    temporal:\n      w_temp_joint: 0.5\n      w_temp_trans: 2.0\n")
    args = p.parse_args([])
    for k, v in cfg["args"].items():                                             # as optimise.main applies the YAML's args
        setattr(args, k, v)
    assert optimise.sequence_clip_lengths(args, 3) == [3]
    kw = cfg["stages"]["fit"]
    assert eng.temporal_weights(kw["temporal"]) == dict(w_temp_joint=0.5, w_temp_global=0.0, w_temp_trans=2.0)
    params = inspect.signature(trainer.Stage.__init__).parameters
    assert set(kw) - {"scheme", "nits"} <= set(params)                           # optimise.py passes the block on
    assert params["clip_lengths"].default is None and params["share_shape"].default is True and params["temporal"].default is None
