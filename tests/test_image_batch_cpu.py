"""The arithmetic of a batch of independent images that needs no device: ImageBatchFitter's flat layout and Adam ranges,
the launch form every case of tests/test_gpu_image_batch.py takes, the argument block's two fields, and the expected
values' plumbing (an independent image is a one-frame problem of the unchanged oracle)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from smalify_amd import _lib, image_batch as ib
from tests import fold_forms as ff
from tests import host_plan
from tests import image_batch_cases as ic
from tests import lbs_forms as lf

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def test_flat_layout_and_adam_ranges():
    for N in (1, 2, 6, 64):
        offs, shapes, size = ib.flat_layout(N)
        assert list(offs) == ["betas", "log_beta_scales", "joint_rotations", "global_rotation", "trans"]
        assert size == N * (20 + 6 + 102 + 3 + 3)
        # tensors tile the buffer without gaps or overlaps, each as large as its shape
        at = 0
        for k, (o, c) in offs.items():
            assert o == at and c == int(np.prod(shapes[k])) and shapes[k][0] == N
            at += c
        assert at == size
        # stage 0: global rotation + translation, one range
        assert ib.trainable_names(0) == ("global_rotation", "trans")
        assert ib.adam_ranges(offs, ib.trainable_names(0)) == [(offs["global_rotation"][0], size)]
        # stages 1-3 with limb scaling: everything, one range
        assert ib.adam_ranges(offs, ib.trainable_names(1)) == [(0, size)] == ib.adam_ranges(offs, ib.trainable_names(3))
        # ... without: the limb scales are a gap, two ranges that cover exactly the four trained tensors
        names = ib.trainable_names(2, allow_limb_scaling=False)
        assert "log_beta_scales" not in names and len(names) == 4
        r = ib.adam_ranges(offs, names)
        assert r == [(0, N * 20), (N * 26, size)]
        covered = set()
        for b, e in r:
            covered |= set(range(b, e))
        want = set()
        for k in names:
            want |= set(range(offs[k][0], offs[k][0] + offs[k][1]))
        assert covered == want
        assert len(r) <= 4                                     # smalfit_adam_args holds four ranges


def test_the_fitters_ranges_are_the_layouts():
    """ImageBatchFitter takes FusedFitter's _segments over this layout: the same ranges as adam_ranges"""
    from smalify_amd import fitter as fit

    class Probe(ib.ImageBatchFitter):
        def __init__(self, N):
            self.offsets, _, _ = self._parameter_layout(N)
    for N in (1, 6):
        p = Probe(N)
        for stage in (0, 1):
            for als in (True, False):
                names = ib.trainable_names(stage, als)
                assert [tuple(s) for s in fit.FusedFitter._segments(p, names)] == ib.adam_ranges(p.offsets, names)
    assert Probe(3)._limb_scales_shared() is False
    assert Probe(3)._sequence_kwargs() == dict(window=1, temporal=False, subject_frames=1)


@pytest.fixture(scope="module")
def plan():
    return host_plan.load()


def test_eval_cases_take_every_skinning_launch(plan):
    assert {form for _, form in ic.EVAL_CASES} == {"plain", "split", "wide"}
    for N, form in ic.EVAL_CASES:
        assert ic.skin_form(N) == form == plan.skin_form(N, lf.NUM_VERTS), N
    assert [ic.skin_form(M) for M in (4, 5, 48, 49)] == ["plain", "split", "split", "wide"]
    # independent mode reaches that launch with one shape set per frame: M times the shape blocks, M sets of dbeta partials in
    # one frame group each, a prior block per 16 frames
    Vp = lf.padded_verts()
    for N, _ in ic.EVAL_CASES:
        assert plan.head_blocks(N, Vp, True, "per_frame") - plan.head_blocks(N, Vp, False, "shared") == (N - 1) * (Vp // 256) + (N + 15) // 16 - 1
        assert plan.dbeta_grid(True, Vp, False, N)[1:] == (N, 1) and plan.dbeta_grid(True, Vp, True, N)[1:] == (1, ff.BETA_GROUPS)
    # ... and keeps the plain chain: plan_fold refuses the mode whatever the ranges, so smalfit_fit_run never folds it
    for N in (1, 6):
        offs, shapes, size = ib.flat_layout(N)
        o = {k: v[0] for k, v in offs.items()}
        for stage in (0, 1):
            ranges = ib.adam_ranges(offs, ib.trainable_names(stage))
            ok, train, why = plan.plan_fold(N, 2, o, ranges, dict.fromkeys(offs, True), subject_frames=1)
            assert not ok and not any(train.values())
            assert all(plan.path(K, False, False, ds, ok) == "plain" for K in (1, 2, 7) for ds in (True, False))


def test_argument_block_fields():
    names = [f[0] for f in _lib.FitArgs._fields_]
    assert names[-2:] == ["subject_frames", "losses_per_frame"] and names[-3] == "total_frames"
    header = open(os.path.join(ROOT, "include", "smalfit.h")).read()
    assert "#define SMALFIT_ABI_VERSION %d" % _lib.ABI_VERSION in header and _lib.ABI_VERSION == 6
    a = _lib.FitArgs()
    assert a.subject_frames == 0 and not a.losses_per_frame and a.struct_size == C.sizeof(_lib.FitArgs)


def test_images_differ_and_are_one_frame_problems_of_the_oracle():
    images = ic.make_images(3, 32)
    st = ic.stack([im["near"] for im in images])
    assert st["betas"].shape == (3, 20) and st["log_beta_scales"].shape == (3, 6) and st["joint_rotations"].shape == (3, 34, 3)
    for k in ("betas", "log_beta_scales", "global_rotation", "trans"):
        assert not np.allclose(st[k][0], st[k][1]) and not np.allclose(st[k][1], st[k][2]), k
    assert all(im["prob"].N == 1 and im["prob"].window == 1 for im in images)
    tg = ic.targets(images)
    assert tg["tsil"].shape == (3, 32, 32) and set(np.unique(tg["tsil"])) <= {0.0, 1.0}      # storable as bytes
    # the expected terms: no temporal share, a prior term of its own per image
    terms, grads = ic.oracle_eval(images[1]["prob"], images[1]["near"], 2)
    assert terms[3] > 0 and terms[4] > 0 and (terms[5:8] == 0).all() and grads["betas"].shape == (20,)
    terms2, _ = ic.oracle_eval(images[2]["prob"], images[2]["near"], 2)
    assert terms2[3] != terms[3]
    # the 20-dim case drops the limb scales from the prior
    im20 = ic.make_images(1, 32, unity=False)[0]
    assert im20["prob"].shape_prec.shape == (20, 20) and not im20["prob"].unity and (im20["near"]["log_beta_scales"] == 0).all()
    # two iterations of the loop move the stage's parameters only
    out = ic.oracle_loop(images[0]["prob"], ic.initial_state(), ((0, 2),))
    init = ic.initial_state()
    assert np.array_equal(out["betas"], init["betas"].astype(np.float64)) and not np.array_equal(out["trans"], init["trans"])
