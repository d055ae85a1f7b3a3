"""CPU: the bound behind raster_bwd_kernel's 32-bit lane offsets (smalfit_plan.h: kMaxModelFaces) -- a face's byte offset in its
frame's candidate lists, the largest of the five it forms, fits 32 bits for every model smalfit_model_create accepts."""
import os
import re

import pytest

from tests import host_plan

CSRC = os.path.join(os.path.dirname(__file__), "..", "smalify_amd", "csrc")


@pytest.fixture(scope="module")
def plan():
    return host_plan.load()


def _constant(text, name):
    return eval(re.search(r"constexpr int %s = ([0-9<>() ]+);" % name, text).group(1))


def test_a_face_offset_fits_32_bits_for_every_accepted_model(plan):
    max_faces = _constant(open(os.path.join(CSRC, "smalfit_plan.h")).read(), "kMaxModelFaces")
    raster = open(os.path.join(CSRC, "kernels_raster.inc")).read()
    list_cap = _constant(raster, "kListCap")
    assert max_faces * list_cap <= 2 ** 32 and max_faces == 2 ** 25
    # the other per-face strides are smaller: record 64, adjoint row 24, box 8, length 1 bytes
    assert list_cap >= 64
    assert "static_assert((unsigned long long)kMaxModelFaces * kListCap <= (1ull << 32)" in raster
    assert plan.model_dims_refusal(3889, max_faces, 41) is None
    for F in (max_faces + 1, 2 ** 31 - 1):
        assert plan.model_dims_refusal(3889, F, 41) == \
            "num_faces above 33554432 is not supported (the backward gather addresses a frame's faces by 32-bit byte offsets)"
    assert plan.model_dims_refusal(3889, max_faces + 1, 65).startswith("num_faces")        # the first fault is reported

