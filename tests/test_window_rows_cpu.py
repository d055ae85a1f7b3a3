"""CPU: smalfit_fit_eval_windows as far as it goes without a device -- the symbol and the struct's layout, the refusals of
smalfit_plan.h called through a g++ shim of their own (tests/window_rows_shim.cpp), the number of rows against the oracle's
window groups, and the drop-in's partition / key bookkeeping on CPU tensors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import smal_oracle as so
from smalify_amd import _lib
from smalify_amd.smal_fitter.epoch import StateKey, WindowPartition
from tests import host_shim
from tests.host_plan import valid_fit_args

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER_DIR = os.path.join(HERE, "..", "include")

SIZE_TEXT = "smalfit_window_rows.struct_size does not match this library (built against another smalfit.h?)"
LOSSES_TEXT = "smalfit_window_rows.losses missing"
COUNT_TEXT = "smalfit_window_rows.num_windows is not the number of windows these frames belong to"
SUBJECT_TEXT = "window rows need subject_frames = 0 (independent images already have one row per image)"
SCALES_TEXT = "smalfit_window_rows.g_log_beta_scales needs shared log_beta_scales (logscale_mode 1)"


@pytest.fixture(scope="module")
def shim():
    lib = host_shim.build("window_rows_shim.cpp", "window_rows_shim")
    lib.wr_refusal.restype = C.c_char_p
    lib.wr_window_rows_size_refusal.restype = C.c_char_p
    return lib


def _rows(num_windows, **fields):
    r = _lib.WindowRows()
    r.num_windows, r.losses, r.g_betas = num_windows, 0x10000, 0x20000
    for k, v in fields.items():
        setattr(r, k, v)
    return r


def _refusal(shim, a, r, max_frames=64, shape_dim=26):
    why = shim.wr_refusal(C.byref(a), C.byref(r), max_frames, 1, shape_dim)
    return why.decode() if why else None


def test_symbol_is_exported_and_abi_version_unchanged():
    if _lib.needs_rebuild():
        _lib.build_library()
    lib = _lib.load()
    assert hasattr(lib, "smalfit_fit_eval_windows")
    assert "smalfit_fit_eval_windows" in _lib.SIGNATURES and "smalfit_fit_eval_windows" in _lib.LAZY_SYMBOLS
    assert _lib.resolve(lib, "smalfit_fit_eval_windows").argtypes[-1] == C.POINTER(_lib.WindowRows)
    assert _lib.ABI_VERSION == 6 and lib.smalfit_version() == 6
    text = open(os.path.join(HEADER_DIR, "smalfit.h")).read()
    assert "#define SMALFIT_ABI_VERSION 6" in text


def test_a_library_without_the_symbol_is_named(tmp_path):
    """the binding resolves the entry point lazily: a version-6 library built before it loads, and asking for the symbol says which"""
    class Old:
        _name = "libsmalfit-old.so"
    with pytest.raises(_lib.SmalfitError, match="smalfit_fit_eval_windows"):
        _lib.resolve(Old(), "smalfit_fit_eval_windows")


def test_struct_layout_matches_the_header(tmp_path, shim):
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "smalfit.h"', "int main(void) {",
             'printf("sizeof %zu\\n", sizeof(smalfit_window_rows));']
    for field, _ in _lib.WindowRows._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(smalfit_window_rows, %s));' % (field, field))
    lines += ["return 0; }"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", HEADER_DIR, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = {a: int(b) for a, b in (ln.split() for ln in out.strip().splitlines())}
    assert got["sizeof"] == C.sizeof(_lib.WindowRows) == shim.wr_sizeof_window_rows()
    assert [f for f, _ in _lib.WindowRows._fields_] == ["struct_size", "num_windows", "losses", "g_betas", "g_log_beta_scales"]
    for field, _ in _lib.WindowRows._fields_:
        assert got[field] == getattr(_lib.WindowRows, field).offset, field
    assert _lib.WindowRows().struct_size == got["sizeof"]
    # a row of the engine's workspace holds a row of either gradient
    assert shim.wr_row_floats(0) >= 20 and shim.wr_row_floats(1) >= 6


def test_every_refusal_text(shim):
    a = valid_fit_args()                                   # 4 frames, windows of 2, shared limb scales
    assert _refusal(shim, a, _rows(2)) is None
    assert _refusal(shim, a, _rows(2, g_betas=None)) is None
    assert _refusal(shim, a, _rows(2, g_log_beta_scales=0x30000)) is None
    # the rows' struct_size before any other field of either block: a fit block that would be refused does not get a word in
    short = _rows(2)
    short.struct_size -= 8
    assert _refusal(shim, a, short) == SIZE_TEXT
    assert _refusal(shim, valid_fit_args(window=0), short) == SIZE_TEXT
    assert shim.wr_window_rows_size_refusal(C.byref(short)).decode() == SIZE_TEXT
    # ... then the fit block, by smalfit_fit_eval's rules
    assert _refusal(shim, valid_fit_args(window=0), _rows(2)) == "window must be positive"
    assert _refusal(shim, a, _rows(2, losses=None)) == LOSSES_TEXT
    for wrong in (0, 1, 3, -1):
        assert _refusal(shim, a, _rows(wrong)) == COUNT_TEXT
    indep = valid_fit_args(subject_frames=1, window=1, temporal=0, logscale_mode=2)
    assert _refusal(shim, indep, _rows(4), shape_dim=20) == SUBJECT_TEXT
    for mode in (0, 2):
        b = valid_fit_args(logscale_mode=mode)
        assert _refusal(shim, b, _rows(2), shape_dim=20) is None
        assert _refusal(shim, b, _rows(2, g_log_beta_scales=0x30000), shape_dim=20) == SCALES_TEXT


def test_row_count_is_the_oracles_window_groups(shim):
    """num_windows for every (M, window, frame_offset, total_frames) with M, window <= 12, frame_offset <= 12 and total_frames
    0 (= the frames end the sequence), exactly that, or three frames more: the rows are the groups of FitProblem.window_groups(),
    and the owned ones those whose prior term the evaluation carries"""
    z = np.zeros
    checked = 0
    for M in range(1, 13):
        for window in range(1, 13):
            for off in range(0, 13):
                for total in (0, off + M, off + M + 3):
                    p = so.FitProblem(None, 8, z((M, 25, 2)), z((M, 25)), z((M, 1, 1)), z((1, 1)), z(1), z(1), z((1, 1)), z(1), window,
                                      frame_offset=off, total_frames=total or None)
                    groups = p.window_groups()
                    W = len(groups)
                    assert shim.wr_window_rows_count(window, off, M) == W, (M, window, off, total)
                    assert shim.wr_prior_windows(window, off, M) == sum(1 for g in groups if g[2])
                    a = valid_fit_args(num_frames=M, window=window, frame_offset=off, total_frames=total)
                    assert _refusal(shim, a, _rows(W)) is None
                    assert _refusal(shim, a, _rows(W + 1)) == COUNT_TEXT and _refusal(shim, a, _rows(W - 1)) == COUNT_TEXT
                    # rows are consecutive runs of frames, in order
                    assert [i for g in groups for i in g[0]] == list(range(M))
                    checked += 1
    assert checked == 12 * 12 * 13 * 3


# ---- the drop-in's bookkeeping --------------------------------------------------------------------------------------
def test_partition_aligned_unaligned_ragged_and_oversized():
    p = WindowPartition(5, 2)
    assert p.num_windows == 3
    assert [p.window_of(list(p.frames(w))) for w in range(3)] == [0, 1, 2]
    assert p.window_of([4]) == 2 and p.window_of(range(2, 4)) == 1           # the ragged last window; a range object
    assert p.window_of(np.arange(0, 2)) == 0                                   # integer-likes
    for other in ([1, 2], [0], [0, 1, 2], [1], [3, 2], [2, 3, 4], [4, 5], [], [6, 7], [0.5, 1.5], [-2, -1]):
        assert p.window_of(other) is None, other
    assert p.frame_windows() == [0, 0, 1, 1, 2]
    big = WindowPartition(3, 8)                                                # window > N: one window, the whole sequence
    assert big.num_windows == 1 and big.window_of([0, 1, 2]) == 0 and big.window_of([0, 1]) is None
    assert big.window_of(list(range(8))) is None and big.frame_windows() == [0, 0, 0]
    one = WindowPartition(4, 1)
    assert [one.window_of([i]) for i in range(4)] == [0, 1, 2, 3] and one.window_of([0, 1]) is None
    with pytest.raises(ValueError):
        WindowPartition(0, 2)


def test_state_key_turnover():
    a, b, vis = torch.zeros(3, requires_grad=True), torch.ones(4, 2), torch.ones(2, 5, dtype=torch.long)
    w = (10.0, 0.0, 1.0, 5.0, 0.0, 2.0, False)
    key = StateKey((a, b, vis), w)
    assert key.matches((a, b, vis), w)
    a.requires_grad_(False)                                    # changes no value: no turnover
    assert key.matches((a, b, vis), w)
    a.requires_grad_(True)
    assert key.matches((a, b, vis), w)
    vis *= 0                                                   # the driver's in-place edit
    assert not key.matches((a, b, vis), w)
    key = StateKey((a, b, vis), w)
    vis[:, [1, 3]] = 1                                         # ... and its item assignment
    assert not key.matches((a, b, vis), w)
    key = StateKey((a, b, vis), w)
    with torch.no_grad():
        a.add_(1.0)                                            # what optimizer.step() does
    assert not key.matches((a, b, vis), w)
    key = StateKey((a, b, vis), w)
    vis_cpu = vis.clone().float()                              # replaced by another tensor of the same values
    assert not key.matches((a, b, vis_cpu), w)
    assert key.matches((a, b, vis), w)
    assert not key.matches((a, b, vis), w[:1] + (9.0,) + w[2:])            # a weight
    assert not key.matches((a, b, vis), w[:-1] + (True,))                  # the joint-limit switch
    assert not key.matches((a, b), w)
    # the key keeps its tensors alive: an id cannot come back as another tensor's
    assert key.tensors[0] is a and key.tensors[2] is vis
