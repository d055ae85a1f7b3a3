"""The sweep launch's grid and its role decode (smalfit_plan.h: sweep_launch_grid, sweep_block_at), through
tests/host_sweep_shim.cpp: the host launches what the first returns and raster_sweep_kernel asks the second what its workgroup
does, so every workgroup id must have exactly one role and every (frame, block) of the problem exactly one workgroup."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import host_shim

FRAMES = (1, 8, 9, 64)
FACES = (8, 33, 7774)
FRAME, SWEEP, JOINT = 0, 1, 2


@pytest.fixture(scope="module")
def shim():
    return host_shim.build("host_sweep_shim.cpp", "host_sweep_shim")


def _grid(shim, F, M, joints):
    out = (C.c_int * 5)()
    shim.hs_sweep_launch_grid(F, M, int(joints), out)
    return tuple(out)


def _blocks(shim, F, M, joints):
    grid = _grid(shim, F, M, joints)[3]
    out = np.zeros((grid, 3), np.int32)
    shim.hs_sweep_blocks(F, M, int(joints), out.ctypes.data_as(C.c_void_p))
    return out


@pytest.mark.parametrize("M,F,joints", list(itertools.product(FRAMES, FACES, (False, True))))
def test_grid_is_the_sum_of_its_parts(shim, M, F, joints):
    nfr, nsw, nj, grid, bpf = _grid(shim, F, M, joints)
    pad = (M + 7) // 8 * 8
    assert bpf == (F + 31) // 32
    assert nfr == pad and nfr % 8 == 0 and nfr >= M
    assert nsw == bpf * pad
    assert nj == (shim.hs_joint_blocks() * M if joints else 0) and shim.hs_joint_blocks() == 41
    assert grid == nfr + nsw + nj


@pytest.mark.parametrize("M,F,joints", list(itertools.product(FRAMES, FACES, (False, True))))
def test_every_workgroup_has_one_role_and_every_block_one_workgroup(shim, M, F, joints):
    nfr, nsw, nj, grid, bpf = _grid(shim, F, M, joints)
    d = _blocks(shim, F, M, joints)
    role, n, bx = d[:, 0], d[:, 1], d[:, 2]
    assert set(np.unique(role)) <= {FRAME, SWEEP, JOINT}
    # the layout: frame riders first, sweep blocks, joint riders last
    assert np.all(role[:nfr] == FRAME) and np.all(role[nfr:nfr + nsw] == SWEEP) and np.all(role[nfr + nsw:] == JOINT)
    # frame riders: frames 0 .. pad - 1 once each, those >= M are padding; a multiple of 8, so the sweep blocks keep their XCD
    assert np.array_equal(n[:nfr], np.arange(nfr)) and np.all(bx[:nfr] == 0)
    assert int(np.sum(role == FRAME)) % 8 == 0
    # sweep blocks: every (frame, block) below (M, blocks per frame) exactly once, the rest are frames of the padding
    sw = d[nfr:nfr + nsw]
    live = sw[sw[:, 1] < M]
    assert len(live) == M * bpf
    assert len({(int(a), int(b)) for _, a, b in live}) == M * bpf
    assert np.all((live[:, 2] >= 0) & (live[:, 2] < bpf)) and np.all(live[:, 1] >= 0)
    assert np.all((sw[:, 2] >= 0) & (sw[:, 2] < bpf)) and np.all(sw[:, 1] < nfr)
    # frame n on XCD n % 8: workgroups are dealt to the XCDs round-robin by their id in the whole launch
    ids = np.arange(nfr, nfr + nsw)
    assert np.array_equal(ids % 8, sw[:, 1] % 8)
    # joint riders: every (frame, joint) once
    jr = d[nfr + nsw:]
    assert len(jr) == nj
    if joints:
        assert {(int(a), int(b)) for _, a, b in jr} == set(itertools.product(range(M), range(41)))


def test_single_ids_agree_with_the_table(shim):
    F, M = 33, 9
    d = _blocks(shim, F, M, True)
    out = (C.c_int * 3)()
    for b in (0, 8, 15, 16, 17, 16 + 2 * 16 - 1, 16 + 2 * 16, len(d) - 1):
        shim.hs_sweep_block_at(b, F, M, out)
        assert tuple(out) == tuple(int(x) for x in d[b])
    # the sweep blocks' decode is xcd_block_at of the id behind the frame riders
    o2 = (C.c_int * 2)()
    shim.hs_xcd_block_at(5, 2, o2)
    assert tuple(o2) == (5, 0)
    shim.hs_xcd_block_at(8 + 5, 2, o2)
    assert tuple(o2) == (5, 1)
    shim.hs_xcd_block_at(16 + 5, 2, o2)
    assert tuple(o2) == (13, 0)
    assert tuple(int(x) for x in d[16 + 16 + 5]) == (SWEEP, 13, 0)
