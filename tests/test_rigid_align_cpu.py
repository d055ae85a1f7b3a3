"""CPU: the rigid pre-alignment's host side -- rigid_align_math.h's solve and sums against SVD Kabsch in float64, smalfit_plan.h's
refusals in their order, the block's layout against gcc, the binding, the 24 built-in starts, and the admission condition of every
recovery case of tests/rigid_align_cases.py (the float64 restatement alone recovers R*).  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from smalify_amd import _lib
from tests import host_rigid_align as hr
from tests import rigid_align_cases as rc

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "smalfit.h")
EPS32 = float(np.finfo(np.float32).eps)
NEW_EXPORTS = ("smalfit_rigid_aligner_create", "smalfit_rigid_aligner_destroy", "smalfit_rigid_align")


# ---- the solve ------------------------------------------------------------------------------------------------------------------
def _pair_set(kind, seed=0, n=60):
    rs = np.random.RandomState(seed)
    x = rs.randn(n, 3) * [1.0, 0.6, 0.3]
    R = rc.axis_angle(rs.randn(3), rs.uniform(20, 160))
    t = rs.randn(3)
    if kind == "planar":
        x[:, 2] = 0.0
    elif kind == "collinear":
        x = rs.uniform(-1, 1, n)[:, None] * np.array([[0.5, -0.7, 0.2]]) + [0.1, 0.2, 0.3]
    elif kind == "coincident":
        x = np.tile([[0.4, -0.1, 0.7]], (n, 1))
    p = x @ R.T + t
    if kind == "mirror":
        p = (x * [-1.0, 1.0, 1.0]) @ R.T + t      # the unconstrained optimum is a reflection
    if kind == "random":
        p = p + 0.01 * rs.randn(n, 3)
    w = rs.uniform(0.5, 1.5, n) / n
    return x.astype(np.float32), p.astype(np.float32), w.astype(np.float32)


@pytest.mark.parametrize("seed", (0, 1, 2))
@pytest.mark.parametrize("kind", ("random", "planar", "mirror", "collinear", "coincident"))
def test_solve_against_svd_kabsch(kind, seed):
    x, p, w = _pair_set(kind, seed)
    cX, cP = hr.means(x), hr.means(p)
    M = hr.moments_of_pairs(x, p, w, cX, cP)
    prev = np.concatenate([rc.axis_angle([1, -1, 2], 33.0), [[0.1], [0.2], [0.3]]], 1).astype(np.float32).reshape(-1)
    T, kept, gap, scale = hr.solve(M, cX, cP, prev)
    T = T.reshape(3, 4).astype(np.float64)
    R, t = T[:, :3], T[:, 3]
    assert np.isfinite(T).all() and np.isfinite([gap, scale]).all()
    x64, p64, w64 = x.astype(np.float64), p.astype(np.float64), w.astype(np.float64)
    Rk, tk, determined = rc.kabsch(x64, p64, w64, cX.astype(np.float64), cP.astype(np.float64))
    W = w64.sum()
    mx, mp = (w64[:, None] * x64).sum(0) / W, (w64[:, None] * p64).sum(0) / W
    if kind in ("collinear", "coincident"):
        assert not determined and kept == 1
        assert np.array_equal(T[:, :3].astype(np.float32), prev.reshape(3, 4)[:, :3])      # the previous rotation, bit for bit
        assert np.abs(t - (mp - R @ mx)).max() <= 64 * EPS32 * (1.0 + np.abs(mp).max() + np.abs(mx).max())
        return
    assert determined and kept == 0
    # a proper rotation, never a reflection: float32 products of a unit quaternion normalised in float32
    assert abs(np.linalg.det(R) - 1.0) <= 16 * EPS32
    assert np.abs(R @ R.T - np.eye(3)).max() <= 16 * EPS32
    # the float32 sums of n pairs are off by at most ~n eps of `scale`, the Jacobi sweeps by a few eps more; an eigenvector moves by
    # the matrix's error over the gap to the next eigenvalue (both from the float64 restatement, not from the code under test)
    U, s, Vt = np.linalg.svd((w64[:, None, None] * (x64 - mx)[:, :, None] * (p64 - mp)[:, None, :]).sum(0))
    d = np.sign(np.linalg.det(U) * np.linalg.det(Vt))
    gap64 = 2.0 * (s[1] + d * s[2])
    scale64 = np.sqrt((w64 * ((x64 - cX) ** 2).sum(1)).sum() * (w64 * ((p64 - cP) ** 2).sum(1)).sum())
    tol = (len(x) + 64) * EPS32 * scale64 / gap64
    print(kind, seed, "angle", rc.rotation_angle(R, Rk), "tol", tol, "gap/scale", gap64 / scale64)
    assert abs(gap - gap64) <= (len(x) + 64) * EPS32 * scale64
    assert rc.rotation_angle(R, Rk) <= tol
    assert np.abs(t - tk).max() <= tol * (1.0 + np.abs(mx).max()) + 16 * EPS32 * (1.0 + np.abs(mp).max())


def test_pair_sums_and_combination():
    rs = np.random.RandomState(5)
    xc, pc = rs.randn(3).astype(np.float32), rs.randn(3).astype(np.float32)
    m = hr.pair_moments(xc, pc, 0.25)
    assert m[0] == 1.0 and np.array_equal(m[1:4], xc) and np.array_equal(m[4:7], pc) and m[18] == np.float32(0.25)
    assert np.array_equal(m[7:16].reshape(3, 3), np.outer(xc, pc).astype(np.float32))
    assert abs(m[16] - float(xc.astype(np.float64) @ xc)) <= 2 * EPS32 * m[16] and abs(m[17] - float(pc.astype(np.float64) @ pc)) <= 2 * EPS32 * m[17]
    mv, mp = rs.randn(19).astype(np.float32), rs.randn(19).astype(np.float32)
    both = hr.combine(mv, mp, 0.25, 0.5)
    assert np.abs(both - (0.25 * mv.astype(np.float64) + 0.5 * mp)).max() <= 2 * EPS32 * 2
    # a skipped direction adds nothing, whatever its slots hold
    assert np.array_equal(hr.combine(mv, None, 0.25, 0.5), (np.float32(0.25) * mv).astype(np.float32))
    assert np.array_equal(hr.combine(None, mp, 0.25, 0.5), (np.float32(0.5) * mp).astype(np.float32))


def test_transform_chain_means_and_scan():
    rs = np.random.RandomState(9)
    x, p = rs.randn(300, 3).astype(np.float32), rs.randn(70, 3).astype(np.float32)
    T = np.concatenate([rc.axis_angle([1, 2, 3], 40.0), [[0.3], [-0.2], [0.1]]], 1).astype(np.float32)
    z = hr.apply(T, x)
    z64 = x.astype(np.float64) @ T[:, :3].astype(np.float64).T + T[:, 3]
    assert np.abs(z - z64).max() <= 4 * EPS32 * (np.abs(z64).max() + 1.0)
    assert np.abs(hr.means(x) - x.astype(np.float64).mean(0)).max() <= 16 * EPS32 * np.abs(x).max()
    assert np.array_equal(hr.means(x[:1]), x[0])
    # the scan: nearest by the term's own float32 d^2, the lowest index among equal ones
    p[40] = p[3]                                                     # a duplicate point: index 3 wins
    for direction, q, o in ((0, z, p), (1, p, z)):
        idx, d2 = hr.nearest(direction, T, x, p)
        ref_idx, ref_d2 = rc.nearest(q.astype(np.float64), o.astype(np.float64))
        assert np.abs(d2 - ref_d2).max() <= 8 * EPS32 * (ref_d2.max() + 1.0)
        same = idx == ref_idx
        # where float32 and float64 disagree the two candidates are as near as float32 can tell
        alt = ((q[~same].astype(np.float64) - o[idx[~same]].astype(np.float64)) ** 2).sum(1)
        assert np.all(np.abs(alt - ref_d2[~same]) <= 8 * EPS32 * (ref_d2.max() + 1.0))
        if direction == 0:
            assert 40 not in idx and 3 in idx


def test_one_float32_iteration_is_the_definition():
    c = rc.RECOVERY_CASES["cube5_skew15"]
    x, p = c["x"], c["p"]
    R0, t0 = rc.start_transform(rc.cube_rotations()[5], x.astype(np.float64), p.astype(np.float64))
    T0 = np.concatenate([R0, t0[:, None]], 1).astype(np.float32)
    o = hr.iterate(x, p, T0)
    R64, t64, cost64, kept64 = rc.iterate(x.astype(np.float64), p.astype(np.float64), T0[:, :3].astype(np.float64), T0[:, 3].astype(np.float64))
    assert o["kept"] == kept64 == 0
    assert abs(float(o["cost"]) - cost64) <= 64 * EPS32 * cost64
    Tn = o["T"].reshape(3, 4)
    assert rc.rotation_angle(Tn[:, :3], R64) <= 1e-5 and np.abs(Tn[:, 3] - t64).max() <= 1e-5
    # the start of the header: z = R (x - c_X) + c_P, the means summed as the header says
    Ts = hr.start_transform(rc.cube_rotations()[5], hr.means(x), hr.means(p)).reshape(3, 4)
    assert np.abs(Ts - T0).max() <= 16 * EPS32 * 2.0


# ---- the rules ------------------------------------------------------------------------------------------------------------------
def _good_block(keep):
    a = _lib.RigidAlignArgs()
    a.num_meshes, a.num_verts, a.num_points, a.num_starts, a.iterations = 2, 100, 90, 24, 5
    a.w_point = a.w_vert = 1.0
    for f in ("verts", "points", "transforms", "scores", "best", "best_transform", "kept_rotation"):
        setattr(a, f, 0x1000)
    return a


def test_every_refusal_in_its_order():
    keep = []
    a = _good_block(keep)
    assert hr.refusal(a) is None
    bad_R = np.eye(3, dtype=np.float32)[None].repeat(24, 0).copy()
    bad_R[7] *= 1.001
    # break everything at once, then mend one rule at a time: the first fault is the one worded
    a.struct_size += 4
    a.num_meshes, a.num_verts, a.num_points, a.num_starts, a.iterations = 5, 513, 0, 65, 1001
    a.w_point, a.w_vert = float("nan"), 0.0
    a.verts = None
    a.starts, a.start_transforms = bad_R.ctypes.data, 0x1000
    a.best = None
    steps = [
        ("struct_size does not match", lambda: setattr(a, "struct_size", C.sizeof(_lib.RigidAlignArgs))),
        ("num_meshes must be 1 .. the aligner's max_meshes", lambda: setattr(a, "num_meshes", 4)),
        ("num_verts must be 1 .. the aligner's max_verts", lambda: setattr(a, "num_verts", 512)),
        ("num_points must be 1 .. the aligner's max_points", lambda: setattr(a, "num_points", 1)),
        ("num_starts must be 1 .. the aligner's max_starts (at most 64)", lambda: setattr(a, "num_starts", 24)),
        ("iterations must be 0..1000", lambda: setattr(a, "iterations", 1000)),
        ("w_point and w_vert must be finite and >= 0", lambda: setattr(a, "w_point", 0.0)),
        ("w_point and w_vert are both 0", lambda: setattr(a, "w_vert", 2.0)),
        ("verts / points missing", lambda: setattr(a, "verts", 0x1000)),
        ("starts and start_transforms are both given", lambda: setattr(a, "start_transforms", None)),
        ("every start must be orthonormal to within 1e-4", lambda: setattr(a, "starts", None)),
        ("transforms / scores / best / best_transform / kept_rotation missing", lambda: setattr(a, "best", 0x1000)),
    ]
    for text, mend in steps:
        msg = hr.refusal(a)
        assert msg is not None and text in msg, (text, msg)
        mend()
    assert hr.refusal(a) is None
    # the built-in starts are 24
    a.num_starts = 23
    assert hr.refusal(a) == "the built-in starts are 24: num_starts must be 24 without starts"
    a.start_transforms = 0x1000           # ... unless the transforms are given
    assert hr.refusal(a) is None
    a.start_transforms, a.num_starts = None, 24
    # the handle's max_starts below 64
    assert "num_starts" in hr.refusal(a, max_starts=23)
    # negative weights, infinite weights, iterations < 0
    for field, value in (("w_vert", -1.0), ("w_point", float("inf")), ("iterations", -1), ("num_verts", 0), ("num_meshes", 0)):
        b = _good_block(keep)
        setattr(b, field, value)
        assert hr.refusal(b) is not None, field


def test_start_matrices():
    assert hr.start_refusal(np.eye(3)) is None
    R = rc.axis_angle([1, 2, 3], 77.0).astype(np.float32)           # a caller's float32 rotation is not exact: accepted
    assert hr.start_refusal(R) is None
    assert hr.start_refusal(np.diag([1.0, 1.0, -1.0])) == "every start must have determinant +1 (a reflection is no start)"
    assert hr.start_refusal(R * 1.001) == "every start must be orthonormal to within 1e-4"
    bad = R.copy()
    bad[1, 2] = np.nan
    assert hr.start_refusal(bad) == "every start must be finite"
    assert hr.start_refusal(R + np.float32(2e-5)) is None and hr.start_refusal(R + np.float32(2e-3)) is not None


def test_create_refusals_and_grids():
    assert hr.create_refusal(1, 1, 1, 1, 1) is None and hr.create_refusal(1, 32, 3889, 3000, 64) is None
    assert hr.create_refusal(0, 1, 1, 1, 1) == "null argument"
    for bad in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1)):
        assert hr.create_refusal(1, *bad) == "max_meshes, max_verts and max_points must be positive"
    assert hr.create_refusal(1, 1, 1, 1, 0) == hr.create_refusal(1, 1, 1, 1, 65) == "max_starts must be 1..64"
    assert hr.create_refusal(1, 65535, 1, 1, 1) is None and hr.create_refusal(1, 65536, 1, 1, 1) == "max_meshes must be at most 65535"
    g = hr.grids(3889, 3000, 24, 1, 30)
    assert g["scan_vert"] == (61, 24, 1) and g["scan_point"] == (47, 24, 1) and g["solve"] == (24, 1)
    assert g["init"] == 1 and g["pick"] == 1
    # the init, I + 1 rounds of (two scans, the solve), the pick
    assert g["launches"] == 1 + 31 * 3 + 1 and g["launches_one_direction"] == 1 + 31 * 2 + 1
    g = hr.grids(65, 64, 3, 70, 0)
    assert g["scan_vert"] == (2, 3, 70) and g["scan_point"] == (1, 3, 70) and g["pick"] == 2 and g["launches"] == 5
    k = hr.constants()
    assert k == dict(moments=19, sweeps=8, rank_eps=float(np.float32(1e-5)), cube_rotations=24, max_iterations=1000,
                     start_tolerance=float(np.float32(1e-4)), queries=64)
    assert rc.RANK_EPS == 1e-5


# ---- the block, the binding, the header -----------------------------------------------------------------------------------------
def test_struct_layout_matches_the_header(tmp_path):
    cls = _lib.RigidAlignArgs
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "smalfit.h"', "int main(void) {",
             'printf("sizeof %zu\\n", sizeof(smalfit_rigid_align_args));']
    for field, _ in cls._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(smalfit_rigid_align_args, %s));' % (field, field))
    lines += ["return 0; }"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = {a: int(b) for a, b in (ln.split() for ln in out.strip().splitlines())}
    assert got["sizeof"] == C.sizeof(cls) == hr.sizeof_args()
    assert [got[f] for f, _ in cls._fields_] == [getattr(cls, f).offset for f, _ in cls._fields_] == hr.offsets()
    assert _lib.RigidAlignArgs().struct_size == C.sizeof(cls)


def test_entry_points_are_bound_lazily_under_abi_version_6():
    text = open(HEADER).read()
    assert _lib.ABI_VERSION == 6 and re.search(r"#define SMALFIT_ABI_VERSION 6\b", text)
    for name in NEW_EXPORTS:
        assert name in _lib.SIGNATURES and name in _lib.LAZY_SYMBOLS
    assert _lib.SIGNATURES["smalfit_rigid_align"][1][-1]._type_ is _lib.RigidAlignArgs
    declared = set(re.findall(r"\b(smalfit_[a-z_0-9]+)\s*\(", text))
    assert {n for n in declared if n.startswith("smalfit_rigid_")} == set(NEW_EXPORTS)          # exactly three, no token of a comment among them
    # none takes an engine or a mesh objective first: the aligner is a handle of its own
    firsts = set(re.findall(r"\b(smalfit_\w+)\s*\(\s*(?:const\s+)?(?:struct\s+)?smalfit_(?:engine|mesh_objective)\s*\*", text))
    assert not firsts & set(NEW_EXPORTS)
    assert _lib.MAX_RIGID_STARTS == 64 == int(re.search(r"#define SMALFIT_MAX_RIGID_STARTS (\d+)", text).group(1))
    assert _lib.NUM_CUBE_ROTATIONS == 24 == int(re.search(r"#define SMALFIT_NUM_CUBE_ROTATIONS (\d+)", text).group(1))


def test_built_in_starts_are_the_rotation_group_of_the_cube():
    cube = hr.cube_rotations().astype(np.float64)
    assert cube.shape == (24, 3, 3)
    assert np.array_equal(cube, rc.cube_rotations())                    # the header's order, restated independently
    assert np.array_equal(cube[0], np.eye(3))
    keys = {tuple(R.reshape(-1).astype(int)) for R in cube}
    assert len(keys) == 24                                              # distinct
    for R in cube:
        assert np.array_equal(np.abs(R).sum(0), np.ones(3)) and np.array_equal(np.abs(R).sum(1), np.ones(3))   # signed permutations
        assert np.linalg.det(R) == pytest.approx(1.0, abs=1e-12)
        assert hr.start_refusal(R) is None
    for A in cube:                                                      # closed under multiplication (and so under inverses)
        for B in cube:
            assert tuple((A @ B).reshape(-1).astype(int)) in keys
    assert np.array_equal(hr.cube_rotation(24), np.eye(3)) and np.array_equal(hr.cube_rotation(-1), np.eye(3))


# ---- the cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rc.RECOVERY_CASES))
def test_recovery_case_is_admitted(name):
    """the float64 restatement alone, from the 24 built-in starts and the same iterations, recovers R* (and t*): a case where it
    lands elsewhere would prove nothing about the kernels"""
    c = rc.RECOVERY_CASES[name]
    ref = rc.reference(name)
    b = ref["best"]
    angle = rc.rotation_angle(ref["R"][b], c["R"])
    print(name, "best", b, "angle", angle, "score", ref["scores"][b])
    assert angle <= rc.RECOVERY_ADMISSION
    assert np.abs(ref["t"][b] - c["t"]).max() <= rc.RECOVERY_ADMISSION * (1.0 + c["extent"])
    assert ref["kept"].sum() == 0 and np.isfinite(ref["history"]).all()
    # no rotational symmetry: the winner's rotation is R*, and every start that ends elsewhere scores clearly worse
    others = [k for k in range(24) if rc.rotation_angle(ref["R"][k], c["R"]) > 1e-3]
    assert others and min(ref["scores"][k] for k in others) > 1e-3
    if name == "back_to_front":
        assert ref["scores"][0] > 1e-3          # the identity start settles back to front


def test_rank_deficient_sets_of_the_cases():
    x = rc.lopsided_blob().astype(np.float64)
    for p in (rc.coincident_points(), rc.collinear_points()):
        R0, t0 = rc.start_transform(np.eye(3), x, p.astype(np.float64))
        R, t, cost, kept = rc.iterate(x, p.astype(np.float64), R0, t0)
        assert kept == 1 and np.array_equal(R, R0) and np.isfinite(t).all()
        T0 = np.concatenate([R0, t0[:, None]], 1).astype(np.float32)
        o = hr.iterate(x.astype(np.float32), p, T0)
        assert o["kept"] == 1 and np.isfinite(o["T"]).all() and np.array_equal(o["T"].reshape(3, 4)[:, :3], T0[:, :3])
