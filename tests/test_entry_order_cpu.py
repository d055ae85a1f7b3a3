"""The books of the entry-order matrix (tests/entry_order_cases.py), without a GPU: every entry point with an engine or a
mesh-objective handle is reached or excluded by name; the two scenes are as foreign to each other as the GPU tests assume; the
table and its inputs are deterministic."""
import importlib
import os
import re

import numpy as np
import torch

from oracle import smal_oracle as so
from smalify_amd import _lib
from tests import entry_order_cases as oc
from tests import fold_forms as ff
from tests import parity_cases as pc

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "smalfit.h")


def _handle_entry_points():
    """the functions include/smalfit.h declares with an engine or a mesh objective as their first argument"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"\b(smalfit_\w+)\s*\(\s*(?:const\s+)?(?:struct\s+)?smalfit_(?:engine|mesh_objective)\s*\*", text))


def test_every_entry_point_with_a_handle_is_in_the_matrix_or_excluded_by_name():
    declared = _handle_entry_points()
    assert len(declared) >= 35 and {"smalfit_fit_eval", "smalfit_mesh_score", "smalfit_fit3d_step_robust"} <= declared
    assert declared <= set(_lib.SIGNATURES), sorted(declared - set(_lib.SIGNATURES))
    reached = set(oc.HARNESS_CALLS) | set(oc.MESH_HARNESS_CALLS)
    for act in list(oc.ACTS.values()) + list(oc.MESH_ACTS.values()):
        reached |= set(act.calls)
    assert reached <= set(_lib.SIGNATURES), sorted(reached - set(_lib.SIGNATURES))
    both = reached & set(oc.EXCLUDED)
    assert not both, "reached AND excluded: %s" % sorted(both)
    missing = declared - reached - set(oc.EXCLUDED)
    assert not missing, ("entry points that take a handle and are neither reached by an act of tests/entry_order_cases.py nor "
                         "excluded there with a reason: %s" % sorted(missing))
    stale = set(oc.EXCLUDED) - declared
    assert not stale, "excluded but not declared with a handle: %s" % sorted(stale)
    assert all(isinstance(r, str) and len(r) > 10 and "\n" not in r for r in oc.EXCLUDED.values())


def test_the_table_names_what_the_issue_lists():
    kinds = [a.kind for a in oc.ACTS.values()]
    assert kinds.count("refusal") == 3 and kinds.count("rows") == 2 and len(oc.NAMES) == len(set(oc.NAMES)) >= 30
    assert set(oc.CACHED) == {n for n, a in oc.ACTS.items() if a.kind in ("eval", "rows", "render")}
    assert "run 3" not in oc.CACHED and "eval Y8" in oc.CACHED and "render backward" in oc.CACHED
    assert oc.SCENE_ARGS["Y8"][0] == oc.MAX_FRAMES                     # frames 4 .. 7 leave state a 4-frame call never touches
    for batch in oc.MESH_BATCHES:
        for head in ("eval chamfer,", "eval gated,", "eval robust,", "eval chamfer off,", "score", "surface plain,", "surface robust,",
                     "surface correspondences,"):
            assert any(n.startswith(head) and batch in n for n in oc.MESH_NAMES), (head, batch)
    assert any("S=1," in n for n in oc.MESH_NAMES) and any("S=%d," % oc.MESH_POINTS in n for n in oc.MESH_NAMES)
    assert any("indexed" in n for n in oc.MESH_NAMES) and any("linear" in n for n in oc.MESH_NAMES)


def test_the_fold_plan_takes_and_refuses_the_layouts_the_runs_are_named_for():
    mode, offs, ranges, grad_at = oc.refused_layout(4)
    ok, _, why = ff.plan_fold(4, mode, offs, ranges, grad_at)
    assert not ok and why
    ok, train, _ = ff.plan_fold(4, mode, offs, ranges, dict.fromkeys(offs, True))
    assert ok and all(train.values())
    for K in (3, 4):                                                   # odd and even: the last prior slot differs
        assert ff.path(K, False, False, True, True) == "folded"
    assert ff.prior_slot(2) != ff.prior_slot(3)
    assert ff.path(1, False, False, True, True) == "plain" and ff.path(3, False, False, True, False) == "plain"
    assert ff.path(3, True, False, False, True) == "graph"             # 'run graph': the switch on, a side stream


def _iou(a, b):
    a, b = a > 0.5, b > 0.5
    return float((a & b).sum()) / float((a | b).sum())


def test_the_two_scenes_are_foreign_to_each_other():
    """float64 oracle, M = 4: the target silhouettes of X and Y overlap with an IoU of 0.14 .. 0.18 per frame, and X is the larger"""
    _, _, x = pc.make_problem_cpu(4, oc.S, oc.WINDOW, seed=oc.SCENE_ARGS["X4"][1], z=oc.SCENE_ARGS["X4"][2])
    _, _, y = pc.make_problem_cpu(4, oc.S, oc.WINDOW, seed=oc.SCENE_ARGS["Y8"][1], z=oc.SCENE_ARGS["Y8"][2])
    assert np.array_equal(x["tsil"], oc.scene("X4")["tg"]["tsil"])
    for n in range(4):
        assert _iou(x["tsil"][n], y["tsil"][n]) < 0.5, n
        assert 0.1 < _iou(x["tsil"][n], y["tsil"][n]) < 0.2, n
        assert x["tsil"][n].sum() > y["tsil"][n].sum() > 0, n
    assert x["tsil"].sum() >= 3 * y["tsil"].sum()                      # 5290 pixels against 1040: X's area is five times Y's
    assert [int(t.sum()) for t in x["tsil"]] == [1252, 953, 1711, 1374] and [int(t.sum()) for t in y["tsil"]] == [249, 325, 253, 213]
    # ... and the evaluated poses too: what the depth cache holds is the render, not the target
    sx = so.soft_silhouette(torch.from_numpy(oc.scene("X4")["verts"]).double(), pc.get_oracle_model()[1].faces, oc.S).numpy()
    sy = so.soft_silhouette(torch.from_numpy(oc.scene("Y8")["verts"][:4]).double(), pc.get_oracle_model()[1].faces, oc.S).numpy()
    for n in range(4):
        assert _iou(sx[n], sy[n]) < 0.5, n


def test_scene_y_overflows_the_k_nearest():
    """the oracle hands out the largest number of candidate faces at a pixel, not a count per pixel: Y (head-on) exceeds K = 100 in
    every batch the acts render.  So does the first frame of X at 64 x 64 (388 candidates where the legs and the head pile up): the
    K-cut is reached from both scenes, and what sets them apart is where on the screen their bounds lie, not whether they overflow"""
    faces = pc.get_oracle_model()[1].faces
    K = so.FACES_PER_PIXEL
    _, stats_y = so.soft_silhouette(torch.from_numpy(oc.scene("Y8")["verts"]).double(), faces, oc.S, return_stats=True)
    _, stats_y3 = so.soft_silhouette(torch.from_numpy(oc.scene("Y3")["verts"]).double(), faces, oc.S, return_stats=True)
    _, stats_x = so.soft_silhouette(torch.from_numpy(oc.scene("X4")["verts"][:1]).double(), faces, oc.S, return_stats=True)
    assert stats_y["max_faces_per_pixel"] > K and stats_y3["max_faces_per_pixel"] > K
    assert stats_x["max_faces_per_pixel"] > 0
    print("largest candidate count at a pixel: Y8 %d, Y3 %d, first frame of X %d" % (
        stats_y["max_faces_per_pixel"], stats_y3["max_faces_per_pixel"], stats_x["max_faces_per_pixel"]))


def test_the_table_and_its_inputs_are_deterministic():
    def digest(mod):
        d = dict(mod.all_inputs())
        d.update({"mesh/" + k: v for k, v in mod.mesh_inputs().items()})
        return {k: (v.dtype.str, v.shape, v.tobytes()) for k, v in d.items()}

    first = (oc.NAMES, oc.MESH_NAMES, oc.CACHED, digest(oc))
    again = importlib.reload(oc)
    assert not again._SCENES and not again._MESH and not again._AUX      # the second import made its inputs anew
    second = (again.NAMES, again.MESH_NAMES, again.CACHED, digest(again))
    assert first[:3] == second[:3]
    assert set(first[3]) == set(second[3]) and len(first[3]) > 60
    for k in first[3]:
        assert first[3][k] == second[3][k], k
    assert all(np.isfinite(np.frombuffer(v[2], np.float32)).all() for k, v in first[3].items() if v[0] == "<f4")
