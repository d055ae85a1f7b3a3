"""The LBS and fit kernels on models unlike the stand-in (-m gpu): the variants of tests/model_forms.py -- other kinematic
trees (the table-driven walks of pose_block and chain_bwd_kernel, the fast walk at its limits), vertices of valence 9 to 40
and vertices without a face, 1 to 9 skinning weights per vertex, other regressor sparsity, other vertex counts and other
numbers of shape directions -- against the float64 oracle on the same variant, frame by frame
(tests/test_model_forms_cpu.py proves on the host which branch each variant reaches).

Bounds are those of tests/test_gpu_frame_counts.py: LBS values 2e-5, LBS gradients 5e-4, fit total 1e-4, fit gradients 2e-3,
d/d verts of the silhouette 1e-2 (tests/test_gpu_parity.py).  On the trees deeper than SMAL's (a product of up to 34 float32
transforms) the bar is the larger of that and YARD = 2 x the float32 ORACLE's own deviation from the float64 one on the same
inputs, computed here on the CPU.  With tests/golden/hip_model_forms_measured.json present every deviation also stays within
RATCHET = 3 x what these kernels measured when the file was written (floors 1e-6 on values, 1e-5 on gradients);
SMALFIT_WRITE_MODEL_MEASURED=<path> writes them.  Every number is printed past the capture."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import smal_oracle as so                 # noqa: E402
from smalify_amd import _lib                         # noqa: E402
from smalify_amd import engine as eng                # noqa: E402
from smalify_amd import synthetic                    # noqa: E402
from tests import model_forms as mf                  # noqa: E402
from tests import parity_cases as pc                 # noqa: E402
from tests import value_forms as vf                  # noqa: E402
from tests.test_gpu_frame_counts import assert_per_frame, frame_errors    # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
MEASURED = os.path.join(HERE, "golden", "hip_model_forms_measured.json")
VALUE_TOL, GRAD_TOL = 2e-5, 5e-4
VALUES = ("verts", "joints", "Rs", "vshaped")
GRADS = ("dbeta", "dtheta", "dls")
S_IMG = 64


class Table:
    """the printed table of one test, its bound and ratchet checks, and the record of what was measured (the layout and the
    rule of tests/test_gpu_value_forms.py: Table, on a file of its own)"""

    def __init__(self, title):
        self.title, self.lines, self.bad, self.measured = title, [], [], {}
        self.recorded = json.load(open(MEASURED)) if os.path.exists(MEASURED) else {}

    def add(self, key, err, bar, gradient, yard=None):
        limit = bar if yard is None else max(bar, vf.YARD * yard)
        line = "%-52s hip %.2e  %s bound %.1e" % (key, err, "" if yard is None else "(f32 oracle %.2e) " % yard, limit)
        self.lines.append(line)
        self.measured[key] = max(self.measured.get(key, 0.0), float(err))
        if not err <= limit:
            self.bad.append(line)
        floor = vf.FLOOR_GRAD if gradient else vf.FLOOR_VALUE
        if key in self.recorded and err > max(vf.RATCHET * self.recorded[key], floor):
            self.bad.append(line + "   [ratchet: %.1f x the recorded %.2e]" % (err / max(self.recorded[key], 1e-300), self.recorded[key]))

    def close(self, capsys):
        with capsys.disabled():
            print("\n[%s: HIP vs float64 oracle]\n" % self.title + "\n".join(self.lines))
        path = os.environ.get("SMALFIT_WRITE_MODEL_MEASURED")
        if path:
            doc = json.load(open(path)) if os.path.exists(path) else {}
            doc.update(self.measured)
            json.dump(doc, open(path, "w"), indent=1, sort_keys=True)
        assert not self.bad, "\n".join(self.bad)
        assert self.recorded, "tests/golden/hip_model_forms_measured.json is missing: run this file with SMALFIT_WRITE_MODEL_MEASURED=<path> on a GPU box and commit the result"
        missing = [k for k in self.measured if k not in self.recorded]
        assert not missing, "not in tests/golden/hip_model_forms_measured.json: %s" % missing


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """a device error ends the session: nothing more is started on a GPU that has just faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:
        pytest.exit("device error, stopping: %s" % exc, returncode=3)


_LAST = {}


def model(name):
    """(model description, device model) of a variant; the one before it is let go (the cases come variant by variant)"""
    if _LAST.get("name") != name:
        _LAST.clear()
        md = mf.variant(name)
        _LAST.update(name=name, md=md, dm=eng.DeviceModel(md), engines={})
    return _LAST["md"], _LAST["dm"]


def engine(name, max_frames, priors=False):
    md, dm = model(name)
    key = (max_frames, priors)
    if key not in _LAST["engines"]:
        e = eng.Engine(dm, max_frames, S_IMG)
        if priors:
            e.set_pose_prior(*synthetic.synthetic_pose_prior())
            e.set_shape_prior(*synthetic.synthetic_shape_prior())
        _LAST["engines"][key] = e
    return md, _LAST["engines"][key]


def hip_lbs(e, x):
    d = {k: pc.dev(v) for k, v in x.items()}
    v, j, Rs, vs = e.lbs_forward(d["beta"], d["theta"], d["ls"])
    db, dt, dl = e.lbs_backward(d["beta"], d["theta"], d["ls"], d["wv"], d["wj"])
    out = dict(verts=v, joints=j, Rs=Rs, vshaped=vs, dbeta=db, dtheta=dt, dls=dl)
    return {k: t.cpu().numpy() for k, t in out.items()}


# ---- LBS forward and backward ----------------------------------------------------------------------------------------
LBS_CASES = mf.lbs_cases()


@pytest.mark.parametrize("name,M,nb", LBS_CASES, ids=["%s-M%d-nb%d" % c for c in LBS_CASES])
def test_lbs_matches_oracle_per_frame(name, M, nb, capsys):
    md, e = engine(name, max(m for n, m, _ in LBS_CASES if n == name))
    x = mf.lbs_inputs(M, nb, md.v_template.shape[0], seed=len(name) + M)
    got, want = hip_lbs(e, x), mf.oracle_lbs(md, x)
    assert e.status() == 0
    f32 = mf.oracle_lbs(md, x, torch.float32) if name in mf.DEEP_TREES else None
    table = Table("LBS on %s, %d frames, %d shape directions" % (name, M, nb))
    for k in VALUES + GRADS:
        assert np.isfinite(got[k]).all(), k
        yard = None if f32 is None else float(frame_errors(f32[k], want[k]).max())
        table.add("lbs/%s/M%d/%s" % (name, M, k), float(frame_errors(got[k], want[k]).max()), VALUE_TOL if k in VALUES else GRAD_TOL,
                  k in GRADS, yard)
    # what a norm over a frame can hide: the joint without vertices, the landmark without faces, the hubs
    f = mf.facts(md)
    for j in sorted(set(f["unskinned_joints"] + f["unregressed_joints"])):
        if j in f["unregressed_joints"]:
            assert (want["joints"][:, j] == 0).all() and (got["joints"][:, j] == 0).all(), "the joint with an empty regressor row"
        table.add("lbs/%s/M%d/joints_row%d" % (name, M, j), float(mf.row_errors(got["joints"], want["joints"])[:, j].max()), VALUE_TOL, False)
        table.add("lbs/%s/M%d/dtheta_row%d" % (name, M, j), float(mf.row_errors(got["dtheta"], want["dtheta"])[:, j].max()), GRAD_TOL, True)
    if name == "valence":
        rows = [35 + so.LANDMARKS.index(v) for v in (mf.HUB_LANDMARK, mf.ISOLATED_LANDMARK)]
        table.add("lbs/valence/M%d/landmark_rows" % M, float(mf.row_errors(got["joints"], want["joints"])[:, rows].max()), VALUE_TOL, False)
        sel = list(mf.valence_facts()[1])
        table.add("lbs/valence/M%d/isolated_verts" % M, float(mf.row_errors(got["verts"], want["verts"])[:, sel].max()), VALUE_TOL, False)
    if nb > mf.FIT_BETAS:
        # d/d betas element by element: the directions past the 20th are the small ones of a frame's row
        table.add("lbs/%s/M%d/dbeta_elements" % (name, M), float(mf.row_errors(got["dbeta"][..., None], want["dbeta"][..., None]).max()),
                  GRAD_TOL, True)
    table.close(capsys)


def test_a_model_of_65_shape_directions_is_refused_before_any_launch():
    """chain_bwd_kernel reduces d/d betas through the rest joints with one lane of a wave per direction: a 65th would read what
    another launch left in LDS.  Such a model is refused by smalfit_model_create, with the limit in the message"""
    with pytest.raises(_lib.SmalfitError, match="smalfit_model_create: num_betas above 64 is not supported"):
        eng.DeviceModel(mf.variant("nb65"))
    torch.cuda.synchronize()


# ---- stand-alone chain operators -------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", (1, 257))
@pytest.mark.parametrize("name", ("chain", "star", "five_children"))
def test_global_rigid_transformation_on_other_trees(name, count, capsys):
    parents = np.asarray(mf.tree_parents(name), np.int32)
    table = Table("smalfit_global_rigid_transformation on %s, %d" % (name, count))
    for scale in (None, 0.3):
        c = vf.chain_case(count, scale)
        Rs, Js, ls = pc.dev(c["Rs"]), pc.dev(c["Js"]), None if scale is None else pc.dev(c["ls"])
        newJ, A = eng.global_rigid_transformation(Rs, Js, parents, ls)
        dRs, dJs, dls = eng.global_rigid_transformation_backward(Rs, Js, parents, ls, pc.dev(c["dnewJ"]), pc.dev(c["dA"]))
        got = dict(newJ=newJ, A=A, dRs=dRs, dJs=dJs)
        if ls is not None:
            got["dls"] = dls
        r64, r32 = vf.chain_oracle(c, parents), vf.chain_oracle(c, parents, torch.float32)
        assert set(got) == set(r64)
        for k in r64:
            g = got[k].cpu().numpy().astype(np.float64)
            assert np.isfinite(g).all()
            table.add("chain/%s/scale_%s/count%d/%s" % (name, "none" if scale is None else "%g" % scale, count, k), vf.rel(g, r64[k]),
                      vf.BAR["chain"], k.startswith("d"), vf.rel(r32[k], r64[k]))
    table.close(capsys)


# ---- fused evaluation ------------------------------------------------------------------------------------------------
def _fit_eval(e, cur, tg, names):
    weights, w_temp = mf.fit_weights()
    d = {k: pc.dev(v) for k, v in cur.items()}
    losses, grads = e.fit_eval(betas=d["betas"], log_beta_scales=d["log_beta_scales"], global_rotation=d["global_rotation"],
                               joint_rotations=d["joint_rotations"], trans=d["trans"], target_joints=pc.dev(tg["tj"]),
                               target_visibility=pc.dev(tg["vis"]), target_sil=pc.dev(tg["tsil"]), weights=weights, w_temp=w_temp,
                               window=mf.FIT_WINDOW, want=names)
    assert e.status() == 0
    return losses.cpu().numpy().astype(np.float64), {k: g.cpu().numpy().astype(np.float64) for k, g in grads.items()}


@pytest.mark.parametrize("name", mf.FIT_VARIANTS)
def test_fit_eval_matches_oracle_per_frame(name, capsys):
    """smalfit_fit_eval with shared betas and the silhouette on, three frames in windows of two, stage 2: the nine loss terms'
    sum and every gradient, the per-frame ones frame by frame"""
    md, e = engine(name, 8, priors=True)
    prob, cur, tg = mf.fit_problem(md)
    total, _, want = mf.oracle_fit(prob, cur)
    names = so.trainable_names(mf.FIT_STAGE)
    e.reset_raster_cache()
    losses, got = _fit_eval(e, cur, tg, names)
    table = Table("smalfit_fit_eval on %s" % name)
    table.add("fit/%s/total" % name, abs(losses.sum() - total) / abs(total), mf.FIT_TOTAL_TOL, False)
    for k in names:
        g = got[k].reshape(want[k].shape)
        assert np.isfinite(g).all(), k
        table.add("fit/%s/%s" % (name, k), pc.rel(g, want[k]), mf.FIT_GRAD_TOL, True)
        if k in mf.PER_FRAME:
            table.add("fit/%s/%s/per_frame" % (name, k), float(frame_errors(g, want[k]).max()), mf.FIT_GRAD_TOL, True)
    table.close(capsys)


def test_the_fitter_refuses_a_model_of_12_shape_directions():
    """the fitter optimises 20 shape directions whatever the model holds: with 12 the head kernels would read the model's
    tables past their rows.  smalfit_fit_eval and smalfit_fit_run refuse the model before any launch, with the count in the
    message; the LBS entry points take it (test_lbs_matches_oracle_per_frame, nb12)"""
    from tests import fold_forms as ff
    md, e = engine("nb12", 8, priors=True)
    M = mf.FIT_FRAMES
    cur = pc.random_pose(M, 21)
    d = {k: pc.dev(v) for k, v in cur.items()}
    tj, vis, tsil = torch.zeros(M, 25, 2, device="cuda"), torch.ones(M, 25, device="cuda"), torch.zeros(M, S_IMG, S_IMG, device="cuda")
    weights, w_temp = mf.fit_weights()
    why = "the model has fewer than the 20 shape directions the fitter optimises"
    with pytest.raises(_lib.SmalfitError, match="smalfit_fit_eval: " + why):
        e.fit_eval(betas=d["betas"], log_beta_scales=d["log_beta_scales"], global_rotation=d["global_rotation"],
                   joint_rotations=d["joint_rotations"], trans=d["trans"], target_joints=tj, target_visibility=vis, target_sil=tsil,
                   weights=weights, w_temp=w_temp, window=mf.FIT_WINDOW)
    offs, size = ff.layout(M, 1, None, 0)
    flat, grad, m, v = (torch.zeros(size, device="cuda") for _ in range(4))
    shapes = dict(betas=(20,), log_beta_scales=(6,), global_rotation=(M, 3), joint_rotations=(M, 34, 3), trans=(M, 3))
    p = {k: flat[o:o + c].view(shapes[k]) for k, (o, c) in offs.items()}
    g = {k: grad[o:o + c].view(shapes[k]) for k, (o, c) in offs.items()}
    for k in p:
        p[k].copy_(d[k])
    before = flat.clone()
    a, _, _, keep = e.build_fit_args(betas=p["betas"], log_beta_scales=p["log_beta_scales"], global_rotation=p["global_rotation"],
                                     joint_rotations=p["joint_rotations"], trans=p["trans"], target_joints=tj, target_visibility=vis,
                                     target_sil=tsil, weights=weights, w_temp=w_temp, window=mf.FIT_WINDOW, grads=g, want=ff.TENSORS)
    aa = eng.make_adam_args(flat, grad, m, v, ff.merged_ranges(offs, ff.TENSORS), 1e-3)
    for graph in (False, True):
        e.set_graph(graph)
        try:
            with pytest.raises(_lib.SmalfitError, match="smalfit_fit_run: " + why):
                e.fit_run(a, aa, 3)
        finally:
            e.set_graph(False)
    torch.cuda.synchronize()
    assert torch.equal(flat, before) and not grad.any() and not m.any() and e.status() == 0
    del keep


# ---- the silhouette's adjoint, vertex by vertex ----------------------------------------------------------------------
def test_silhouette_adjoint_per_vertex_on_valence(capsys):
    """smalfit_render_backward gathers a vertex's adjoint from its incident corners: the hubs (9, 9, 16, 17 and 40 of them: past
    the eight held in registers) and the vertices without any, each against the oracle's row"""
    md, e = engine("valence", 8, priors=True)
    hubs, isolated = mf.valence_facts()
    verts, w = mf.render_case(md)
    want = mf.oracle_render_grad(md, verts, w)
    e.reset_raster_cache()
    v = pc.dev(verts)
    sil, _ = e.render_forward(v)
    got = e.render_backward(v, sil, pc.dev(w)).cpu().numpy().astype(np.float64)
    assert e.status() == 0 and np.isfinite(got).all()
    table = Table("smalfit_render_backward on valence")
    table.add("render/valence/dverts", pc.rel(got, want), mf.RENDER_TOL, True)
    err = mf.row_errors(got, want)
    for h, (_, n) in zip(hubs, mf.HUBS):
        table.add("render/valence/hub%d_valence%d" % (h, n), float(err[:, h].max()), mf.RENDER_TOL, True)
    assert np.linalg.norm(want[:, list(hubs)], axis=-1).max() > np.sqrt((np.linalg.norm(want, axis=-1) ** 2).mean()), "no hub has a gradient"
    assert (want[:, list(isolated)] == 0).all() and (got[:, list(isolated)] == 0).all(), "a vertex without a face has a gradient"
    table.close(capsys)


# ---- the folded step and the image batch on the table-driven walk ------------------------------------------------------
def _fitter_on(name, seed):
    """tests/test_gpu_fold_step.py: _small_fitter (8 frames at 64^2, shared limb scales, the 26-dim prior) on a variant"""
    from smalify_amd import fitter as fit
    md, e = engine(name, 8, priors=True)
    _, cur, tg = pc.make_problem_cpu(8, S_IMG, 4, seed, model=(md, so.OracleModel(md)))

    def new_fitter():
        e.reset_raster_cache()
        f = fit.FusedFitter(e, tg["tj"], tg["vis"], tg["tsil"], 4, True, cur["betas"], cur["log_beta_scales"])
        for k in ("global_rotation", "joint_rotations", "trans"):
            f.p[k].copy_(pc.dev(cur[k]))
        return f
    return e, new_fitter


@pytest.mark.parametrize("name", ("chain", "five_children"))
def test_folded_step_on_the_table_driven_walk(name):
    """lbs_head_step_kernel has its own copy of the table-driven walk: three iterations in one call (folded), through the
    captured graph and as three calls of one (the plain chain) leave the same bits, as
    tests/test_gpu_fold_step.py::test_one_call_of_k_iterations_equals_k_calls_of_one and
    ::test_graph_switch_and_profiled_run_give_the_same_state demand of the stand-in"""
    from tests import test_gpu_fold_step as fs
    K, calls = 3, ((0, True), (2, True))
    e, new_fitter = _fitter_on(name, 41)
    ref = fs._run_calls(new_fitter(), K, whole=False, calls=calls)
    got = fs._run_calls(new_fitter(), K, whole=True, calls=calls)
    assert e.status() == 0
    for (stage, _), a, b in zip(calls, ref, got):
        fs._assert_same(a, b, "%s folded, stage %d" % (name, stage))
    assert np.count_nonzero(got[-1]["exp_avg"]) > got[-1]["exp_avg"].size // 2
    side = torch.cuda.Stream()
    e.set_graph(True)
    try:
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            graphed = fs._run_calls(new_fitter(), K, whole=True, calls=calls)
            side.synchronize()
    finally:
        e.set_graph(False)
    for (stage, _), a, b in zip(calls, ref, graphed):
        fs._assert_same(a, b, "%s graph, stage %d" % (name, stage))
    assert e.status() == 0


def test_independent_images_on_the_table_driven_walk(monkeypatch, capsys):
    """lbs_head_images_kernel on `chain`: one subject_frames = 1 evaluation of three images against each image's own
    one-frame oracle problem, as tests/test_gpu_image_batch.py::test_one_evaluation_matches_the_oracle_per_image"""
    from tests import image_batch_cases as ic
    from tests import test_gpu_image_batch as ib
    md, e = engine("chain", 8, priors=True)
    monkeypatch.setattr(pc, "get_oracle_model", lambda dense=False: (md, so.OracleModel(md)))
    N = 3
    images = ic.make_images(N, S_IMG)
    states = [im["near"] for im in images]
    e.reset_raster_cache()
    losses, rows, grads = ib._batch_eval(e, ic.stack(states), ic.targets(images), 2)
    lines, bad = [], []
    ib._check_against_oracle("chain N=%d" % N, images, states, rows, grads, 2, lines, bad)
    with capsys.disabled():
        print("\n[image batch on chain: HIP vs float64 oracle per image]\n" + "\n".join(lines))
    assert not bad, "\n".join(bad)
