"""raster_sweep_kernel forms its faces' records, boxes, union boxes and the frame's reference depth itself (-m gpu): one
evaluation against the float64 oracle at the shapes where that prologue and the launch's grid take another path.

Models: the stand-in with its face list cut to a connected patch (the way tests/model_forms.py cuts its variants) of
  25 faces    fewer than 32: one sweep block per frame, its last three union boxes partial or empty;
  1003 faces  a multiple of neither 8 nor 32: the last union box holds 3 faces, the last sweep block 11.
Frames: 1, 7 and 9 -- the grid is padded to 8 or 16 frames, whose workgroups must store nothing.  From 7 frames on one frame is
translated wholly off screen and one wholly behind the camera (every record culled, the active region empty), between
ordinary frames.  Image size 64.

The joint riders of the launch exist exactly when the evaluation is smalfit_fit_eval with the silhouette on (they regress the
joints the keypoint term reads); smalfit_render_forward / smalfit_render_backward launch the sweep without them.  Both are
checked, the fit with and without the keypoint weight.

Bounds are those of tests/test_gpu_raster_forms.py for SMAL poses: silhouette 2e-3 per pixel, gradients 1e-2 rel-L2; the
silhouette term, a weighted mean of |sil - target|, by the silhouette bound over the pixels the scene reaches (that file's
rule); the other eight terms do not pass through the rasteriser: GRAD_TOL = 1e-3 of that file relative to the term, with the
silhouette term's bound as the floor.  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import smal_oracle as so                 # noqa: E402
from smalify_amd import engine as eng                # noqa: E402
from smalify_amd import synthetic                    # noqa: E402
from tests import model_forms as mf                  # noqa: E402
from tests import parity_cases as pc                 # noqa: E402
from tests import raster_forms as rf                 # noqa: E402

S = 64
WINDOW = 2
MAX_FRAMES = 16
FACE_COUNTS = (25, 1003)
FRAME_COUNTS = (1, 7, 9)
SIL_TOL, GRAD_TOL = 2e-3, 1e-2          # tests/test_gpu_raster_forms.py: test_image_sizes_with_the_stand_in
TERM_TOL = 1e-3                         # tests/test_gpu_raster_forms.py: GRAD_TOL
OFF_SCREEN, BEHIND = 2, 4               # frames of a problem of 7 or more
SEED_VERTEX = 2000                      # a vertex of the stand-in's flank: the patch grows from it

_CACHE = {}


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """a device error ends the session: nothing more is started on a GPU that has just faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:
        pytest.exit("device error, stopping: %s" % exc, returncode=3)


def patch_model(F):
    """the stand-in with the F faces nearest (in rings of shared vertices) to SEED_VERTEX; every vertex stays"""
    if ("md", F) not in _CACHE:
        md = mf.base()
        faces = np.asarray(md.faces)
        seen, front, picked = {SEED_VERTEX}, {SEED_VERTEX}, []
        taken = np.zeros(len(faces), bool)
        while len(picked) < F:
            hit = np.flatnonzero(~taken & np.isin(faces, list(front)).any(1))
            assert len(hit), "the patch ran out of faces"
            taken[hit] = True
            picked += [int(i) for i in hit]
            nxt = set(int(v) for v in faces[hit].reshape(-1)) - seen
            seen |= nxt
            front = nxt
        out = mf._take_verts(md, np.arange(md.v_template.shape[0]), faces[np.asarray(picked[:F])])
        assert len(out.faces) == F and F % 8 != 0
        _CACHE["md", F] = (out, so.OracleModel(out))
    return _CACHE["md", F]


def engine(F):
    if ("engine", F) not in _CACHE:
        md, _ = patch_model(F)
        e = eng.Engine(eng.DeviceModel(md), MAX_FRAMES, S)
        e.set_pose_prior(*synthetic.synthetic_pose_prior())
        e.set_shape_prior(*synthetic.synthetic_shape_prior())
        _CACHE["engine", F] = e
    return _CACHE["engine", F]


def problem(F, M):
    """(oracle problem, parameters, targets) of tests/parity_cases.py: make_problem_cpu on the patch model, with the two
    special frames from 7 frames on"""
    if ("problem", F, M) not in _CACHE:
        prob, cur, tg = pc.make_problem_cpu(M, S, WINDOW, model=patch_model(F))
        if M > BEHIND:
            cur["trans"][OFF_SCREEN, 0] += 6.0                       # x_ndc far beyond the image on every vertex
            cur["trans"][BEHIND, 2] = so.CAM_DIST + 1.5              # z_view < 0 on every vertex
        _CACHE["problem", F, M] = (prob, cur, tg)
    return _CACHE["problem", F, M]


def posed(om, cur):
    M = cur["trans"].shape[0]
    theta = np.concatenate([cur["global_rotation"][:, None], cur["joint_rotations"]], 1)
    with torch.no_grad():
        vo, _, _, _ = so.smal_forward(om, torch.from_numpy(np.tile(cur["betas"], (M, 1))).double(), torch.from_numpy(theta).double(),
                                      torch.from_numpy(np.tile(cur["log_beta_scales"], (M, 1))).double())
    return vo + torch.from_numpy(cur["trans"]).double()[:, None]


def weights_of(keypoints):
    weights, w_temp = mf.fit_weights()
    weights = np.array(weights, np.float64)
    if not keypoints:
        weights[0] = 0.0
    return weights, w_temp


def oracle(F, M, keypoints):
    """-> (terms (9,), gradients, silhouettes (M, S, S)) in float64, once per case"""
    key = ("oracle", F, M, keypoints)
    if key not in _CACHE:
        prob, cur, _ = problem(F, M)
        weights, w_temp = weights_of(keypoints)
        names = so.trainable_names(mf.FIT_STAGE)
        _, sums, grads = so.loss_and_grads(prob, {k: torch.from_numpy(v).double() for k, v in cur.items()}, weights, w_temp, names)
        om = patch_model(F)[1]
        with torch.no_grad():
            sil = so.soft_silhouette(posed(om, cur), om.faces, S).numpy()
        terms = np.array([sums.get(n, 0.0) for n in eng.LOSS_NAMES])
        _CACHE[key] = (terms, {k: g.numpy() for k, g in grads.items()}, sil)
    return _CACHE[key]


def hip(F, M, keypoints, reset=True):
    """-> (terms (9,), gradients, silhouettes) of one smalfit_fit_eval, as float32 arrays"""
    e = engine(F)
    _, cur, tg = problem(F, M)
    weights, w_temp = weights_of(keypoints)
    if reset:
        e.reset_raster_cache()
    d = {k: pc.dev(v) for k, v in cur.items()}
    sil = torch.full((M, S, S), -1.0, device="cuda")
    losses, grads = e.fit_eval(betas=d["betas"], log_beta_scales=d["log_beta_scales"], global_rotation=d["global_rotation"],
                               joint_rotations=d["joint_rotations"], trans=d["trans"], target_joints=pc.dev(tg["tj"]),
                               target_visibility=pc.dev(tg["vis"]), target_sil=pc.dev(tg["tsil"]), weights=weights, w_temp=w_temp,
                               window=WINDOW, want=so.trainable_names(mf.FIT_STAGE), sil_out=sil)
    assert e.status() == 0
    return losses.cpu().numpy(), {k: g.cpu().numpy() for k, g in grads.items()}, sil.cpu().numpy()


def same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in ((a[0], b[0]), (a[2], b[2]))) and all(np.array_equal(a[1][k], b[1][k]) for k in a[1])


def check_against_oracle(F, M, keypoints, capsys):
    terms, grads, sil = hip(F, M, keypoints)
    terms_o, grads_o, sil_o = oracle(F, M, keypoints)
    weights, _ = weights_of(keypoints)
    lines, bad = [], []

    def row(name, err, bound):
        lines.append("F=%-4d M=%d kp=%d  %-28s %.2e (<%.1e)" % (F, M, keypoints, name, err, bound))
        if not err < bound:
            bad.append(lines[-1])

    row("sil max-abs", float(np.abs(sil - sil_o).max()), SIL_TOL)
    # w_sil x the mean over a window's frames and pixels of |sil - target|: SIL_TOL at every pixel the scene reaches
    reach = (sil_o > 0.0).reshape(M, -1).sum(1)
    wsize = np.array([min(WINDOW, M - (n // WINDOW) * WINDOW) for n in range(M)])
    sil_bound = float(weights[1] * SIL_TOL * (reach / wsize).sum() / S ** 2)
    i_sil = eng.LOSS_NAMES.index("sil_reproj")
    assert terms_o[i_sil] > 10 * sil_bound
    for i, name in enumerate(eng.LOSS_NAMES):
        bound = sil_bound if i == i_sil else max(TERM_TOL * abs(terms_o[i]), sil_bound)
        row("term " + name, abs(float(terms[i]) - terms_o[i]), bound)
    for k in grads_o:
        g = grads[k].reshape(grads_o[k].shape)
        assert np.isfinite(g).all(), k
        row("d/d " + k, pc.rel(g, grads_o[k]), GRAD_TOL)
    if M > BEHIND:                                     # nothing of the two special frames is drawn
        assert sil_o[OFF_SCREEN].max() == 0.0 and sil_o[BEHIND].max() == 0.0
        assert sil[OFF_SCREEN].max() == 0.0 and sil[BEHIND].max() == 0.0
    assert sil_o.max() > 0.5                           # and something of the others is
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("M", FRAME_COUNTS)
@pytest.mark.parametrize("F", FACE_COUNTS)
def test_fit_eval_matches_oracle(F, M, capsys):
    """silhouette, the nine terms and every gradient of one evaluation, the joint riders behind the sweep blocks"""
    check_against_oracle(F, M, True, capsys)


@pytest.mark.parametrize("F", FACE_COUNTS)
def test_fit_eval_without_the_keypoint_term(F, capsys):
    check_against_oracle(F, 7, False, capsys)


@pytest.mark.parametrize("F", FACE_COUNTS)
def test_evaluations_repeat_bit_for_bit(F):
    """two consecutive evaluations, the second on the depth bounds the first left, and one after reset_raster_cache: the same bits"""
    first = hip(F, 9, True)
    second = hip(F, 9, True, reset=False)
    cold = hip(F, 9, True)
    assert same_bits(first, second)
    assert same_bits(second, cold)


@pytest.mark.parametrize("F", FACE_COUNTS)
def test_frames_of_the_padding_store_nothing(F):
    """An evaluation of 16 frames, then evaluations of 1, 7 and 9 frames, whose grids are padded to 8 and 16 frames, then the 16
    frames again: a padding workgroup that swept its frame's stale vertices would leave candidates in the per-pixel accumulators
    of a frame no later kernel of that call clears, and the second 16-frame evaluation would differ from the first."""
    full = hip(F, MAX_FRAMES, True)
    for M in FRAME_COUNTS:
        hip(F, M, True)
    again = hip(F, MAX_FRAMES, True)
    assert same_bits(full, again)
    # and each smaller evaluation is what a fresh engine computes (frames 0 .. M - 1 of nothing else)
    md, _ = patch_model(F)
    fresh = eng.Engine(eng.DeviceModel(md), MAX_FRAMES, S)
    fresh.set_pose_prior(*synthetic.synthetic_pose_prior())
    fresh.set_shape_prior(*synthetic.synthetic_shape_prior())
    used, _CACHE["engine", F] = _CACHE["engine", F], fresh
    try:
        clean = hip(F, 7, True)
    finally:
        _CACHE["engine", F] = used
    assert same_bits(hip(F, 7, True), clean)


@pytest.mark.parametrize("F", FACE_COUNTS)
def test_render_without_joint_riders(F, capsys):
    """smalfit_render_forward / smalfit_render_backward: the sweep launch without joint riders, 9 frames with the two special
    ones; silhouette and d/d verts against the oracle, and the list lengths against the box restatement of tests/raster_forms.py"""
    md, om = patch_model(F)
    e = engine(F)
    M = 9
    _, cur, _ = problem(F, M)
    verts = posed(om, cur).float().numpy()
    w = np.random.RandomState(F).randn(M, S, S).astype(np.float32)
    v64 = torch.from_numpy(verts).double().requires_grad_(True)
    sil_o = so.soft_silhouette(v64, om.faces, S)
    (sil_o * torch.from_numpy(w).double()).sum().backward()
    sil_o, dv_o = sil_o.detach().numpy(), v64.grad.numpy()
    vd = torch.from_numpy(verts).cuda().contiguous()
    e.reset_raster_cache()
    sil, _ = e.render_forward(vd)
    lengths = e.face_list_lengths(M).cpu().numpy()
    e.reset_raster_cache()
    dv = e.render_backward(vd, sil, torch.from_numpy(w).cuda())
    assert e.status() == 0
    sil, dv = sil.cpu().numpy(), dv.cpu().numpy()
    es, eg = float(np.abs(sil - sil_o).max()), pc.rel(dv, dv_o)
    with capsys.disabled():
        print("\nF=%-4d render: sil %.2e (<%.0e)  dverts %.2e (<%.0e)" % (F, es, SIL_TOL, eg, GRAD_TOL))
    assert es < SIL_TOL and eg < GRAD_TOL
    assert np.all(sil[sil_o == 0.0] == 0.0)
    assert not sil[OFF_SCREEN].any() and not sil[BEHIND].any() and not dv[OFF_SCREEN].any() and not dv[BEHIND].any()
    # a face without a pixel box hands the backward gather an empty list; the engine keeps faces in its own order
    order = mf.internal_face_order(md)
    faces = np.asarray(md.faces)[order]
    assert not lengths[OFF_SCREEN].any() and not lengths[BEHIND].any()
    checked = 0
    for n in range(M):
        if n in (OFF_SCREEN, BEHIND):
            continue
        boxes, margin = rf.face_boxes(verts[n].astype(np.float64), faces, S)
        clear = margin > 1.0 / 32                      # no box edge within the kernel's 1/64-pixel slack of a pixel-centre line
        empty = rf.box_pixels(boxes) == 0
        assert np.all(lengths[n][clear & empty] == 0), n
        P = rf.pairs(verts[n].astype(np.float64), faces, S)
        cnt, _ = rf.per_face(P, F)
        safe = np.ones(F, bool)
        unsafe = (P["edge_margin"] < rf.MARGIN_PX) | (P["blur_margin"] < rf.MARGIN_PX)
        safe[P["face"][unsafe]] = False
        sel = clear & ~empty & safe
        listed = sel & (lengths[n] < 254)
        assert np.array_equal(lengths[n][listed], cnt[listed]), n       # cold cache: every candidate of the box is listed
        checked += int(listed.sum())
    assert checked > 0
