"""GPU tests of the LBS, fit and fit3d paths at every frame-count and shape-parameter-count branch of the host code.

The host picks the skinning kernel and the pose-blend adjoint's frame chunks from the frame count M (tests/lbs_forms.py
restates the rules; tests/test_lbs_forms_cpu.py checks that the lists below reach every form), and the gradient assembly
sums d/d betas for any number of shape parameters up to the model's 41.  Here each of those branches runs against the
float64 oracle (oracle/smal_oracle.py, oracle/mesh3d_oracle.py), frame by frame: an error confined to a few frames of a
tile or a chunk would vanish in a relative norm over the whole tensor.  A frame's error is taken relative to its own norm,
or to the median frame norm where that is larger.  Tolerances are those of tests/test_gpu_parity.py: LBS values 2e-5, LBS
gradients 5e-4, fitter total 1e-4 and gradients 2e-3, fit3d d/d verts 2e-4.

Matrix-core tile rows are independent and per-frame betas add nothing across frames, so some results must hold bit for
bit: a prefix of a call equals the shorter call where both run the same kernel forms, an engine's capacity changes no
bit, and frames a longer earlier call left in the engine's padded tiles never leak into a later, shorter one."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import smal_oracle as so  # noqa: E402
from smalify_amd import config as cfg  # noqa: E402
from smalify_amd import engine as eng  # noqa: E402
from tests import lbs_forms as lf  # noqa: E402
from tests import mesh3d_cases as mc  # noqa: E402
from tests import parity_cases as pc  # noqa: E402

S_IMG = 64
MAX_M = max(lf.LBS_FRAMES)
VALUES = ("verts", "joints", "Rs", "vshaped")
GRADS = ("dbeta", "dtheta", "dls")


def frame_errors(got, want):
    """per-frame |got - want| / max(|want_n|, median_n |want_n|) over the leading (frame) axis"""
    w = np.asarray(want, np.float64)
    g = np.asarray(got, np.float64).reshape(w.shape).reshape(w.shape[0], -1)
    w = w.reshape(w.shape[0], -1)
    den = np.linalg.norm(w, axis=1)
    return np.linalg.norm(g - w, axis=1) / np.maximum(den, max(float(np.median(den)), 1e-30))


def assert_per_frame(got, want, tol, what):
    err = frame_errors(got, want)
    assert np.isfinite(np.asarray(got, np.float64)).all(), what
    n = int(np.argmax(err))
    assert err[n] < tol, (what, "frame", n, float(err[n]), "of", len(err))


def lbs_inputs(M, nb=20, seed=0, V=lf.NUM_VERTS):
    rs = np.random.RandomState(1000 + seed)
    theta = (0.3 * rs.randn(M, 35, 3)).astype(np.float32)
    theta[0, 3:] = 0.0                                  # a frame with exactly-zero joint rotations
    return dict(beta=(0.5 * rs.randn(M, nb)).astype(np.float32), theta=theta,
                ls=(0.2 * rs.randn(M, 6)).astype(np.float32),
                wv=rs.randn(M, V, 3).astype(np.float32), wj=rs.randn(M, 41, 3).astype(np.float32))


def hip_lbs(e, x):
    d = {k: pc.dev(v) for k, v in x.items()}
    v, j, Rs, vs = e.lbs_forward(d["beta"], d["theta"], d["ls"])
    db, dt, dl = e.lbs_backward(d["beta"], d["theta"], d["ls"], d["wv"], d["wj"])
    out = dict(verts=v, joints=j, Rs=Rs, vshaped=vs, dbeta=db, dtheta=dt, dls=dl)
    return {k: t.cpu().numpy() for k, t in out.items()}


def oracle_lbs(om, x):
    b64 = torch.from_numpy(x["beta"]).double().requires_grad_(True)
    t64 = torch.from_numpy(x["theta"]).double().requires_grad_(True)
    l64 = torch.from_numpy(x["ls"]).double().requires_grad_(True)
    vo, jo, Ro, vso = so.smal_forward(om, b64, t64, l64)
    ((vo * torch.from_numpy(x["wv"]).double()).sum() + (jo * torch.from_numpy(x["wj"]).double()).sum()).backward()
    return dict(verts=vo.detach().numpy(), joints=jo.detach().numpy(), Rs=Ro.detach().numpy(), vshaped=vso.detach().numpy(),
                dbeta=b64.grad.numpy(), dtheta=t64.grad.numpy(), dls=l64.grad.numpy())


def check_lbs(M, nb=20, dense=False, seed=0):
    _, om, _ = pc.get_model(dense)
    e = pc.get_engine(MAX_M, S_IMG, dense)[0]
    x = lbs_inputs(M, nb, seed)
    got, want = hip_lbs(e, x), oracle_lbs(om, x)
    assert e.status() == 0
    for k in VALUES:
        assert_per_frame(got[k], want[k], 2e-5, (M, nb, dense, k))
    for k in GRADS:
        assert_per_frame(got[k], want[k], 5e-4, (M, nb, dense, k))


# ---- LBS component against the oracle ----------------------------------------------------------------------------
@pytest.mark.parametrize("M", lf.LBS_FRAMES)
def test_lbs_matches_oracle_per_frame(M):
    check_lbs(M)


@pytest.mark.parametrize("M", lf.ONE_PER_FORM)
def test_lbs_dense_weights_per_frame(M):
    """the reference's dense (V,35) weight matrices: 35 skinning weights per vertex, past the 8 of the fast loop"""
    check_lbs(M, dense=True, seed=1)


@pytest.fixture(scope="module")
def smal_module():
    from smalify_amd.smal_model.smal_torch import SMAL
    md, om = pc.get_oracle_model()
    return SMAL("cuda", shape_family_id=1, model_data=md), om


@pytest.mark.parametrize("M", lf.ONE_PER_FORM)
@pytest.mark.parametrize("tag", ["delv", "vtmpl", "rs"])
def test_smal_call_options_per_frame(smal_module, M, tag):
    """SMAL.__call__ with a per-frame del_v, a per-call v_template, or rotation matrices for theta: values and autograd
    against the oracle, frame by frame, once in each skinning form"""
    smal, om = smal_module
    x = lbs_inputs(M, seed=2)
    rs = np.random.RandomState(77 + M)
    V = om.V
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device="cuda", requires_grad=True)  # noqa: E731
    o = lambda a: torch.from_numpy(np.asarray(a, np.float32)).double().requires_grad_(True)  # noqa: E731
    theta_in = so.rodrigues(torch.from_numpy(x["theta"]).double().reshape(-1, 3)).reshape(M, 35, 3, 3).numpy() \
        if tag == "rs" else x["theta"]
    extra = {"delv": (0.01 * rs.randn(M, V, 3)),
             "vtmpl": (om.v_template.numpy() + 0.01 * rs.randn(V, 3))}.get(tag)
    beta, theta, ls = t(x["beta"]), t(theta_in), t(x["ls"])
    b64, th64, l64 = o(x["beta"]), o(theta_in), o(x["ls"])
    kw, kw64 = {}, {}
    if tag == "delv":
        kw["del_v"], kw64["del_v"] = t(extra), o(extra)
    if tag == "vtmpl":
        kw["v_template"], kw64["v_template"] = t(extra), o(extra)
    verts, joints, Rs, vs = smal(beta, theta, betas_logscale=ls, **kw)
    vo, jo, Ro, vso = so.smal_forward(om, b64, th64, l64, **kw64)
    for k, a, b in (("verts", verts, vo), ("joints", joints, jo), ("Rs", Rs, Ro), ("vshaped", vs, vso)):
        assert_per_frame(a.detach().cpu().numpy(), b.detach().numpy(), 2e-5, (M, tag, k))
    wv, wj = torch.from_numpy(x["wv"]), torch.from_numpy(x["wj"])
    ((verts * wv.cuda()).sum() + (joints * wj.cuda()).sum()).backward()
    ((vo * wv.double()).sum() + (jo * wj.double()).sum()).backward()
    for k, a, b in (("dbeta", beta, b64), ("dtheta", theta, th64), ("dls", ls, l64)):
        assert_per_frame(a.grad.cpu().numpy(), b.grad.numpy(), 5e-4, (M, tag, k))
    if tag == "delv":
        assert_per_frame(kw["del_v"].grad.cpu().numpy(), kw64["del_v"].grad.numpy(), 5e-4, (M, tag, "ddel_v"))
    if tag == "vtmpl":
        assert pc.rel(kw["v_template"].grad.cpu().numpy(), kw64["v_template"].grad.numpy()) < 5e-4


# ---- shape-parameter counts --------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", lf.BETA_COUNTS)
def test_lbs_beta_counts(nb):
    """smalfit_lbs_*_ex with nb of the model's 41 shape directions (oracle: shapedirs[:nb])"""
    check_lbs(9, nb=nb, seed=3)


@pytest.mark.parametrize("nb", lf.BETA_COUNTS)
def test_smal_autograd_beta_counts(smal_module, nb):
    """the drop-in SMAL with beta.shape[1] = nb (the reference accepts up to 41), in the wide skinning form"""
    smal, om = smal_module
    M = 50
    x = lbs_inputs(M, nb, seed=4)
    beta = torch.tensor(x["beta"], device="cuda", requires_grad=True)
    theta = torch.tensor(x["theta"], device="cuda", requires_grad=True)
    verts, joints, _, _ = smal(beta, theta)
    ((verts * pc.dev(x["wv"])).sum() + (joints * pc.dev(x["wj"])).sum()).backward()
    b64 = torch.from_numpy(x["beta"]).double().requires_grad_(True)
    t64 = torch.from_numpy(x["theta"]).double().requires_grad_(True)
    vo, jo, _, _ = so.smal_forward(om, b64, t64)
    ((vo * torch.from_numpy(x["wv"]).double()).sum() + (jo * torch.from_numpy(x["wj"]).double()).sum()).backward()
    assert_per_frame(verts.detach().cpu().numpy(), vo.detach().numpy(), 2e-5, (nb, "verts"))
    assert_per_frame(beta.grad.cpu().numpy(), b64.grad.numpy(), 5e-4, (nb, "dbeta"))
    assert_per_frame(theta.grad.cpu().numpy(), t64.grad.numpy(), 5e-4, (nb, "dtheta"))


# ---- bit-exact invariants ----------------------------------------------------------------------------------------
def assert_same_bits(a, b, what, n=None):
    for k in VALUES + GRADS:
        x = a[k] if n is None else a[k][:n]
        assert np.array_equal(x, b[k]), (what, k)


@pytest.mark.parametrize("M1,M2", lf.PREFIX_PAIRS)
def test_prefix_of_a_longer_call_has_the_same_bits(M1, M2):
    e = pc.get_engine(MAX_M, S_IMG)[0]
    x = lbs_inputs(M2, seed=5)
    long_call = hip_lbs(e, x)
    short_call = hip_lbs(e, {k: v[:M1] for k, v in x.items()})
    assert_same_bits(long_call, short_call, (M1, M2), n=M1)


@pytest.mark.parametrize("M", (17, 65))
def test_engine_capacity_changes_no_bit(M):
    dm = pc.get_model()[2]
    x = lbs_inputs(M, seed=6)
    tight = hip_lbs(eng.Engine(dm, M, S_IMG), x)
    roomy = hip_lbs(eng.Engine(dm, 2 * M + 3, S_IMG), x)
    assert_same_bits(tight, roomy, M)


@pytest.mark.parametrize("M_before,M", ((64, 49), (130, 65)))
def test_frames_of_an_earlier_longer_call_do_not_leak(M_before, M):
    """frames [M, M_before) of the earlier call stay in the engine's buffers, inside the later call's last 16-frame tile
    or pose-blend chunk"""
    dm = pc.get_model()[2]
    used = eng.Engine(dm, M_before, S_IMG)
    hip_lbs(used, lbs_inputs(M_before, seed=7))
    x = lbs_inputs(M, seed=8)
    assert_same_bits(hip_lbs(used, x), hip_lbs(eng.Engine(dm, M_before, S_IMG), x), (M_before, M))


# ---- fused fitter evaluation --------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", lf.FIT_FRAMES)
def test_fit_eval_matches_oracle_per_frame(M):
    """smalfit_fit_eval with shared betas, the silhouette on and a ragged last window, at frame counts of the split and
    the wide skinning kernel and of one to three pose-blend chunks"""
    window, stage = 4, 2
    assert M % window != 0
    W = np.array(cfg.OPT_WEIGHTS).T
    weights, w_temp = W[stage][:6].copy(), float(W[stage][6])
    assert weights[1] > 0
    e, prob, cur, tg = pc.make_problem(M, S_IMG, window)
    names = so.trainable_names(stage)
    total, _, grads_o = so.loss_and_grads(prob, {k: torch.from_numpy(v).double() for k, v in cur.items()}, weights,
                                          w_temp, names)
    d = {k: pc.dev(v) for k, v in cur.items()}
    losses, grads = e.fit_eval(betas=d["betas"], log_beta_scales=d["log_beta_scales"],
                               global_rotation=d["global_rotation"], joint_rotations=d["joint_rotations"],
                               trans=d["trans"], target_joints=pc.dev(tg["tj"]), target_visibility=pc.dev(tg["vis"]),
                               target_sil=pc.dev(tg["tsil"]), weights=weights, w_temp=w_temp, window=window, want=names)
    assert e.status() == 0
    l = losses.cpu().numpy().astype(np.float64)
    assert abs(l.sum() - float(total)) / abs(float(total)) < 1e-4
    for k in names:
        g, go = grads[k].cpu().numpy(), grads_o[k].numpy()
        assert pc.rel(g.reshape(go.shape), go) < 2e-3, k
        if k in ("global_rotation", "joint_rotations", "trans"):
            assert_per_frame(g, go, 2e-3, (M, k))


# ---- fit3d at batch sizes past the small end ---------------------------------------------------------------------
def test_fit3d_objective_and_gradient_at_32_meshes():
    """as test_gpu_fit3d.py::test_objective_and_gradient_match_oracle, at N = 32 (400 target points: the oracle's (S, V)
    chamfer temporaries stay within host memory)"""
    N, S, weights = 32, 400, (1.0, 1.0, 0.01, 0.1)
    md, lbs, trans, dfm, pts = mc.objective_problem(N, S, seed=32)
    obj = eng.MeshObjective(md.num_verts, md.faces, N, S)
    o = obj.eval(pc.dev(lbs), pc.dev(trans), pc.dev(dfm), pc.dev(pts), weights)
    torch.cuda.synchronize()
    verts = o["verts"].cpu().numpy()
    assert np.abs(verts - (lbs.astype(np.float64) + trans[:, None, :] + dfm)).max() < 1e-6
    total, terms, g = mc.oracle_objective(verts, pts, md.faces, weights)
    losses = o["losses"].cpu().numpy()
    for i, k in enumerate(("chamfer", "edge", "normal", "laplacian")):
        if k in terms:
            assert abs(losses[i] - terms[k]) <= 2e-5 * abs(terms[k]), (k, losses[i], terms[k])
    assert abs(losses[4] - total) <= 2e-5 * abs(total)
    assert mc.rel(o["dverts"].cpu().numpy(), g) < 2e-4
    assert_per_frame(o["dverts"].cpu().numpy(), g, 2e-4, "dverts")
    gt = g.sum(1)
    assert np.abs(o["dtrans"].cpu().numpy() - gt).max() <= 2e-4 * np.abs(gt).max() + 1e-7


@pytest.mark.parametrize("N,iters", ((32, 6), (57, 3)))
def test_fit3d_fused_step_equals_the_component_calls(N, iters):
    """as test_gpu_fit3d.py::test_fused_step_equals_the_component_calls, with the split (N = 32) and the wide (N = 57, a
    ragged tile) skinning kernel in the fused step.  The two paths round a few gradient elements differently in the last
    bit, and Adam turns such a difference at a near-zero gradient into a step of ~lr: with 48 meshes or more (split
    kernel at 48 as much as wide at 49 and beyond) six steps part the parameters by ~1e-5 rel-L2, three do not"""
    assert lf.skin_form(N) == ("split" if N < 49 else "wide")
    (la, pa, xa), (lb, pb, xb) = mc.fused_and_component_runs(N, iters=iters)
    assert np.array_equal(xa, xb)
    assert np.abs(la - lb).max() <= 1e-6 * np.abs(lb).max()
    for k in pa:
        assert mc.rel(pa[k], pb[k]) < 1e-6 or np.array_equal(pa[k], pb[k]), k
