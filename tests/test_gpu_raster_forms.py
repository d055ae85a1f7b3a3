"""The HIP rasteriser against the float64 oracle (oracle/smal_oracle.soft_silhouette, autograd for d/d verts) at every
capacity branch and depth-cache transition, on the crafted scenes of tests/raster_forms.py (tests/test_raster_forms_cpu.py
proves which branch each reaches), at the image sizes the engine accepts, and bit-exact frame independence."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import raster_anchors as ra  # noqa: E402
from tests import raster_forms as rf    # noqa: E402

V_PAD = 8192          # the largest scene (6510 vertices) plus the 64 vertices the frame's reference depth is taken from
PAD_Z = 2.0           # z_view of the unused vertices: the reference depth, constant whatever the scene does
SIL_TOL = 2e-4        # float32 squared distances over sigma = 1e-4; no ties, no pixel centre near an edge or the blur radius
GRAD_TOL = 1e-3       # rel-L2 of d/d verts: float32 sums of up to 1025 terms per pixel, no K-cut ambiguity
_ENGINES = {}


def _slots():
    """vertex slots of a scene: every index except the 64 face_bbox_kernel averages into the reference depth"""
    sampled = {(t * V_PAD) >> 6 for t in range(64)}
    return np.array([i for i in range(V_PAD) if i not in sampled])


SLOTS = _slots()


def _model_data(faces, template=None, shapedir=None):
    """arbitrary topology over V_PAD vertices, rigid skinning on the root joint, no pose blend shapes; template (V_PAD, 3)
    and shapedir (3 V_PAD,), the first shape direction, default to zero (the renderer entry points take any vertices)"""
    from smalify_amd import model_io, synthetic
    base = synthetic.synthetic_model(seed=0, shape_family_id=1)
    w = np.zeros((V_PAD, 35), np.float32)
    w[:, 0] = 1.0
    jr = np.zeros((V_PAD, 35), np.float32)
    jr[np.arange(35), np.arange(35)] = 1.0
    sd = np.zeros((41, 3 * V_PAD), np.float32)
    if shapedir is not None:
        sd[0] = shapedir
    return model_io.SMALModelData(
        v_template=np.zeros((V_PAD, 3), np.float32) if template is None else template, shapedirs=sd,
        posedirs=np.zeros((306, 3 * V_PAD), np.float32), J_regressor=jr, weights=w, parents=base.parents,
        faces=np.ascontiguousarray(SLOTS[faces], np.int32), left_inds=np.zeros(0, np.int64),
        right_inds=np.zeros(0, np.int64), center_inds=np.zeros(0, np.int64))


def _engine(faces, M=1, tag=0, S=rf.S0):
    from smalify_amd import engine as eng
    key = (faces.tobytes(), M, tag, S)
    if key not in _ENGINES:
        _ENGINES[key] = eng.Engine(eng.DeviceModel(_model_data(faces)), M, S)
    return _ENGINES[key]


def _pad_np(v):
    """(V, 3) scene vertices -> (V_PAD, 3) float32; unused vertices off-screen at z_view = PAD_Z"""
    out = np.tile(ra.world_from_ndc(5.0, 5.0, PAD_Z).astype(np.float32), (V_PAD, 1))
    out[SLOTS[:len(v)]] = v
    return out


def _pad(frames):
    return torch.from_numpy(np.stack([_pad_np(v) for v in frames])).cuda()


def _oracle(verts, faces, w, K=rf.K, S=rf.S0):
    from oracle import smal_oracle as so
    v = torch.from_numpy(rf.to_f32(verts))[None].requires_grad_(True)
    sil = so.soft_silhouette(v, faces, S, faces_per_pixel=K)
    (sil * torch.from_numpy(w).double()).sum().backward()
    return sil[0].detach().numpy(), v.grad[0].numpy()


def _hip(e, verts, w, reset=True, fwd_first=None):
    """(sil, d/d scene verts) of one frame; fwd_first: vertices of an earlier call on the same cache (no reset between)"""
    if reset:
        e.reset_raster_cache()
    if fwd_first is not None:
        e.render_forward(_pad([fwd_first]))
    v = _pad([verts])
    sil, _ = e.render_forward(v)
    if fwd_first is not None:                     # the backward's own forward must see the same cache state as `sil`
        e.reset_raster_cache()
        e.render_forward(_pad([fwd_first]))
    dv = e.render_backward(v, sil, torch.from_numpy(w[None]).cuda())
    assert e.status() == 0
    return sil[0].double().cpu().numpy(), dv[0].double().cpu().numpy()[SLOTS[:len(verts)]]


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _never_near(verts, faces, K=rf.K):
    """vertex ids used only by faces that are among no pixel's K nearest (their gradient is exactly zero)"""
    _, ff, _ = rf.per_pixel(rf.pairs(rf.to_f32(verts), faces))
    near = set()
    for f in ff.values():
        near.update(int(x) for x in f[:K])
    used = {int(v) for i, fc in enumerate(faces) if i in near for v in fc}
    return np.array(sorted({int(v) for fc in faces for v in fc} - used), np.int64)


def _compare(name, sil, dv, sil_o, dv_o, sil_tol=SIL_TOL, grad_tol=GRAD_TOL, report=None, never=None):
    es, eg = float(np.abs(sil - sil_o).max()), _rel(dv, dv_o)
    if report is not None:
        report.append("%-28s sil %.2e (<%.0e)  dverts %.2e (<%.0e)" % (name, es, sil_tol, eg, grad_tol))
    assert es < sil_tol, (name, es)
    assert np.all(sil[sil_o == 0.0] == 0.0), name                 # pixels no face reaches: exactly 0
    assert eg < grad_tol, (name, eg)
    if never is not None and len(never):                            # faces among no pixel's K nearest: exactly 0
        assert np.all(dv[never] == 0.0) and np.all(dv_o[never] == 0.0), (name, int(np.sum(dv[never] != 0.0)))


def _dsil(seed):
    return np.random.RandomState(seed).randn(rf.S0, rf.S0).astype(np.float32)


@pytest.fixture(scope="module")
def report():
    lines = []
    yield lines
    print("\n" + "\n".join(lines))


@pytest.mark.parametrize("n", rf.STACK_COUNTS)
def test_candidate_counts(n, report):
    verts, faces = rf.count_stack(n)
    v = rf.to_f32(verts)
    w = _dsil(n)
    sil, dv = _hip(_engine(faces), v, w)
    sil_o, dv_o = _oracle(v, faces, w)
    never = _never_near(v, faces)
    assert (len(never) > 0) == (n >= rf.K + 32)                                    # far layers out of every pixel's cut
    _compare("stack N=%d" % n, sil, dv, sil_o, dv_o, report=report, never=never)


def test_cover_cap(report):
    verts, faces = rf.cover_stack()
    v = rf.to_f32(verts)
    w = _dsil(5)
    sil, dv = _hip(_engine(faces), v, w)
    sil_o, dv_o = _oracle(v, faces, w)
    _compare("cover > 1024", sil, dv, sil_o, dv_o, report=report, never=_never_near(v, faces))


def test_union_box_cap(report):
    verts, faces = rf.hit_stack()
    v = rf.to_f32(verts)
    w = _dsil(9)
    sil, dv = _hip(_engine(faces), v, w)
    sil_o, dv_o = _oracle(v, faces, w)
    _compare("union boxes > 1024", sil, dv, sil_o, dv_o, report=report, never=_never_near(v, faces))


def test_face_formats(report):
    verts, faces, names = rf.format_faces()
    v = rf.to_f32(verts)
    w = _dsil(3)
    e = _engine(faces)
    sil, dv = _hip(e, v, w)
    sil_o, dv_o = _oracle(v, faces, w)
    _compare("face formats (cold)", sil, dv, sil_o, dv_o, report=report)
    # per named face: its own vertices' gradient (each face has three vertices of its own)
    for name in set(names):
        idx = np.concatenate([np.arange(3 * i, 3 * i + 3) for i, nm in enumerate(names) if nm == name])
        assert _rel(dv[idx], dv_o[idx]) < GRAD_TOL, name
    # the same scene once more on the warm cache (render_backward re-runs the forward on the bounds render_forward left)
    sil2, dv2 = _hip(e, v, w, reset=False)
    _compare("face formats (warm)", sil2, dv2, sil_o, dv_o, report=report)


def test_list_capacity(report):
    """a list filled to its last entry, and one candidate more (masks): every candidate of the two faces carries gradient"""
    verts, faces, names = rf.list_edge_faces()
    v = rf.to_f32(verts)
    w = _dsil(4)
    sil, dv = _hip(_engine(faces), v, w)
    sil_o, dv_o = _oracle(v, faces, w)
    _compare("list capacity", sil, dv, sil_o, dv_o, report=report)
    for f in (3, 7):
        assert _rel(dv[3 * f:3 * f + 3], dv_o[3 * f:3 * f + 3]) < GRAD_TOL, names[f]


@pytest.mark.parametrize("name", sorted(rf.cache_sequences()))
def test_cache_transitions(name, report):
    z1, on1, z2, on2, sh = rf.cache_sequences()[name]
    v1, faces = rf.stack(z1, sh, on1)
    v2, _ = rf.stack(z2, sh, on2)
    v1, v2 = rf.to_f32(v1), rf.to_f32(v2)
    w = _dsil(sum(map(ord, name)))
    e = _engine(faces)
    # a tie at the cut: both tied layers are kept (the selection's rule; pytorch3d's pick among equals is unspecified) --
    # the layers' footprints are identical, so this is the oracle with one more face per pixel wherever the tie is at the cut
    K = rf.K + 1 if name == "band_tie" else rf.K
    sil1, dv1 = _hip(e, v1, w)
    sil1_o, dv1_o = _oracle(v1, faces, w)
    _compare(name + " call 1", sil1, dv1, sil1_o, dv1_o, report=report)
    warm, dvw = _hip(e, v2, w, reset=True, fwd_first=v1)
    cold, dvc = _hip(e, v2, w, reset=True)
    sil2_o, dv2_o = _oracle(v2, faces, w, K=K)
    _compare(name + " call 2", warm, dvw, sil2_o, dv2_o, report=report, never=_never_near(v2, faces, K))
    _compare(name + " call 2 (reset)", cold, dvc, sil2_o, dv2_o)
    # the cache changes the path, so the summation order, never the result beyond float32 noise
    assert np.abs(warm - cold).max() < 1e-5 and _rel(dvw, dvc) < 1e-4


@pytest.mark.parametrize("S", rf.SIZES)
def test_image_sizes_with_the_stand_in(S, report):
    from tests import parity_cases as pc
    from oracle import smal_oracle as so
    from smalify_amd import engine as eng
    md, om, dm = pc.get_model()
    p = pc.random_pose(1, 11, z=1.45)
    theta = np.concatenate([p["global_rotation"][:, None], p["joint_rotations"]], 1)
    with torch.no_grad():
        vo, _, _, _ = so.smal_forward(om, torch.from_numpy(np.tile(p["betas"], (1, 1))).double(), torch.from_numpy(theta).double(),
                                      torch.from_numpy(np.tile(p["log_beta_scales"], (1, 1))).double())
    verts = (vo + torch.from_numpy(p["trans"]).double()[:, None]).float()
    e = eng.Engine(dm, 1, S)
    sil, _ = e.render_forward(verts.cuda().contiguous())
    w = np.random.RandomState(S).randn(1, S, S).astype(np.float32)
    grad = S <= 64                                  # the float64 autograd of a megapixel image is left to the crafted case
    v64 = verts.double().requires_grad_(grad)
    sil_o = so.soft_silhouette(v64, om.faces, S)
    if grad:
        (sil_o * torch.from_numpy(w).double()).sum().backward()
        dv = e.render_backward(verts.cuda().contiguous(), sil, pc.dev(w)).double().cpu().numpy()
    assert e.status() == 0
    err = float(np.abs(sil.double().cpu().numpy() - sil_o.detach().numpy()).max())
    line = "S=%-5d sil %.2e (<2e-3)" % (S, err)
    assert err < 2e-3, (S, err)                     # SMAL poses: test_gpu_parity.test_renderer's bound
    if grad:
        g = _rel(dv, v64.grad.numpy())
        line += "  dverts %.2e (<1e-2)" % g
        assert g < 1e-2, (S, g)
    report.append(line)


def test_full_image_triangle_at_1024(report):
    from smalify_amd import engine as eng
    verts, faces, S, checks = rf.big_triangle_1024()
    v = rf.to_f32(verts)
    e = _engine(faces, S=S)
    vp = _pad([v])
    sil, _ = e.render_forward(vp)
    w = np.random.RandomState(1024).randn(S, S).astype(np.float32)
    dv = e.render_backward(vp, sil, torch.from_numpy(w[None]).cuda())[0].double().cpu().numpy()[SLOTS[:len(v)]]
    assert e.status() == 0
    s = sil[0].double().cpu().numpy()
    err = max(abs(s[r, c] - exp) for r, c, exp in checks)
    for r, c, exp in checks:
        assert abs(s[r, c] - exp) < SIL_TOL, (r, c, s[r, c], exp)
        if exp == 0.0:
            assert s[r, c] == 0.0
    # the backward's pixel walk at the largest size: ~10^6 (face, pixel) pairs, rows up to 1023
    sil_o, dv_o = _oracle(v, faces, w, S=S)
    es, eg = float(np.abs(s - sil_o).max()), _rel(dv, dv_o)
    report.append("S=1024 triangle: closed form %.2e, oracle sil %.2e (<2e-4), dverts %.2e (<1e-3)" % (err, es, eg))
    assert es < SIL_TOL and eg < GRAD_TOL, (es, eg)
    with pytest.raises(eng.SmalfitError):
        eng.Engine(e.model, 1, rf.MAX_S + 1)


# ---- (c) the same branches with a target: fit_eval, silhouette term only ------------------------------------------------------
W_SIL = 100.0
FIT_SCENES = ("stack_99", "stack_165", "band_narrow", "band_wide", "band_overflow", "need_eq_0", "short_miss", "all_band",
              "need_lt_0")


def _fit_scene(name):
    """(v1, v2, faces): call 1 renders v1, call 2 v2; the stacks are one cold call (v1 = v2)"""
    if name.startswith("stack_"):
        verts, faces = rf.count_stack(int(name[6:]))
        return verts, verts, faces
    z1, on1, z2, on2, sh = rf.cache_sequences()[name]
    v1, faces = rf.stack(z1, sh, on1)
    return v1, rf.stack(z2, sh, on2)[0], faces


def _target(sil):
    """1 where the oracle's silhouette is above 1/2, except every third diagonal (0: saturated pixels that still owe a loss)"""
    r, c = np.mgrid[0:rf.S0, 0:rf.S0]
    return ((sil > 0.5) & ((r + c) % 3 != 0)).astype(np.float32)


@pytest.mark.parametrize("name", FIT_SCENES)
def test_fit_eval_silhouette_term(name, report):
    """the crafted vertices go in as the template, v2 - v1 as the first shape direction (betas[0] = 0 renders v1, 1 renders
    v2), rigid skinning, zero pose: the resolve, band and select kernels' loss and adjoint-seed arithmetic with a target,
    against the oracle's window_loss on the same model"""
    from oracle import smal_oracle as so
    from smalify_amd import engine as eng, synthetic
    v1, v2, faces = _fit_scene(name)
    t1, t2 = _pad_np(rf.to_f32(v1)), _pad_np(rf.to_f32(v2))
    md = _model_data(faces, t1, (t2.astype(np.float64) - t1).reshape(-1))
    e = eng.Engine(eng.DeviceModel(md), 1, rf.S0)
    pp, sp = synthetic.synthetic_pose_prior(), synthetic.synthetic_shape_prior()
    e.set_pose_prior(*pp)
    e.set_shape_prior(*sp)
    om = so.OracleModel(md)
    weights = [0.0, W_SIL, 0.0, 0.0, 0.0, 0.0]
    zero = dict(log_beta_scales=np.zeros(6, np.float32), global_rotation=np.zeros((1, 3), np.float32),
                joint_rotations=np.zeros((1, 34, 3), np.float32), trans=np.zeros((1, 3), np.float32))
    tj, vis = np.zeros((1, 25, 2), np.float32), np.zeros((1, 25), np.float32)

    def params(b0):
        b = np.zeros(20, np.float32)
        b[0] = b0
        return dict(zero, betas=b)

    def oracle(b0, vv):
        sil = so.soft_silhouette(torch.from_numpy(rf.to_f32(vv))[None], faces, rf.S0)[0].numpy()
        tsil = _target(sil)
        prob = so.FitProblem(om, rf.S0, tj, vis, tsil[None], pp[0], pp[1], pp[2], sp[0], sp[1], 1, use_unity_prior=True)
        _, sums, g = so.loss_and_grads(prob, {k: torch.from_numpy(x).double() for k, x in params(b0).items()}, weights, 0.0,
                                       ("trans",))
        return tsil, sums["sil_reproj"], g["trans"].numpy(), int(np.sum(sil > 0.0))

    def hip(b0, tsil):
        d = {k: torch.from_numpy(x).cuda() for k, x in params(b0).items()}
        losses, grads = e.fit_eval(**d, target_joints=torch.from_numpy(tj).cuda(), target_visibility=torch.from_numpy(vis).cuda(),
                                   target_sil=torch.from_numpy(tsil[None]).cuda(), weights=weights, w_temp=0.0, window=1,
                                   want=("trans",))
        assert e.status() == 0
        return float(losses[4]), grads["trans"].double().cpu().numpy()

    tsil1, l1o, g1o, n1 = oracle(0.0, v1)
    tsil2, l2o, g2o, n2 = oracle(1.0, v2)
    e.reset_raster_cache()
    l1, g1 = hip(0.0, tsil1)
    l2, g2 = hip(1.0, tsil2)                        # on the bounds call 1 left
    e.reset_raster_cache()
    l2c, g2c = hip(1.0, tsil2)
    # loss: W_SIL times the mean of |sil - target| over the image, so SIL_TOL at every pixel the scene reaches bounds it
    bound = W_SIL * SIL_TOL * max(n1, n2) / rf.S0 ** 2
    report.append("fit %-17s sil loss %.2e / %.2e (<%.0e abs)  d/d trans %.2e / %.2e (<1e-3)"
                  % (name, abs(l1 - l1o), abs(l2 - l2o), bound, _rel(g1, g1o), _rel(g2, g2o)))
    assert l2o > 10 * bound
    for l, lo, g, go in ((l1, l1o, g1, g1o), (l2, l2o, g2, g2o), (l2c, l2o, g2c, g2o)):
        assert abs(l - lo) < bound, (name, l, lo)
        assert _rel(g, go) < GRAD_TOL, (name, g, go)


def _frame_scenes(M):
    """M different scenes of one topology (165 layers): lateral offsets, depth orders, layers switched off, one frame
    off-screen and one behind the camera"""
    n = rf.K + 65
    frames = []
    for i in range(M):
        rs = np.random.RandomState(i)
        depths = rf.Z0 + rf.GAP * rs.permutation(n).astype(np.float64)
        on = rs.rand(n) < (1.0 if i % 3 else 0.7)
        v, _ = rf.stack(depths, rf.mixed_shifts(n, i), on, u0=20.5 + 2 * (i % 9), v0=20.3 + 1.5 * (i % 7))
        if i == 5:
            v, _ = rf.stack(depths, None, None, u0=-3.0 * rf.S0)                 # off-screen
        if i == 6:
            v = v.copy(); v[:, 2] = ra.CAM_DIST + 1.0                              # behind the camera: every face culled
        frames.append(rf.to_f32(v).astype(np.float32))
    return frames, np.arange(3 * n).reshape(n, 3)


def test_frames_are_independent_bit_for_bit():
    frames, faces = _frame_scenes(17)
    dsil = torch.from_numpy(np.stack([_dsil(100 + i) for i in range(17)])).cuda()
    e = _engine(faces, M=17)

    def run(eng_, idx):
        eng_.reset_raster_cache()
        v = _pad([frames[i] for i in idx])
        sil, _ = eng_.render_forward(v)
        eng_.reset_raster_cache()
        dv = eng_.render_backward(v, sil, dsil[idx].contiguous())
        assert eng_.status() == 0
        return sil.cpu().numpy(), dv.cpu().numpy()

    singles = [run(e, [i]) for i in range(17)]
    for M in (1, 8, 9, 17):
        sil, dv = run(e, list(range(M)))
        for i in range(M):
            assert np.array_equal(sil[i], singles[i][0][0]), (M, i)
            assert np.array_equal(dv[i], singles[i][1][0]), (M, i)
    assert singles[6][0].max() == 0.0 and singles[5][0].max() == 0.0
    # after the larger call and a reset, a call has the bits of a fresh engine
    fresh = _engine(faces, M=17, tag=1)
    for i in (0, 3):
        a, b = run(e, [i]), run(fresh, [i])
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), i
