"""Models unlike the stand-in: every variant is derived in memory from synthetic.synthetic_model(seed=0, shape_family_id=1)
as a model_io.SMALModelData and is a valid input of smalfit_model_create (parents[i] < i, face indices in range, V >= 3056).
tests/test_model_forms_cpu.py proves on the host which branch each variant reaches; tests/test_gpu_model_forms.py runs the
kernels on them against the float64 oracle.  Nothing here needs a GPU.

  trees      only `parents` changes: which of the two tree walks of pose_block / chain_bwd_kernel runs is decided by
             smalfit_plan.h: tree_levels (fast = at most kTreeMaxPass passes and kTreeMaxChildren children per non-root joint)
  valence    hub vertices with 9, 16, 17 and 40 incident corners (vertex_bwd_kernel holds kPre = 8 in registers and loops over
             the rest) and four vertices without any face
  weights8/9 1..8 / 1..9 skinning weights per vertex (the skin kernels hold 8 in registers and loop from the 9th), one
             joint without a vertex
  regressor  vertices in 0..12 rows of the joint regressor, one joint with an empty row; regressor_k1: at most one row each
  v*         other vertex counts: no padding lane (3328 = 13 x 256), the smallest model accepted (3056), a larger one (4100)
  nb*        other numbers of shape directions round the thresholds of chain_bwd_kernel (48 | 49: rest-joint table in LDS or
             not; 64 | 65: lanes of the reduction) and of the fitter (20 directions)
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from oracle import smal_oracle as so
from smalify_amd import synthetic
from tests import lbs_forms as lf

K_PRE = 8                  # kernels_lbs_backward.inc: vertex_bwd_kernel, constexpr int kPre = 8
SKIN_SLOTS = 8             # kernels_lbs_forward.inc: the skin kernels' register slots (min(m.Kw, 8))
JS_LDS_BETAS = 48          # kernels_lbs_backward.inc: js_lds = dbetaJ && m.NBall <= 48
MAX_MODEL_BETAS = 64       # smalfit_plan.h: kMaxModelBetas
FIT_BETAS = 20             # smalfit_plan.h: kFitBetas
MIN_VERTS = max(so.LANDMARKS) + 1

_CACHE = {}


def base():
    if "base" not in _CACHE:
        _CACHE["base"] = synthetic.synthetic_model(seed=0, shape_family_id=1)
    return _CACHE["base"]


def _replace(md, **changes):
    out = dataclasses.replace(md, **changes)
    V = out.v_template.shape[0]
    assert out.shapedirs.shape[1] == 3 * V and out.posedirs.shape == (306, 3 * V)
    assert out.J_regressor.shape == (V, 35) and out.weights.shape == (V, 35)
    assert out.faces.min() >= 0 and out.faces.max() < V and V >= MIN_VERTS
    p = np.asarray(out.parents)
    assert p[0] == -1 and all(0 <= p[i] < i for i in range(1, 35))
    return out


# ------------------------------------------------------------------------------------------------
# trees
# ------------------------------------------------------------------------------------------------
def _fast_limit(chain_len):
    """a chain over joints 1..chain_len, four joints under the root, then three more children for each of the chain's first
    joints until the 35 are used up: chain_len passes, four children per joint on the chain"""
    p = [-1, 0] + list(range(1, chain_len))
    p += [0] * 4
    k = 1
    while len(p) < 35:
        p += [k] * min(3, 35 - len(p))
        k += 1
    return p


def tree_parents(name):
    smal = [int(x) for x in base().parents]
    return {"smal": smal,
            "chain": [-1] + list(range(34)),
            "star": [-1] + [0] * 34,
            "five_children": [-1, 0, 1, 1, 1, 1, 1] + [i - 5 for i in range(7, 35)],
            "fast_limit": _fast_limit(16),
            "one_past": _fast_limit(17)}[name]


# name -> (fast, passes of the walk, levels)
TREES = {"smal": (True, 10, 11), "chain": (False, 34, 35), "star": (True, 7, 2), "five_children": (False, 8, 9),
         "fast_limit": (True, 16, 17), "one_past": (False, 17, 18)}
DEEP_TREES = ("chain", "fast_limit", "one_past")      # deeper than SMAL's: the float32 yardstick may take over the bar


# ------------------------------------------------------------------------------------------------
# meshes
# ------------------------------------------------------------------------------------------------
def corner_counts(faces, V):
    return np.bincount(np.asarray(faces).reshape(-1), minlength=V)


def _rings(faces, V):
    nbr = [set() for _ in range(V)]
    for a, b, c in np.asarray(faces):
        nbr[a].update((b, c)); nbr[b].update((a, c)); nbr[c].update((a, b))
    return nbr


HUB_LANDMARK, ISOLATED_LANDMARK = so.LANDMARKS[0], so.LANDMARKS[3]
# (vertex, incident corners).  Beside the landmark, the hubs are the vertices that the silhouette term of the fit case pulls
# hardest in every one of its frames (tests/test_model_forms_cpu.py: the regime proof needs them on the outline); their new faces
# reach HUB_RINGS rings out, so that they cover pixels
HUBS = ((HUB_LANDMARK, K_PRE + 1), (3646, K_PRE + 1), (2790, 16), (2884, 17), (3324, 40))
HUB_RINGS = 2


def valence_facts():
    """-> (hubs, isolated): the hub vertices and the four vertices without a face (vertex 0, the last vertex, one mid-mesh,
    one landmark)"""
    V = base().v_template.shape[0]
    return tuple(h for h, _ in HUBS), (0, V - 1, V // 2, ISOLATED_LANDMARK)


def valence_model(hub_list=HUBS, rings=HUB_RINGS):
    key = ("valence", hub_list, rings)
    if key in _CACHE:
        return _CACHE[key]
    md = base()
    V = md.v_template.shape[0]
    hubs, isolated = tuple(h for h, _ in hub_list), valence_facts()[1]
    faces = np.asarray(md.faces)
    faces = faces[~np.isin(faces, isolated).any(1)]
    nbr = _rings(faces, V)
    extra = []
    for h, want in hub_list:
        have = int(corner_counts(faces, V)[h])
        assert 0 < have <= K_PRE and not set(isolated) & nbr[h]
        inner, far = {h}, {h}
        for _ in range(rings):
            inner = set(far)
            far = far.union(*(nbr[u] for u in far))
        ring = sorted(far - inner - set(isolated) - set(hubs))
        assert len(ring) >= 6
        # (h, a, b) with a, b from the outermost ring, every pair used once: faces with the extent of `rings` rings
        pairs = [(ring[i], ring[(i + d) % len(ring)]) for d in range(1, len(ring) // 2) for i in range(len(ring))]
        assert len(set(map(frozenset, pairs))) == len(pairs) >= want - have
        extra += [(h, a, b) for a, b in pairs[:want - have]]
    faces = np.ascontiguousarray(np.concatenate([faces, np.asarray(extra, faces.dtype)], 0))
    _CACHE[key] = _replace(md, faces=faces)
    return _CACHE[key]


def internal_face_order(md):
    """smalfit_model_create's face order (Morton order of the template's face centroids on a 1024^3 grid, ties by face index),
    restated in float32: the order in which vertex_bwd_kernel meets a vertex's corners (tests/test_model_pack_cpu.py holds it to
    pack_smal_model's faces on every variant)"""
    vt = np.asarray(md.v_template, np.float32)
    f = np.asarray(md.faces)
    cen = ((vt[f[:, 0]] + vt[f[:, 1]]) + vt[f[:, 2]]) / np.float32(3.0)
    lo, hi = cen.min(0), cen.max(0)
    span = hi - lo
    q = np.minimum(np.float32(1023.0), (cen - lo) / np.where(span > 0, span, 1).astype(np.float32) * np.float32(1023.0)).astype(np.uint64)
    q[:, span <= 0] = 0
    code = np.zeros(len(f), np.uint64)
    for a in range(3):
        for bit in range(10):
            code |= ((q[:, a] >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit + a)
    return np.lexsort((np.arange(len(f)), code))


def truncated_faces(md, hubs, keep=K_PRE):
    """the face list with every hub's corners past the first `keep` (in the kernel's order) pointed at vertex V + k, k the
    hub's position in `hubs`: with detached duplicates of the hubs appended to the vertices, the silhouette's gradient as a
    gather that stops after `keep` corners would leave it"""
    V = md.v_template.shape[0]
    f = np.asarray(md.faces).astype(np.int64).copy()
    order = internal_face_order(md)
    for k, h in enumerate(hubs):
        seen = 0
        for fi in order:
            for c in range(3):
                if f[fi, c] == h:
                    seen += 1
                    if seen > keep:
                        f[fi, c] = V + k
    return f


class silhouette_truncated_at:
    """context: so.soft_silhouette renders `faces` over the vertices plus detached duplicates of `hubs` (truncated_faces)"""

    def __init__(self, hubs, faces):
        self.hubs, self.faces = list(hubs), torch.from_numpy(np.asarray(faces, np.int64))

    def __enter__(self):
        self.orig = so.soft_silhouette
        so.soft_silhouette = lambda verts, faces, *a, **k: self.orig(torch.cat([verts, verts[:, self.hubs].detach()], 1), self.faces, *a, **k)
        return self

    def __exit__(self, *exc):
        so.soft_silhouette = self.orig


# ------------------------------------------------------------------------------------------------
# sparsity
# ------------------------------------------------------------------------------------------------
EMPTY_JOINT = 12           # a leg's middle joint (it has a parent and a child): no skinned vertex / no regressor vertex


def _joint_d2(md):
    vt = np.asarray(md.v_template, np.float64)
    J = np.asarray(md.J_regressor, np.float64).T @ vt
    return ((vt[:, None] - J[None]) ** 2).sum(-1)


def weights_model(K):
    """vertex v has 1 + v % K skinning weights, on its nearest joints other than EMPTY_JOINT; rows sum to 1"""
    md = base()
    V = md.v_template.shape[0]
    d2 = _joint_d2(md)
    d2[:, EMPTY_JOINT] = np.inf
    near = np.argsort(d2, axis=1)
    w = np.zeros((V, 35))
    for v in range(V):
        j = near[v, :1 + v % K]
        w[v, j] = np.exp(-d2[v, j] / (2 * 0.05 ** 2)) + 1e-6
    w = (w / w.sum(1, keepdims=True)).astype(np.float32)
    return _replace(md, weights=np.ascontiguousarray(w))


REGRESSOR_ROWS = 12


def regressor_model(single=False):
    """EMPTY_JOINT's row of the regressor is empty.  single: every vertex keeps its largest entry only (Kj 1); else twelve
    vertices are put into 1 .. 12 rows (Kj 12) beside the stand-in's 0 .. 5.  Rows of the regressor (one per joint) sum to 1"""
    md = base()
    jr = np.asarray(md.J_regressor, np.float64).copy()          # (V, 35)
    jr[:, EMPTY_JOINT] = 0.0
    if single:
        top = jr.argmax(1)
        keep = np.zeros_like(jr)
        rows = np.arange(jr.shape[0])
        keep[rows, top] = jr[rows, top]
        jr = keep
    else:
        d2 = _joint_d2(md)
        d2[:, EMPTY_JOINT] = np.inf
        for k in range(1, REGRESSOR_ROWS + 1):
            v = 100 * k + 7
            jr[v] = 0.0
            jr[v, np.argsort(d2[v])[:k]] = 0.02
    s = jr.sum(0)
    jr = jr / np.where(s > 0, s, 1.0)
    return _replace(md, J_regressor=np.ascontiguousarray(jr.astype(np.float32)))


# ------------------------------------------------------------------------------------------------
# vertex counts
# ------------------------------------------------------------------------------------------------
def _take_verts(md, idx, faces):
    idx = np.asarray(idx)
    col = (3 * idx[:, None] + np.arange(3)[None]).reshape(-1)
    jr = np.asarray(md.J_regressor, np.float64)[idx]
    s = jr.sum(0)
    V = len(idx)
    inds = {k: np.asarray(getattr(md, k))[np.asarray(getattr(md, k)) < V] for k in ("left_inds", "right_inds", "center_inds")}
    return _replace(md, v_template=np.ascontiguousarray(md.v_template[idx]), shapedirs=np.ascontiguousarray(md.shapedirs[:, col]),
                    posedirs=np.ascontiguousarray(md.posedirs[:, col]), weights=np.ascontiguousarray(md.weights[idx]),
                    J_regressor=np.ascontiguousarray((jr / np.where(s > 0, s, 1.0)).astype(np.float32)),
                    faces=np.ascontiguousarray(faces.astype(md.faces.dtype)), **inds)


def verts_model(V):
    """V below the stand-in's 3889: its first V vertices, faces that touch a removed vertex dropped.  Above: a connected patch
    of the mesh appended as jittered copies with faces of their own"""
    md = base()
    V0 = md.v_template.shape[0]
    faces = np.asarray(md.faces)
    if V <= V0:
        return _take_verts(md, np.arange(V), faces[(faces < V).all(1)])
    nbr = _rings(faces, V0)
    patch, front = [2000], [2000]
    while len(patch) < V - V0:
        nxt = []
        for u in front:
            for w in sorted(nbr[u]):
                if w not in patch and len(patch) < V - V0:
                    patch.append(w); nxt.append(w)
        front = nxt
    remap = {u: V0 + k for k, u in enumerate(patch)}
    own = np.asarray([[remap[a], remap[b], remap[c]] for a, b, c in faces if a in remap and b in remap and c in remap])
    out = _take_verts(md, np.concatenate([np.arange(V0), np.asarray(patch)]), np.concatenate([faces, own], 0))
    vt = out.v_template.copy()
    vt[V0:] += (0.01 * np.random.RandomState(5).randn(V - V0, 3) + np.array([0.0, 0.0, 0.05])).astype(np.float32)
    return dataclasses.replace(out, v_template=np.ascontiguousarray(vt))


def skin_boundary(V):
    """(last frame count of the split form, first of the wide form) at this vertex count"""
    M = 5
    while lf.skin_form(M + 1, V) != "wide":
        M += 1
    return M, M + 1


def verts_frames(V):
    """one frame count per skinning form and the two on either side of the split | wide boundary, which moves with Vp.  (At
    V = 3056 the boundary lies at 80 | 81 frames: these two cases are the only ones past 65 frames)"""
    lo, hi = skin_boundary(V)
    return tuple(sorted({3, 17, lo, hi}))


# ------------------------------------------------------------------------------------------------
# shape directions
# ------------------------------------------------------------------------------------------------
def betas_model(NB):
    """the stand-in's 41 shape directions cut to NB rows, or extended with smooth random ones (quadratic fields of position, as
    the stand-in's are made)"""
    md = base()
    sd = np.asarray(md.shapedirs)
    if NB > sd.shape[0]:
        vt = np.asarray(md.v_template, np.float64)
        x, y, z = vt[:, 0], vt[:, 1], vt[:, 2]
        basis = np.stack([np.ones(len(vt)), x, y, z, x * x, y * y, z * z, x * y, x * z, y * z], 1)
        rs = np.random.RandomState(41)
        more = [((basis @ (rs.randn(10, 3) * np.array([0.3, 1, 1, 1, 2, 2, 2, 2, 2, 2])[:, None])) * (0.035 / (1.0 + 0.15 * b))).reshape(-1)
                for b in range(sd.shape[0], NB)]
        sd = np.concatenate([sd, np.asarray(more, np.float32)], 0)
    return _replace(md, shapedirs=np.ascontiguousarray(sd[:NB]))


# ------------------------------------------------------------------------------------------------
# the variants by name
# ------------------------------------------------------------------------------------------------
VERT_COUNTS = {"v3328": 3328, "v3056": 3056, "v4100": 4100}
BETA_COUNTS = {"nb12": 12, "nb20": 20, "nb48": 48, "nb49": 49, "nb64": 64, "nb65": 65}
SPARSITY = ("weights8", "weights9", "regressor", "regressor_k1")
ONE_PER_FORM = lf.ONE_PER_FORM


def variant(name):
    """-> SMALModelData"""
    if name in TREES:
        return _replace(base(), parents=np.asarray(tree_parents(name), np.int32))
    if name == "valence":
        return valence_model()
    if name in ("weights8", "weights9"):
        return weights_model(int(name[-1]))
    if name in ("regressor", "regressor_k1"):
        return regressor_model(single=name.endswith("k1"))
    if name in VERT_COUNTS:
        return verts_model(VERT_COUNTS[name])
    if name in BETA_COUNTS:
        return betas_model(BETA_COUNTS[name])
    raise KeyError(name)


def lbs_cases():
    """[(variant, M, nb)] of the LBS forward / backward comparison.  nb65 is absent: smalfit_model_create refuses the model"""
    out = [(t, M, 20) for t in TREES for M in ONE_PER_FORM]
    out += [(w, M, 20) for w in ("weights8", "weights9") for M in ONE_PER_FORM]      # the three skin kernels each have the loop
    out += [(r, M, 20) for r in ("regressor", "regressor_k1") for M in (3, 17)]
    out += [("valence", 3, 20)]
    out += [(v, M, 20) for v, V in VERT_COUNTS.items() for M in verts_frames(V)]
    out += [(b, M, NB) for b, NB in BETA_COUNTS.items() if NB <= MAX_MODEL_BETAS for M in (3, 17)]
    return out


FIT_VARIANTS = ("chain", "five_children", "star", "valence", "weights9", "v3328", "v4100", "nb20", "nb48", "nb49", "nb64")


def facts(md):
    """what the kernels specialise on"""
    V = md.v_template.shape[0]
    w, jr = np.asarray(md.weights) != 0, np.asarray(md.J_regressor) != 0
    cc = corner_counts(md.faces, V)
    return dict(V=V, Vp=lf.padded_verts(V), F=int(np.asarray(md.faces).shape[0]), NB=int(md.shapedirs.shape[0]),
                Kw=int(w.sum(1).max()), Kw_min=int(w.sum(1).min()), Kj=int(jr.sum(1).max()), Kj_min=int(jr.sum(1).min()),
                unskinned_joints=[int(j) for j in np.nonzero(w.sum(0) == 0)[0]],
                unregressed_joints=[int(j) for j in np.nonzero(jr.sum(0) == 0)[0]],
                valence_max=int(cc.max()), isolated=[int(v) for v in np.nonzero(cc == 0)[0]])


# ------------------------------------------------------------------------------------------------
# inputs and references of the LBS comparison
# ------------------------------------------------------------------------------------------------
def lbs_inputs(M, nb, V, seed=0):
    """tests/test_gpu_frame_counts.py: lbs_inputs (joint rotations of ~0.3 rad, limb scales of ~0.2) without the frame of zero
    rotations: every edge of the tree carries a rotation and a scale"""
    rs = np.random.RandomState(2000 + seed)
    return dict(beta=(0.5 * rs.randn(M, nb)).astype(np.float32), theta=(0.3 * rs.randn(M, 35, 3)).astype(np.float32),
                ls=(0.2 * rs.randn(M, 6)).astype(np.float32),
                wv=rs.randn(M, V, 3).astype(np.float32), wj=rs.randn(M, 41, 3).astype(np.float32))


def oracle_lbs(md, x, dtype=torch.float64):
    """values and gradients of so.smal_forward in `dtype`, as float64 arrays"""
    om = so.OracleModel(md, dtype)
    b = torch.from_numpy(x["beta"]).to(dtype).requires_grad_(True)
    t = torch.from_numpy(x["theta"]).to(dtype).requires_grad_(True)
    s = torch.from_numpy(x["ls"]).to(dtype).requires_grad_(True)
    vo, jo, Ro, vso = so.smal_forward(om, b, t, s)
    ((vo * torch.from_numpy(x["wv"]).to(dtype)).sum() + (jo * torch.from_numpy(x["wj"]).to(dtype)).sum()).backward()
    out = dict(verts=vo, joints=jo, Rs=Ro, vshaped=vso, dbeta=b.grad, dtheta=t.grad, dls=s.grad)
    return {k: v.detach().double().numpy() for k, v in out.items()}


# ------------------------------------------------------------------------------------------------
# the silhouette's adjoint per vertex, on `valence`
# ------------------------------------------------------------------------------------------------
RENDER_FRAMES, RENDER_SIZE = 2, 64
RENDER_TOL = 1e-2          # tests/test_gpu_parity.py::test_renderer: d/d verts of the silhouette, rel-L2


def render_case(md):
    """(verts (2,V,3) float32 in camera space, upstream gradient (2,64,64) float32): the model posed as
    tests/parity_cases.py: case_render poses the stand-in"""
    from tests import parity_cases as pc
    M = RENDER_FRAMES
    p = pc.random_pose(M, 11)
    theta = np.concatenate([p["global_rotation"][:, None], p["joint_rotations"]], 1)
    with torch.no_grad():
        vo, _, _, _ = so.smal_forward(so.OracleModel(md), torch.from_numpy(np.tile(p["betas"], (M, 1))).double(),
                                      torch.from_numpy(theta).double(), torch.from_numpy(np.tile(p["log_beta_scales"], (M, 1))).double())
    verts = (vo + torch.from_numpy(p["trans"]).double()[:, None]).float().numpy()
    return np.ascontiguousarray(verts), np.random.RandomState(12).randn(M, RENDER_SIZE, RENDER_SIZE).astype(np.float32)


def oracle_render_grad(md, verts, w, truncate_at=None):
    """d sum(sil * w) / d verts in float64; truncate_at: hubs whose corners past the K_PRE-th are cut off"""
    v = torch.from_numpy(verts).double().requires_grad_(True)
    if truncate_at is None:
        sil = so.soft_silhouette(v, torch.from_numpy(np.asarray(md.faces, np.int64)), RENDER_SIZE)
    else:
        ext = torch.cat([v, v[:, list(truncate_at)].detach()], 1)
        sil = so.soft_silhouette(ext, torch.from_numpy(truncated_faces(md, truncate_at)), RENDER_SIZE)
    (sil * torch.from_numpy(w).double()).sum().backward()
    return v.grad.numpy()


def row_errors(got, want):
    """per (frame, vertex): |got - want| / max(|want|, rms over all rows of |want|)"""
    g, w = np.asarray(got, np.float64), np.asarray(want, np.float64)
    n = np.linalg.norm(w, axis=-1)
    return np.linalg.norm(g - w, axis=-1) / np.maximum(n, np.sqrt((n ** 2).mean()))


# ------------------------------------------------------------------------------------------------
# the fused evaluation
# ------------------------------------------------------------------------------------------------
FIT_FRAMES, FIT_SIZE, FIT_WINDOW, FIT_STAGE = 3, 64, 2, 2
FIT_TOTAL_TOL, FIT_GRAD_TOL = 1e-4, 2e-3        # tests/test_gpu_frame_counts.py::test_fit_eval_matches_oracle_per_frame
PER_FRAME = ("global_rotation", "joint_rotations", "trans")


def fit_weights():
    from smalify_amd import config as cfg
    W = np.array(cfg.OPT_WEIGHTS).T
    weights, w_temp = W[FIT_STAGE][:6].copy(), float(W[FIT_STAGE][6])
    assert weights[1] > 0                       # the silhouette is on
    return weights, w_temp


def fit_problem(md):
    """(oracle problem, parameters, targets) of the fit case on this model: tests/parity_cases.py: make_problem_cpu"""
    from tests import parity_cases as pc
    return pc.make_problem_cpu(FIT_FRAMES, FIT_SIZE, FIT_WINDOW, model=(md, so.OracleModel(md)))


def oracle_fit(prob, cur):
    """-> (total, terms, gradients of stage 2) in float64"""
    weights, w_temp = fit_weights()
    total, sums, grads = so.loss_and_grads(prob, {k: torch.from_numpy(v).double() for k, v in cur.items()}, weights, w_temp,
                                           so.trainable_names(FIT_STAGE))
    return float(total), sums, {k: g.numpy() for k, g in grads.items()}
