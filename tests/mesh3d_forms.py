"""Which branches of the 3D mesh objective a case reaches -- a restatement of the launch geometry of
smalify_amd/csrc/kernels_mesh3d.inc and of the host's grids (smalfit_plan.h: mesh_grids), the cases of tests/test_gpu_mesh3d_forms.py, and a float64
numpy reference of the objective whose nearest-neighbour rule is explicit.  tests/test_mesh3d_forms_cpu.py checks that the
restatement still matches the source, that the cases reach every form and that the reference agrees with the oracle and
the host shim.  Nothing here asserts or needs a GPU.

  mesh3d_chamfer<ROLE>  one block per kChamQueries = 64 queries (ROLE 0: the S target points, ROLE 1: the V vertices);
                        the scanned set (ROLE 0: vertices, ROLE 1: points) is staged kChamChunk = 1024 at a time and each
                        of the 4 waves scans per = (cnt + 3) >> 2 of a chunk; nearest_merge combines the 4 waves
  grids                 bx = ceil(S / 64), by = ceil(V / 64), bv = ceil(V / 256), bp = ceil(P / 256)  (kMeshBlock = 256)
  tie rule              among equal squared distances the lowest index wins (strict '<' in nearest_scan over ascending
                        indices, lexicographic nearest_merge); torch's min, which the oracle uses, does not define one

Open question, not tested here: for an isolated vertex (empty ring) the kernel, the shim and the oracle all take the
Laplacian residual as 0.  PyTorch3D v0.2.5 is believed to put -1 on every diagonal entry of its uniform Laplacian, which
would give |v| instead; its source is not available to check, and SMAL meshes have no isolated vertex.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from oracle import mesh3d_oracle as mo

CHAM_QUERIES = 64          # kChamQueries
CHAM_CHUNK = 1024          # kChamChunk
MESH_BLOCK = 256           # kMeshBlock
WAVES = 4                  # waves of a 256-thread chamfer block
COS_EPS2 = 1e-16           # kCosEps2
MAX_MESHES = 5             # the objective capacity of the GPU cases (N = MAX_MESHES is one of the batch sizes)
DVERTS_TOL = 2e-4          # GPU bar on d/d verts (rel-L2 per mesh), the unit of the tie-discrimination check


def ceil_div(a, b):
    return (a + b - 1) // b


def grids(V, S, P):
    """launch grids of one evaluation (S = 1 stands for the chamfer-off call)"""
    return dict(bx=ceil_div(S, CHAM_QUERIES), by=ceil_div(V, CHAM_QUERIES), bv=ceil_div(V, MESH_BLOCK),
                bp=ceil_div(P, MESH_BLOCK))


def chunk_counts(no):
    """points of each staged chunk of a scanned set of `no` points"""
    return [min(CHAM_CHUNK, no - base) for base in range(0, no, CHAM_CHUNK)]


def wave_ranges(cnt):
    """[begin, end) of each wave's scan within a chunk of cnt points"""
    per = (cnt + 3) >> 2
    out = []
    for w in range(WAVES):
        b = min(w * per, cnt)
        out.append((b, min(b + per, cnt)))
    return out


def wave_of(index, no):
    """(chunk, wave) that scans point `index` of a scanned set of `no` points"""
    c = index // CHAM_CHUNK
    cnt = chunk_counts(no)[c]
    local = index - c * CHAM_CHUNK
    for w, (b, e) in enumerate(wave_ranges(cnt)):
        if b <= local < e:
            return c, w
    raise ValueError("index outside the scanned set")


def chamfer_form(role, nq, no):
    """role 0: nq = S queries scanning no = V vertices; role 1: nq = V, no = S
    -> (chunks, last-chunk count, waves with an empty range in the last chunk, 'partial' | 'full' last query block)"""
    counts = chunk_counts(no)
    empty = sum(1 for b, e in wave_ranges(counts[-1]) if b == e)
    return len(counts), counts[-1], empty, "full" if nq % CHAM_QUERIES == 0 else "partial"


# ---------------------------------------------------------------------------------------------------------------
# meshes
# ---------------------------------------------------------------------------------------------------------------
def ribbon(V, seed):
    """a triangle strip of V >= 3 vertices along a perturbed helix of radius 1 in z in [-1, 1] -> (verts float32, faces)"""
    assert V >= 3
    rs = np.random.RandomState(seed)
    k = np.arange(V) // 2
    n = max((V + 1) // 2, 1)
    turns = max(1.0, n / 64.0)
    t = 2.0 * np.pi * turns * k / n
    z = 2.0 * k / n - 1.0 + np.where(np.arange(V) % 2 == 0, -0.03, 0.03)
    v = np.stack([np.cos(t), np.sin(t), z], axis=1) + 0.01 * rs.randn(V, 3)
    f = [(i, i + 1, i + 2) if i % 2 == 0 else (i + 1, i, i + 2) for i in range(V - 2)]
    return v.astype(np.float32), np.asarray(f, np.int32)


def _d(rows):
    return np.asarray(rows, np.float32)           # every coordinate a multiple of 1/8: exact in float32


HAND_MESHES = {
    # one face: P = 0 (no face pairs, the normal term must be exactly 0)
    "triangle": (_d([[0, 0, 0], [1, 0, 0], [0, 1, 0.5]]), np.array([[0, 1, 2]], np.int32)),
    # closed: every edge has two faces
    "tetra": (_d([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.25, 0.25, 1]]),
              np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)),
    # test_mesh3d_cpu.py's strip of 4 triangles, a fin on edge (1,2) (3 faces: 3 pairs) and vertex 7 isolated
    "strip_fin": (_d([[0, 0, 0], [0.5, 0.25, 0], [0.25, 0.75, 0.125], [1, 0.75, 0], [0.75, 1.25, 0.25], [1.5, 1.25, 0],
                      [0.125, 0.5, 0.75], [2, -1, 1]]),
                  np.array([[0, 1, 2], [2, 1, 3], [2, 3, 4], [4, 3, 5], [1, 2, 6]], np.int32)),
    # 4 pages on the spine (0,1): 4 faces on one edge -> 6 pairs, every other edge a boundary
    "book": (_d([[0, 0, 0], [0, 0, 1], [1, 0, 0.5], [0, 1, 0.25], [-1, 0.125, 0.5], [0.25, -1, 0.75]]),
             np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4], [1, 0, 5]], np.int32)),
    # degree-4 fan whose centre equals its ring mean exactly: zero Laplacian residual at vertex 0
    "fan": (_d([[0, 0, 0], [0.5, 0, 0.25], [0, 0.5, -0.25], [-0.5, 0, 0.25], [0, -0.5, -0.25]]),
            np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1]], np.int32)),
    # a collinear face (0,1,2) next to the regular face (2,0,3): the pair on edge (0,2) falls under the cosine clamp
    "collinear": (_d([[0, 0, 0], [0.5, 0, 0], [1, 0, 0], [0.5, 0.75, 0.25]]), np.array([[0, 1, 2], [2, 0, 3]], np.int32)),
}


# ---------------------------------------------------------------------------------------------------------------
# float64 reference: explicit nearest neighbours, closed-form gradients
# ---------------------------------------------------------------------------------------------------------------
def sq_dists(q, o):
    """(len(q), len(o)) squared distances in float64, difference first (exact for dyadic inputs)"""
    q = np.asarray(q, np.float64)
    o = np.asarray(o, np.float64)
    out = np.empty((len(q), len(o)))
    for s in range(0, len(q), 256):
        d = q[s:s + 256, None, :] - o[None, :, :]
        out[s:s + 256] = (d * d).sum(-1)
    return out


def nearest(d2, rule="low"):
    """argmin along axis 1; among equal distances the lowest ('low') or the highest ('high') index"""
    if rule == "low":
        return d2.argmin(1)
    return d2.shape[1] - 1 - d2[:, ::-1].argmin(1)


def laplacian_residual(verts, faces):
    """(N,V,3) mean of the ring - v (0 for an empty ring), float64"""
    v = np.asarray(verts, np.float64)
    e = mo.unique_edges(faces)
    V = v.shape[1]
    deg = np.bincount(e.reshape(-1), minlength=V).astype(np.float64)
    acc = np.zeros_like(v)
    np.add.at(acc, (slice(None), e[:, 0]), v[:, e[:, 1]])
    np.add.at(acc, (slice(None), e[:, 1]), v[:, e[:, 0]])
    has = deg > 0
    return np.where(has[None, :, None], acc / np.maximum(deg, 1.0)[None, :, None] - v, 0.0), deg


def normal_pair_products(verts, pairs):
    """(w1 w2) of each face pair: the cosine clamp applies where it is <= 1e-16"""
    v = np.asarray(verts, np.float64)
    p = np.asarray(pairs, np.int64).reshape(-1, 4)
    v0, v1, a, b = (v[:, p[:, i]] for i in range(4))
    n0 = np.cross(v1 - v0, a - v0)
    n1 = np.cross(b - v0, v1 - v0)
    return (n0 * n0).sum(-1) * (n1 * n1).sum(-1)


def reference(verts, points, faces, weights, rule="low"):
    """objective and gradient of N meshes at `verts` (N,V,3) against `points` (N,S,3), weights clamped at 0 like the host
    -> dict(terms [chamfer, edge, normal, laplacian], total, dverts (N,V,3), dtrans (N,3), nn_points (N,S), nn_verts (N,V))"""
    v = np.asarray(verts, np.float64)
    N, V = v.shape[:2]
    wc, we, wn, wl = (max(float(w), 0.0) for w in weights)
    g = np.zeros_like(v)
    terms = np.zeros(4)
    nn_p = nn_v = None
    if wc > 0:
        p = np.asarray(points, np.float64)
        S = p.shape[1]
        nn_p = np.zeros((N, S), np.int64)
        nn_v = np.zeros((N, V), np.int64)
        for n in range(N):
            d2 = sq_dists(p[n], v[n])                                  # (S, V)
            ip = nearest(d2, rule)
            iv = nearest(d2.T, rule)
            nn_p[n], nn_v[n] = ip, iv
            terms[0] += (d2[np.arange(S), ip].mean() + d2[iv, np.arange(V)].mean()) / N
            g[n] += wc * 2.0 / (V * N) * (v[n] - p[n, iv])
            np.add.at(g[n], ip, wc * 2.0 / (S * N) * (v[n, ip] - p[n]))
    e = mo.unique_edges(faces)
    E = len(e)
    d = v[:, e[:, 0]] - v[:, e[:, 1]]
    terms[1] = (d * d).sum(-1).mean(1).sum() / N
    np.add.at(g, (slice(None), e[:, 0]), we * 2.0 / (E * N) * d)
    np.add.at(g, (slice(None), e[:, 1]), -we * 2.0 / (E * N) * d)
    pr = mo.face_pairs(faces)
    P = len(pr)
    if P:
        v0, v1, a, b = (v[:, pr[:, i]] for i in range(4))
        ed, ea, eb = v1 - v0, a - v0, b - v0
        n0, n1 = np.cross(ed, ea), np.cross(eb, ed)
        w12, w1, w2 = (n0 * n1).sum(-1), (n0 * n0).sum(-1), (n1 * n1).sum(-1)
        prod = w1 * w2
        live = prod > COS_EPS2
        r = 1.0 / np.sqrt(np.where(live, prod, COS_EPS2))
        terms[2] = (1.0 - w12 * r).mean(1).sum() / N
        r3 = np.where(live, r ** 3 * w12, 0.0)
        G0 = -(r[..., None] * n1 - (r3 * w2)[..., None] * n0)
        G1 = -(r[..., None] * n0 - (r3 * w1)[..., None] * n1)
        dE = np.cross(ea, G0) + np.cross(G1, eb)
        dA, dB = np.cross(G0, ed), np.cross(ed, G1)
        c = wn / (P * N)
        for col, gg in ((1, dE), (2, dA), (3, dB), (0, -(dE + dA + dB))):
            np.add.at(g, (slice(None), pr[:, col]), c * gg)
    lv, deg = laplacian_residual(v, faces)
    nrm = np.sqrt((lv * lv).sum(-1))
    terms[3] = nrm.mean(1).sum() / N
    unit = np.where(nrm[..., None] > 0, lv / np.where(nrm > 0, nrm, 1.0)[..., None], 0.0)
    gl = -unit * (deg > 0)[None, :, None]
    inv = np.where(deg > 0, 1.0 / np.maximum(deg, 1.0), 0.0)
    np.add.at(gl, (slice(None), e[:, 0]), unit[:, e[:, 1]] * inv[e[:, 1]][None, :, None])
    np.add.at(gl, (slice(None), e[:, 1]), unit[:, e[:, 0]] * inv[e[:, 0]][None, :, None])
    g += wl / (V * N) * gl
    total = wc * terms[0] + we * terms[1] + wn * terms[2] + wl * terms[3]
    return dict(terms=terms, total=total, dverts=g, dtrans=g.sum(1), nn_points=nn_p, nn_verts=nn_v)


# ---------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------
GENERAL_WEIGHTS = (1.0, 0.7, 0.3, 0.2)
TIE_WEIGHTS = (1.0, 0.0, 0.0, 0.0)


@dataclass
class Tie:
    """a designed tie in mesh `mesh`: role 0 -> target point `query` is equidistant from vertices a < b; role 1 ->
    vertex `query` is equidistant from target points a < b"""
    role: int
    mesh: int
    query: int
    a: int
    b: int
    placement: str

    def rows(self):
        """rows of d/d verts whose value depends on which candidate wins"""
        return [self.a, self.b] if self.role == 0 else [self.query]


@dataclass
class Case:
    name: str
    faces: np.ndarray
    lbs: np.ndarray                  # (N,V,3) float32
    trans: np.ndarray                # (N,3) float32
    deform: np.ndarray | None        # (N,V,3) float32 or None
    points: np.ndarray               # (N,S,3) float32
    weights: tuple = GENERAL_WEIGHTS
    ties: list = field(default_factory=list)
    topology: tuple = ()             # topology branches the mesh was built for

    @property
    def N(self):
        return self.lbs.shape[0]

    @property
    def V(self):
        return self.lbs.shape[1]

    @property
    def S(self):
        return self.points.shape[1]

    @property
    def P(self):
        return len(mo.face_pairs(self.faces))

    @property
    def verts(self):
        """the composed vertices exactly as mesh3d_compose_kernel forms them in float32"""
        v = self.lbs + self.trans[:, None, :]
        return v + self.deform if self.deform is not None else v


def _margin_violations(q, o, skip=()):
    """queries (not in skip) whose runner-up is not at least 1e-5 (1 + |q|^2) beyond the nearest -> (query, best, second)"""
    d2 = sq_dists(q, o)
    bad = []
    if d2.shape[1] < 2:
        return bad
    part = np.argpartition(d2, 1, axis=1)[:, :2]
    for i in range(len(q)):
        if i in skip:
            continue
        a, b = part[i]
        if d2[i, a] > d2[i, b]:
            a, b = b, a
        if d2[i, b] - d2[i, a] < 1e-5 * (1.0 + float(np.dot(q[i], q[i]))):
            bad.append((i, a, b))
    return bad


def nn_margin(case):
    """violations of the margin rule in every mesh of the case, both directions: every query that is not a designed tie
    has its runner-up at least 1e-5 (1 + |q|^2) beyond its nearest; a designed tie has its two candidates at exactly the
    same distance, below every other candidate by that margin -> list of (mesh, role, query) that break it"""
    out = []
    verts = case.verts.astype(np.float64)
    pts = case.points.astype(np.float64)
    for n in range(case.N):
        ties = [t for t in case.ties if t.mesh == n]
        for role, q, o in ((0, pts[n], verts[n]), (1, verts[n], pts[n])):
            mine = {t.query: t for t in ties if t.role == role}
            out += [(n, role, i) for i, _, _ in _margin_violations(q, o, skip=mine)]
            for i, t in mine.items():
                d2 = sq_dists(q[i:i + 1], o)[0]
                rest = np.delete(d2, [t.a, t.b])
                if d2[t.a] != d2[t.b] or d2[t.a] != d2.min() or \
                        (len(rest) and rest.min() - d2[t.a] < 1e-5 * (1.0 + float(q[i] @ q[i]))):
                    out.append((n, role, i))
    return out


def _fix_points(case, rs, sample):
    """redraw target points until the case meets nn_margin (designed tie points stay)"""
    fixed = {(t.mesh, x) for t in case.ties if t.role == 1 for x in (t.a, t.b)}
    fixed |= {(t.mesh, t.query) for t in case.ties if t.role == 0}
    verts = case.verts.astype(np.float64)
    for _ in range(200):
        redraw = set()
        for n in range(case.N):
            pts = case.points[n].astype(np.float64)
            for i, _, _ in _margin_violations(pts, verts[n]):
                redraw.add((n, i))
            for _, a, b in _margin_violations(verts[n], pts):
                redraw.update({(n, int(a)), (n, int(b))})
        redraw -= fixed
        if not redraw:
            break
        for n, i in sorted(redraw):
            case.points[n, i] = sample(rs, n)
    assert not nn_margin(case), case.name
    return case


def _surface_sampler(verts, scale=0.05):
    def sample(rs, n):
        return (verts[n, rs.randint(verts.shape[1])] + scale * rs.randn(3)).astype(np.float32)
    return sample


def ribbon_case(V, S, N, seed, weights=GENERAL_WEIGHTS):
    rs = np.random.RandomState(seed)
    base, faces = ribbon(V, seed)
    lbs = (base[None] + 0.004 * rs.randn(N, V, 3)).astype(np.float32)
    trans = (0.02 * rs.randn(N, 3)).astype(np.float32)
    dfm = (0.002 * rs.randn(N, V, 3)).astype(np.float32)
    c = Case("ribbon_V%d_S%d_N%d" % (V, S, N), faces, lbs, trans, dfm, np.zeros((N, S, 3), np.float32), weights)
    sample = _surface_sampler(c.verts)
    for n in range(N):
        for i in range(S):
            c.points[n, i] = sample(rs, n)
    return _fix_points(c, rs, sample)


# the clamped pair's gradient is ~1e8 |n1| |e| per vertex (torch's cosine_similarity clamp) and cancels over the four
# vertices: a weight of 1e-8 keeps it of the order of the other terms, so that d/d trans, the sum over all vertices in
# float32, is not swamped by the rounding of those large cancelling rows
HAND_WEIGHTS = {"collinear": (1.0, 0.7, 1e-8, 0.2)}


def hand_case(name, S, N, seed):
    rs = np.random.RandomState(seed)
    v, faces = HAND_MESHES[name]
    lbs = np.repeat(v[None], N, 0)
    trans = (np.round(rs.uniform(-2, 2, size=(N, 3)) * 8) / 8).astype(np.float32)     # dyadic: composition stays exact
    c = Case("hand_%s_S%d_N%d" % (name, S, N), faces, lbs, trans, None, np.zeros((N, S, 3), np.float32),
             HAND_WEIGHTS.get(name, GENERAL_WEIGHTS))
    sample = _surface_sampler(c.verts, 0.3)
    for n in range(N):
        for i in range(S):
            c.points[n, i] = sample(rs, n)
    return _fix_points(c, rs, sample)


# far corners for the designed ties: dyadic, away from the ribbon (radius ~1, |z| <= 1) and from each other
_FAR = _d([[3, 3, 3], [3, -3, -3], [-3, 3, -3], [-3, -3, 3]])
_STEP = _d([[0.25, 0, 0], [0, 0.25, 0]])   # the two tied candidates sit at distinct positions at squared distance 1/16


def points_tie_case(seed=41):
    """role 1 ties: vertices 97..99 of a 100-vertex ribbon each equidistant from two of 2048 target points, the pair
    placed in one wave, across waves and across chunks (the lower index first, scanned first)"""
    V, S = 100, 2048
    pairs = (("one wave", 10, 20), ("across waves", 30, 700), ("across chunks", 40, 1024 + 40))
    rs = np.random.RandomState(seed)
    base, faces = ribbon(V, seed)
    lbs = base[None].copy()
    c = Case("ties_points", faces, lbs, np.zeros((1, 3), np.float32), None, np.zeros((1, S, 3), np.float32), TIE_WEIGHTS)
    for k, (where, a, b) in enumerate(pairs):
        vq = V - 3 + k
        c.lbs[0, vq] = _FAR[k]
        c.points[0, a] = _FAR[k] + _STEP[0]
        c.points[0, b] = _FAR[k] + _STEP[1]
        c.ties.append(Tie(1, 0, vq, a, b, where))
    tied = {x for t in c.ties for x in (t.a, t.b)}
    near = _surface_sampler(c.lbs[:, :V - 3])
    for i in range(S):
        if i not in tied:
            c.points[0, i] = near(rs, 0)
    return _fix_points(c, rs, near)


def verts_tie_case(seed=43):
    """role 0 ties: target points 0..2 each equidistant from two vertices of a 2049-vertex ribbon, the pair in one wave,
    across waves and across chunks"""
    V, S = 2049, 300
    pairs = (("one wave", 9, 20), ("across waves", 5, 600), ("across chunks", 7, 1024 + 76))
    rs = np.random.RandomState(seed)
    base, faces = ribbon(V, seed)
    c = Case("ties_verts", faces, base[None].copy(), np.zeros((1, 3), np.float32), None, np.zeros((1, S, 3), np.float32),
             TIE_WEIGHTS)
    for k, (where, a, b) in enumerate(pairs):
        c.points[0, k] = _FAR[k]
        c.lbs[0, a] = _FAR[k] + _STEP[0]
        c.lbs[0, b] = _FAR[k] + _STEP[1]
        c.ties.append(Tie(0, 0, k, a, b, where))
    moved = {x for t in c.ties for x in (t.a, t.b)}
    keep = np.array([i for i in range(V) if i not in moved])
    near = _surface_sampler(c.lbs[:, keep])
    for i in range(len(pairs), S):
        c.points[0, i] = near(rs, 0)
    return _fix_points(c, rs, near)


# (mesh, S, N) of the objective cases: chosen so that both chamfer roles reach every form (tests/test_mesh3d_forms_cpu.py)
HAND_CASES = (("triangle", 5, 1), ("tetra", 4, 3), ("strip_fin", 63, MAX_MESHES), ("book", 64, 1), ("fan", 65, 3),
              ("collinear", 2, 1))
RIBBON_CASES = ((3, 1, 1), (4, 2, 3), (6, 3, 1), (63, 64, MAX_MESHES), (64, 65, 1), (65, 1024, 3), (255, 1025, 1),
                (256, 1027, 3), (257, 2048, 1), (1024, 2053, 1), (1025, 3000, 1), (1026, 63, 3), (1029, 5, MAX_MESHES),
                (2049, 4, 1))
TIE_CASES = ("ties_points", "ties_verts")

_CACHE = {}


def case_names():
    return (["hand_%s_S%d_N%d" % h for h in HAND_CASES] + ["ribbon_V%d_S%d_N%d" % r for r in RIBBON_CASES]
            + list(TIE_CASES))


def case(name):
    if name not in _CACHE:
        if name == "ties_points":
            c = points_tie_case()
        elif name == "ties_verts":
            c = verts_tie_case()
        elif name.startswith("hand_"):
            h = next(h for h in HAND_CASES if "hand_%s_S%d_N%d" % h == name)
            c = hand_case(*h, seed=len(name) + h[1])
            c.topology = topology_branches(c)
        else:
            r = next(r for r in RIBBON_CASES if "ribbon_V%d_S%d_N%d" % r == name)
            c = ribbon_case(*r, seed=r[0] + 7 * r[1])
        _CACHE[name] = c
    return _CACHE[name]


def topology_branches(c):
    """the topology branches a case's mesh reaches"""
    out = set()
    faces = np.asarray(c.faces)
    e = mo.unique_edges(faces)
    f = np.sort(faces, axis=1)
    he = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [0, 2]]])
    _, per_edge = np.unique(he, axis=0, return_counts=True)
    if c.P == 0:
        out.add("no face pairs")
    if (per_edge == 1).any():
        out.add("boundary edge")
    if (per_edge == 3).any():
        out.add("edge of 3 faces")
    if (per_edge == 4).any():
        out.add("edge of 4 faces")
    if len(np.unique(e)) < c.V:
        out.add("isolated vertex")
    lv, deg = laplacian_residual(c.verts, faces)
    if ((np.abs(lv).max(-1) == 0) & (deg > 0)[None]).any():
        out.add("zero Laplacian residual")
    if c.P and (normal_pair_products(c.verts, mo.face_pairs(faces)) <= COS_EPS2).any():
        out.add("clamped normal pair")
    return tuple(sorted(out))


TOPOLOGY_BRANCHES = ("no face pairs", "boundary edge", "edge of 3 faces", "edge of 4 faces", "isolated vertex",
                     "zero Laplacian residual", "clamped normal pair")


def coverage_table(names=None):
    """one row per case: grids, both chamfer forms, topology branches"""
    rows = []
    for name in names or case_names():
        c = case(name)
        rows.append(dict(name=name, N=c.N, V=c.V, S=c.S, P=c.P, **grids(c.V, c.S, c.P),
                         role0=chamfer_form(0, c.S, c.V), role1=chamfer_form(1, c.V, c.S),
                         topology=topology_branches(c)))
    return rows
