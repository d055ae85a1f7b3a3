"""Which branch of the soft-silhouette rasteriser a crafted scene reaches -- a restatement of the capacities and decisions of
smalify_amd/csrc/kernels_raster.inc, float64 counting of box pixels and candidates the way the kernels count them, and the
scene builders of tests/test_gpu_raster_forms.py.  tests/test_raster_forms_cpu.py checks that the restated constants still
match the source and that every scene lands in the class it is named for.  Nothing here needs a GPU.

  face formats (raster_sweep_kernel, hand-off to raster_bwd_kernel), per wave of four consecutive faces:
      LIST   every face of the wave: box <= LIST_BOX pixels and <= LIST_LDS candidates
      MASKS  otherwise, when the face's box holds <= 16 MASK_ROUNDS pixels
      NOLIST otherwise (the whole box is walked); also set by the selection for a short miss
  resolve decisions (raster_resolve_kernel), c = #{z <= lo}, b = #{lo < z <= hi}, need = K - c:
      saturated | no bounds (c <= K: done, c > K: select) | need < 0 or b > BAND_CAP: select | need == 0: done |
      need > b: select with finite hi, band (b > 0) or done (b == 0) with hi = inf | band, wide when b > BAND_WIDE
  selection (raster_select_kernel): new bounds lo < z_K <= hi from half-widths delta0 / 2^i, delta0 = BAND_HALF (z_K - z_min) / K,
      the first whose band (z_K - delta, z_K + delta] holds <= fill candidates; hi = inf when no candidate lies beyond it.

Scenes are built in pixel units (u = column, v = row; the centre of pixel (r, c) is (u, v) = (c, r)), mapped to NDC and then
to world coordinates with raster_anchors.world_from_ndc.  Every layer of a stack is flat in depth (one z_view per face), so
depths are exact and the K cut is a pure rank: layers are separated by GAP, far beyond float32 resolution.
"""
from __future__ import annotations

import math

import numpy as np

from tests import raster_anchors as ra

# ---- restated constants (checked against the source by tests/test_raster_forms_cpu.py)
K = 100                     # smalfit_math.h kFacesPerPixel
LIST_CAP = 128              # kListCap: bytes per face
LIST_LDS = 128              # kListLds: list entries staged per face
LIST_BOX = 256              # `listed = npx <= 256`: box-relative indices are bytes
MASK_ROUNDS = 64            # kMaskRounds: a mask covers 16 * 64 = 1024 box pixels
ACC_WIN = 36                # kAccWin: the sweep's LDS window edge
SWEEP_FACES = 32            # kSweepFaces
RECT_FACES = 8              # kRectFaces: faces per union box
BAND_CAP = 64               # kBandCap
BAND_WIDE = 32              # bqueue bit 31: more than 32 band entries
BAND_FILL_WIDE, BAND_FILL, BAND_FILL_NARROW = 40, 24, 12
BAND_HALF = 4.0             # kBandHalf
BAND_TRIES = 6              # kBandTries
CAND_CAP = 1024             # kCandCap
HIT_CAP = 1024              # kHitCap
COVER_CAP = 1024            # kCoverCap
BOX_SLACK = 1.0 / 64.0      # kBoxSlack (pixels)
MAX_S = 1024                # smalfit_engine_create

R_BLUR = math.sqrt(ra.BLUR)  # NDC
S0 = 64                     # image size of the crafted scenes
GAP = 1e-3                  # depth step between stack layers (z_view units; float32 resolves ~2e-7 here)
Z0 = 2.0                    # z_view of the nearest layer
JITTER = 0.1069             # depth jitter of the cache stacks (fraction of GAP): no depth within 5 % of the narrowest half-width of a bound
MARGIN_PX = 0.001           # (float32 places a centre to ~2e-6 px) no pixel centre within this many pixels of an edge, the blur cutoff or a box edge

NUDGE = (0.104, 0.233, 0.132, 0.154, 0.308, 0.303, 0.212)   # fractions of a pixel that keep the format faces' margins

NOLIST, MASKS, LIST = "nolist", "masks", "list"


# ---- geometry --------------------------------------------------------------------------------------------------------------
def ndc_of_px(u, v, S=S0):
    return 1.0 - (2.0 * u + 1.0) / S, 1.0 - (2.0 * v + 1.0) / S


def world_face(uv, z_view, S=S0):
    """(3, 2) pixel-unit corners at one depth -> (3, 3) world"""
    return np.stack([ra.world_from_ndc(*ndc_of_px(u, v, S), z_view) for u, v in uv])


def to_f32(verts):
    """the scene as both sides see it: world coordinates rounded to float32"""
    return np.asarray(verts, np.float32).astype(np.float64)


def project(verts):
    """(V, 3) world -> (x_ndc, y_ndc, z_view) float64, as oracle/smal_oracle.world_to_ndc"""
    zv = ra.CAM_DIST - verts[:, 2]
    return ra.S_CAM * -verts[:, 0] / zv, ra.S_CAM * verts[:, 1] / zv, zv


def face_boxes(verts, faces, S=S0):
    """per face (c0, c1, r0, r1) of pixel centres within the sqrt(blur)-expanded bounding box, clamped to the image
    (empty: c0 > c1), and the smallest distance in pixels of any pixel-centre line to a box edge (face_bbox_kernel)"""
    x, y, _ = project(verts)
    fx, fy = x[faces], y[faces]
    xlo, xhi = fx.min(1) - R_BLUR, fx.max(1) + R_BLUR
    ylo, yhi = fy.min(1) - R_BLUR, fy.max(1) + R_BLUR
    u_lo, u_hi = (1.0 - xhi) * S / 2.0 - 0.5, (1.0 - xlo) * S / 2.0 - 0.5
    v_lo, v_hi = (1.0 - yhi) * S / 2.0 - 0.5, (1.0 - ylo) * S / 2.0 - 0.5
    c0, c1 = np.maximum(np.ceil(u_lo), 0), np.minimum(np.floor(u_hi), S - 1)
    r0, r1 = np.maximum(np.ceil(v_lo), 0), np.minimum(np.floor(v_hi), S - 1)
    area = (fx[:, 2] - fx[:, 0]) * (fy[:, 1] - fy[:, 0]) - (fy[:, 2] - fy[:, 0]) * (fx[:, 1] - fx[:, 0])
    c0 = np.where(np.abs(area) > 1e-8, c0, 1)                          # culled faces get no box
    c1 = np.where(np.abs(area) > 1e-8, c1, 0)
    frac = lambda a: np.where(np.abs(area) > 1e-8, np.abs(a - np.round(a)), 0.5)      # noqa: E731
    margin = np.minimum.reduce([frac(u_lo), frac(u_hi), frac(v_lo), frac(v_hi)])
    return np.stack([c0, c1, r0, r1], 1).astype(np.int64), margin


def box_pixels(boxes):
    c0, c1, r0, r1 = boxes.T
    return np.where((c1 >= c0) & (r1 >= r0), (c1 - c0 + 1) * (r1 - r0 + 1), 0)


def _seg(px, py, ax, ay, bx, by):
    """distance to segment ab and the nearest point"""
    ex, ey = bx - ax, by - ay
    t = np.clip(((px - ax) * ex + (py - ay) * ey) / (ex * ex + ey * ey), 0.0, 1.0)
    qx, qy = ax + t * ex, ay + t * ey
    return np.hypot(qx - px, qy - py), qx, qy


def pairs(verts, faces, S=S0):
    """every (face, pixel of its box) pair in float64: dict of arrays face, pix (r S + c), q (box-relative row-major index),
    cand (the pair is a candidate), z (depth), inside, dist (NDC, nearest edge), edge_margin / blur_margin (pixels)"""
    x, y, z = project(verts)
    boxes, _ = face_boxes(verts, faces, S)
    n = box_pixels(boxes)
    fid = np.repeat(np.arange(len(faces)), n)
    start = np.repeat(np.cumsum(n) - n, n)
    q = np.arange(int(n.sum())) - start
    bw = (boxes[fid, 1] - boxes[fid, 0] + 1)
    rr, cc = boxes[fid, 2] + q // bw, boxes[fid, 0] + q % bw
    px, py = 1.0 - (2.0 * cc + 1.0) / S, 1.0 - (2.0 * rr + 1.0) / S
    f = faces[fid]
    ax, ay, az = x[f[:, 0]], y[f[:, 0]], z[f[:, 0]]
    bx, by, bz = x[f[:, 1]], y[f[:, 1]], z[f[:, 1]]
    cx, cy, cz = x[f[:, 2]], y[f[:, 2]], z[f[:, 2]]
    area = (cx - ax) * (by - ay) - (cy - ay) * (bx - ax)
    live = np.abs(area) > 1e-8                                           # degenerate faces are culled
    area = np.where(live, area, 1.0)
    w0 = ((px - bx) * (cy - by) - (py - by) * (cx - bx)) / area
    w1 = ((px - cx) * (ay - cy) - (py - cy) * (ax - cx)) / area
    w2 = 1.0 - w0 - w1
    inside = (w0 > 0) & (w1 > 0) & (w2 > 0)
    pz = w0 * az + w1 * bz + w2 * cz
    segs = [_seg(px, py, ax, ay, bx, by), _seg(px, py, ax, ay, cx, cy), _seg(px, py, bx, by, cx, cy)]
    d3 = np.stack([sg[0] for sg in segs])
    dist = d3.min(0)
    # two edges (almost) equally near with different nearest points: which one takes the gradient is a float32 coin toss
    tie = np.full(dist.shape, np.inf)
    for i, j in ((0, 1), (0, 2), (1, 2)):
        apart = np.hypot(segs[i][1] - segs[j][1], segs[i][2] - segs[j][2]) > 2e-3 / S     # > 1/1000 px
        near = np.minimum(d3[i], d3[j]) <= dist
        tie = np.where(apart & near, np.minimum(tie, np.abs(d3[i] - d3[j])), tie)
    zmax = np.maximum.reduce([az, bz, cz])
    cand = live & (zmax >= 0) & (pz >= 0) & \
        (inside | (dist * dist < ra.BLUR))
    to_px = S / 2.0
    return dict(face=fid, pix=rr * S + cc, q=q, cand=cand, z=pz, inside=inside, dist=dist,
                edge_margin=dist * to_px, blur_margin=np.abs(dist - R_BLUR) * to_px, tie_margin=tie * to_px)


def per_face(P, F):
    """candidates per face and the largest box-relative index of a candidate (-1: none)"""
    c = P["cand"]
    cnt = np.bincount(P["face"][c], minlength=F)
    qmax = np.full(F, -1)
    np.maximum.at(qmax, P["face"][c], P["q"][c])
    return cnt, qmax


def per_pixel(P, S=S0):
    """{pix: sorted candidate depths}, {pix: face ids in depth order}, {pix: -log2(1 - p) in depth order}"""
    c = P["cand"]
    pix, z, f = P["pix"][c], P["z"][c], P["face"][c]
    d = np.where(P["inside"][c], -1.0, 1.0) * P["dist"][c] ** 2           # signed squared distance
    nlog = np.logaddexp(0.0, -d / ra.SIGMA) / math.log(2.0)             # -log2 sigmoid(d / sigma)
    order = np.lexsort((z, pix))
    pix, z, f, nlog = pix[order], z[order], f[order], nlog[order]
    out_z, out_f, out_l = {}, {}, {}
    for p in np.unique(pix):
        s = np.searchsorted(pix, p), np.searchsorted(pix, p, side="right")
        out_z[int(p)], out_f[int(p)], out_l[int(p)] = z[s[0]:s[1]], f[s[0]:s[1]], nlog[s[0]:s[1]]
    return out_z, out_f, out_l


def margins_ok(P):
    """no pixel centre of any box within MARGIN_PX of an edge (inside / outside is unambiguous), of the blur radius, or of
    a point equally near two edges of a face (the nearest edge, which takes the gradient, is unambiguous)"""
    return bool(np.all(P["edge_margin"] > MARGIN_PX) and np.all(P["blur_margin"] > MARGIN_PX) and
                np.all(P["tie_margin"][P["cand"]] > MARGIN_PX))


# ---- the formats -----------------------------------------------------------------------------------------------------------
def face_format(npx, cnt):
    """what the sweep would pick for a face alone (or with three list-class neighbours)"""
    if npx <= LIST_BOX and cnt <= LIST_LDS:
        return LIST
    return MASKS if npx <= 16 * MASK_ROUNDS else NOLIST


def wave_formats(npx, cnt):
    """per face: one format for each aligned group of four faces (lists only when all four qualify)"""
    out = []
    for w in range(0, len(npx), 4):
        group = [face_format(a, b) for a, b in zip(npx[w:w + 4], cnt[w:w + 4])]
        all_list = all(g == LIST for g in group)
        out += [LIST if all_list else (MASKS if npx[w + i] <= 16 * MASK_ROUNDS else NOLIST) for i in range(len(group))]
    return out


def block_rect(boxes, f0):
    """union rectangle (width, height) of the live boxes of sweep block f0 .. f0 + 31"""
    b = boxes[f0:f0 + SWEEP_FACES]
    live = b[:, 0] <= b[:, 1]
    b = b[live]
    return int(b[:, 1].max() - b[:, 0].min() + 1), int(b[:, 3].max() - b[:, 2].min() + 1)


# ---- the selection rule (raster_select_kernel) and the resolve decision (raster_resolve_kernel) --------------------------
def select_bounds(zs, fill=BAND_FILL_WIDE):
    """(lo, hi, zk, delta) the selection leaves for sorted candidate depths zs (len > K); delta: the chosen half-width
    (0: none chosen, lo = hi = the midpoint between the K-th and the next)"""
    zk, zmn, zmx = zs[K - 1], zs[0], zs[-1]
    nxt = zs[K] if len(zs) > K else math.inf
    delta = BAND_HALF * (zk - zmn) / K
    for _ in range(BAND_TRIES):
        cnt = int(np.sum((zs > zk - delta) & (zs <= zk + delta)))
        if cnt <= fill and zk - delta < zk:
            return zk - delta, (zk + delta if zmx > zk + delta else math.inf), zk, delta
        delta *= 0.5
    mid = 0.5 * (zk + nxt) if nxt < math.inf else zk
    return mid, mid, zk, 0.0


def bound_margin(zs, zk, delta0):
    """smallest distance of a depth to any bound a selection could pick, relative to the smallest half-width"""
    edges = [zk + s * delta0 / 2 ** i for i in range(BAND_TRIES) for s in (-1.0, 1.0)]
    d = min(float(np.min(np.abs(zs - e))) for e in edges)
    return d / (delta0 / 2 ** (BAND_TRIES - 1))


def resolve_action(zs, lo, hi, sat_sum=0.0):
    """the resolve decision for a pixel with sorted candidate depths zs and cached bounds (lo, hi); sat_sum = sum of
    -log2(1 - p) over the candidates <= lo (saturated at >= 26).  Names as in the kernel's comments."""
    c = int(np.sum(zs <= lo))
    b = int(np.sum((zs > lo) & (zs <= hi)))
    need = K - c
    if 0 < c <= K and sat_sum >= 26.0:
        return "saturated"
    if not lo < math.inf:
        return "fresh_done" if c <= K else "fresh_select"
    if need < 0:
        return "need_lt_0"
    if b > BAND_CAP:
        return "band_overflow"
    if need == 0:
        return "need_eq_0"
    if need > b:
        if hi < math.inf:
            return "short"
        return "all_band" if b > 0 else "all_done"
    return "band_wide" if b > BAND_WIDE else "band_narrow"


# ---- scenes ------------------------------------------------------------------------------------------------------------------
def layer_tri(u_e, v_c, z_view, w=4.0, h=2.5, S=S0):
    """a layer: right-pointing wedge whose vertical edge x = u_e spans rows v_c -+ h, apex w pixels to the left"""
    return world_face([(u_e, v_c - h), (u_e, v_c + h), (u_e - w, v_c)], z_view, S)


STACK_COL, STACK_ROW = 30, 31     # the stack's edges run between columns 30 and 31: column 31 sees every layer from outside
SHIFTS = (0.0, 0.1, 0.2, 0.3)


def stack(depths, shifts=None, on=None, u0=STACK_COL + 0.5, v0=STACK_ROW + 0.3, S=S0):
    """len(depths) layers (faces 0 .. N-1, three vertices each) at the given z_view.  Layer i's vertical edge sits shifts[i]
    pixels right of u0, so which layers are the K nearest changes the silhouette; layers with on[i] False are moved off-screen."""
    n = len(depths)
    shifts = np.zeros(n) if shifts is None else np.asarray(shifts)
    on = np.ones(n, bool) if on is None else np.asarray(on)
    verts = []
    for i in range(n):
        if on[i]:
            verts.append(layer_tri(u0 + shifts[i], v0, depths[i], S=S))
        else:
            verts.append(layer_tri(-3 * S, v0, depths[i], S=S))        # off-screen: an empty box
    return np.concatenate(verts), np.arange(3 * n).reshape(n, 3)


def mixed_shifts(n, seed=0):
    return np.asarray(SHIFTS)[np.random.RandomState(seed).randint(0, len(SHIFTS), n)]


def ranked_depths(n, seed=0):
    """layer i at Z0 + GAP * rank(i), the ranks a fixed shuffle: face order is not depth order"""
    return Z0 + GAP * np.random.RandomState(seed + 100).permutation(n).astype(np.float64)


# candidate counts at the stack's full pixels, test (a): K -+ 1, the band queue's wide split and capacity, the candidate cap
STACK_COUNTS = (99, 100, 101, K + 32, K + 33, K + 64, K + 65, 1023, 1024, 1025)


def count_stack(n):
    return stack(ranked_depths(n, n), mixed_shifts(n, n))


def cover_stack(n_cand=150, n_cover=1100):
    """more than COVER_CAP faces whose boxes cover some of the stack's full pixels, only n_cand of them candidates there"""
    depths = ranked_depths(n_cover, 7)
    shifts = mixed_shifts(n_cover, 7)
    verts = []
    for i in range(n_cover):
        if i < n_cand:
            verts.append(layer_tri(STACK_COL + 0.5 + shifts[i], STACK_ROW + 0.3, depths[i]))
        else:                                     # apex 1.6 px below the stack's centre row: more than a blur radius away from
            u_a, v_a = STACK_COL + 0.6, STACK_ROW + 1.87          # the pixels of row 31, whose centres its box still holds
            verts.append(world_face([(u_a, v_a), (u_a - 4, v_a - 2.5), (u_a - 4.3, v_a + 2.2)], depths[i]))
    return np.concatenate(verts), np.arange(3 * n_cover).reshape(n_cover, 3)


def small_face(u, v, z_view):
    """a small face (3 x 2 pixels) at integer-pixel translates of one shape: every translate keeps that shape's margins"""
    return world_face([(u, v - 1.5), (u, v + 1.5), (u - 2, v + NUDGE[0])], z_view)


HIT_PIXEL = (STACK_ROW, STACK_COL + 1)            # (row, col): a full pixel of the stacks (outside every layer)


def hit_stack(n_stack=120, n_groups=HIT_CAP + 1):
    """more than HIT_CAP union boxes (groups of RECT_FACES consecutive faces) containing HIT_PIXEL, while fewer than
    COVER_CAP face boxes and candidates do: n_stack layers at the pixel, then n_groups groups of one small face up-left
    of the pixel, one down-right (neither box holds it, their union does) and six degenerate faces (culled: no box).
    Returns verts, faces (degenerate faces repeat vertex 0)."""
    verts, faces = [], []
    depths, shifts = ranked_depths(n_stack, 11), mixed_shifts(n_stack, 11)
    for i in range(n_stack):
        verts.append(layer_tri(STACK_COL + 0.5 + shifts[i], STACK_ROW + 0.3, depths[i]))
        faces.append([3 * i, 3 * i + 1, 3 * i + 2])
    while len(faces) % RECT_FACES:                  # the stack's last group: padded with degenerate faces
        faces.append([0, 0, 0])
    r, c = HIT_PIXEL
    for g in range(n_groups):
        i, j = g % 15, (g // 15) % 15
        z = Z0 + 0.2 + GAP * g
        for u, v in ((c - 1.5 - i, r - 3 - j), (c + 3.5 + i, r + 3 + j)):
            k = 3 * len(verts)
            verts.append(small_face(u, v, z))
            faces.append([k, k + 1, k + 2])
        faces += [[0, 0, 0]] * (RECT_FACES - 2)
    return np.concatenate(verts), np.asarray(faces, np.int64)


def union_boxes(boxes):
    """(c0, c1, r0, r1) of every group of RECT_FACES consecutive faces (live boxes only; empty: c0 > c1)"""
    out = []
    for g in range(0, len(boxes), RECT_FACES):
        b = boxes[g:g + RECT_FACES]
        b = b[(b[:, 0] <= b[:, 1]) & (b[:, 2] <= b[:, 3])]
        out.append([b[:, 0].min(), b[:, 1].max(), b[:, 2].min(), b[:, 3].max()] if len(b) else [1, 0, 1, 0])
    return np.asarray(out)


def covering(boxes, r, c):
    return int(np.sum((boxes[:, 0] <= c) & (c <= boxes[:, 1]) & (boxes[:, 2] <= r) & (r <= boxes[:, 3])))


def format_faces():
    """faces of chosen box sizes and candidate counts in aligned waves of four (face 4w .. 4w + 3), plus one sweep block of
    32 small faces spread wider than the LDS window.  Returns verts, faces, and per face the class it is named for."""
    tris, names = [], []

    def small(k):                                 # a list-class face: ~35-pixel box, ~15 candidates
        return small_face(4.5 + 7 * (k % 8), 4 + 7 * (k // 8), Z0 + GAP * k)

    def rect_tri(u0, v0, w, h, z, flip=False):
        """right triangle in the box [u0, u0 + w] x [v0, v0 + h] (half-integer corners); flip: right angle at the bottom right"""
        # (the hypotenuse's ends are nudged along the box edges: no pixel centre on it)
        # (and the right angle's corner is moved off the diagonal of pixel centres: no centre equally near both legs)
        if flip:
            return world_face([(u0 + w - NUDGE[2], v0 + NUDGE[3]), (u0 + w - NUDGE[2], v0 + h), (u0 + NUDGE[4], v0 + h)], z)
        return world_face([(u0 + NUDGE[2], v0), (u0 + w - NUDGE[5], v0), (u0 + NUDGE[2], v0 + h - NUDGE[6])], z)

    k = 0
    # wave 0: four list faces
    for _ in range(4):
        tris.append(small(k)); names.append("list"); k += 1
    # wave 1: a face whose 256-pixel box holds exactly LIST_LDS candidates: still lists (the list's last entry is used)
    for _ in range(3):
        tris.append(small(k)); names.append("list"); k += 1
    tris.append(world_face([(40.36, 40.38), (54.42, 44.033), (47.5306, 54.43)], Z0 + 0.5)); names.append("list_full"); k += 1
    # wave 2: a 256-pixel box with LIST_LDS + 1 candidates: the whole wave goes to masks
    for _ in range(3):
        tris.append(small(k)); names.append("masks_by_wave"); k += 1
    tris.append(world_face([(40.34, 40.19), (54.35, 43.6076), (49.0262, 54.43)], Z0 + 0.6)); names.append("masks_list_overflow"); k += 1
    # wave 3: a box of 257..1024 pixels (not listed)
    for _ in range(3):
        tris.append(small(k)); names.append("masks_by_wave"); k += 1
    tris.append(rect_tri(2.5, 40.5, 24, 20, Z0 + 0.7)); names.append("masks_big_box"); k += 1
    # wave 4: a box of exactly 1024 pixels with candidates up to its last pixel (the masks' last round), and one of
    # 1040 pixels (40 x 26) with candidates in its last round: more than the masks cover -> the box is walked
    for _ in range(2):
        tris.append(small(k)); names.append("masks_by_wave"); k += 1
    tris.append(rect_tri(20.5, 20.5, 30, 30, Z0 + 0.8, flip=True)); names.append("masks_1024")
    k += 1
    tris.append(rect_tri(10.5, 30.5, 38, 24, Z0 + 0.9, flip=True)); names.append("nolist_1040")
    k += 1
    # wave 5: a box far beyond 1024 pixels
    for _ in range(3):
        tris.append(small(k)); names.append("masks_by_wave"); k += 1
    tris.append(rect_tri(4.5, 4.5, 50, 50, Z0 + 1.0)); names.append("nolist_big_box"); k += 1
    # faces 24 .. 31: fill the first sweep block with list faces; block 2 (faces 32 .. 63): 32 small faces over 60 x 60 pixels
    while k < 32:
        tris.append(small(k)); names.append("list"); k += 1
    for j in range(32):
        u, v = 3.5 + 8 * (j % 8), 3 + 15 * (j // 8)
        tris.append(world_face([(u, v - 1.5), (u, v + 1.5), (u - 2, v + NUDGE[1])], Z0 + 0.05 + GAP * j)); names.append("clip_block")
    verts = np.concatenate(tris)
    return verts, np.arange(len(verts)).reshape(-1, 3), names


def list_edge_faces():
    """the list capacity alone: a wave of three list faces and one whose 256-pixel box holds exactly LIST_LDS candidates
    (lists: the last entry in use), then one with LIST_LDS + 1 (masks).  Nothing overlaps them, so the pixels of their
    last rows -- the last list entries the sweep appends -- are not saturated and every entry carries gradient."""
    tris = [small_face(4.5 + 7 * k, 4, Z0 + GAP * k) for k in range(3)]
    tris.append(world_face([(40.36, 40.38), (54.42, 44.033), (47.5306, 54.43)], Z0 + 0.5))
    tris += [small_face(4.5 + 7 * k, 18, Z0 + GAP * (k + 3)) for k in range(3)]
    tris.append(world_face([(40.34 - 36, 40.19), (54.35 - 36, 43.6076), (49.0262 - 36, 54.43)], Z0 + 0.6))
    verts = np.concatenate(tris)
    names = ["list"] * 3 + ["list_full"] + ["masks_by_wave"] * 3 + ["masks_list_overflow"]
    return verts, np.arange(len(verts)).reshape(-1, 3), names


# ---- cache transitions, test (b) ---------------------------------------------------------------------------------------------
def cache_sequences():
    """name -> (depths_1, on_1, depths_2, on_2, shifts, transition): two calls on one engine.  Depths by rank: the layer
    ranked j lies at Z0 + GAP j at the first call.  Every transition is reached at the stack's full pixels (all layers
    candidates); the first call's bounds are lo = z_K - delta0, hi = z_K + delta0 with delta0 = 3.96 GAP (8 or fewer
    candidates in that band) -- see tests/test_raster_forms_cpu.py, which derives them from select_bounds."""
    out = {}

    def base(n):                      # (jittered by < 0.1 GAP: no depth lands on a bound a selection could choose)
        j = np.arange(n, dtype=np.float64)
        return Z0 + GAP * (j + JITTER * ((j * 0.6180339887) % 1.0))

    n = 180
    z1 = base(n)
    on = np.ones(n, bool)
    sh = mixed_shifts(n, 3)
    lo, hi, zk, _ = select_bounds(np.sort(z1))          # the bounds call 1 leaves at the full pixels
    c, b = int(np.sum(z1 <= lo)), int(np.sum((z1 > lo) & (z1 <= hi)))
    inband = lambda m: zk - 0.1 * GAP + 0.002 * GAP * np.arange(m)          # noqa: E731  (inside any band a selection picks)
    # steady state: nothing moves (band kernel, narrow); the interior pixels are saturated
    out["band_narrow"] = (z1, on, z1.copy(), on, sh)
    # far layers move into the band: more than 32 entries
    z2 = z1.copy(); z2[110:110 + 38 - b] = inband(38 - b)
    out["band_wide"] = (z1, on, z2, on, sh)
    # near layers move into the band: 65 entries, one past the capacity
    z2 = z1.copy(); z2[c - (65 - b):c] = inband(65 - b)
    out["band_overflow_65"] = (z1, on, z2, on, sh)
    # 70 far layers into the band
    z2 = z1.copy(); z2[105:175] = inband(70)
    out["band_overflow"] = (z1, on, z2, on, sh)
    # everything 10 GAP nearer: more than K at or below lo
    out["need_lt_0"] = (z1, on, z1 - 10 * GAP, on, sh)
    # far layers move in front: exactly K at or below lo
    z2 = z1.copy(); z2[110:110 + K - c] = Z0 - GAP * np.arange(1, K - c + 1)
    out["need_eq_0"] = (z1, on, z2, on, sh)
    # the ten nearest layers move behind everything: the K-th nearest now lies beyond hi (short miss)
    z2 = z1.copy(); z2[0:10] = z1[-1] + GAP * np.arange(1, 11)
    out["short_miss"] = (z1, on, z2, on, sh)
    # a tie at the cut inside the band: layer K moves onto layer K - 1 (identical footprints, so the tie is at every pixel)
    z2 = z1.copy(); z2[K] = z1[K - 1]
    out["band_tie"] = (z1, on, z2, on, np.zeros(n))
    # no bounds yet: 90 layers on the first call, 180 on the second
    on1 = np.zeros(n, bool); on1[:90] = True
    out["fresh_select"] = (z1, on1, z1.copy(), on, sh)
    # hi = inf (101 layers, none beyond the band); then the ten nearest leave the image: c + b < K, the band finishes
    n2 = 101
    z1b, onb, shb = base(n2), np.ones(n2, bool), mixed_shifts(n2, 4)
    lob = select_bounds(np.sort(z1b))[0]
    on2 = onb.copy(); on2[:10] = False
    out["all_band"] = (z1b, onb, z1b.copy(), on2, shb)
    # ... and with the band's layers gone too: nothing to rank, done in resolve
    on3 = on2 & (z1b <= lob)
    out["all_done"] = (z1b, onb, z1b.copy(), on3, shb)
    return out


# ---- image sizes, test (d) ---------------------------------------------------------------------------------------------------
SIZES = (1, 2, 16, 17, 31, 33, 1023, 1024)


def big_triangle_1024(row=1000, offset=0.25, S=1024):
    """one triangle over most of a 1024^2 image whose lower edge runs horizontally `offset` pixels below the centres of
    `row` (inside) and whose right edge is vertical between two columns; checks at rows row - 2 .. row + 3"""
    y_e = 1.0 - (2.0 * row + 1.0) / S - offset * 2.0 / S                    # below row `row` (y decreases with rows)
    x_e = 1.0 - (2.0 * 700 + 1.0) / S + 0.3 * 2.0 / S                       # 0.3 px left of column 700's centre... (x grows left)
    tri = [(x_e, y_e), (-0.99, y_e), (x_e, 0.99)]
    verts = np.stack([ra.world_from_ndc(x, y, 2.0) for x, y in tri])
    checks = []
    for r in range(row - 2, row + 4):
        for c in (100, 400, 698, 699, 700, 701, 702):
            p = ra.pixel_centre(r, c, S)
            checks.append((r, c, ra.single_face_sil(p, tri)))
    return verts, np.array([[0, 1, 2]]), S, checks


def transitions(seq):
    """per pixel of call 2 of a cache sequence: (resolve action, details) given the bounds call 1 leaves (select_bounds with
    the cold call's fill: every bounded pixel was selected, miss rate 1).  Also the smallest bound margin of call 1."""
    z1s, on1, z2s, on2, sh = seq
    zz1, _, _ = per_pixel(pairs(to_f32(stack(z1s, sh, on1)[0]), stack(z1s, sh, on1)[1]))
    zz2, ff2, ll2 = per_pixel(pairs(to_f32(stack(z2s, sh, on2)[0]), stack(z2s, sh, on2)[1]))
    out, worst = {}, math.inf
    for p in set(zz1) | set(zz2):
        z1 = zz1.get(p, np.zeros(0))
        lo, hi, zk1 = math.inf, math.inf, math.inf
        if len(z1) > K:
            lo, hi, zk1, delta = select_bounds(z1)
            worst = min(worst, bound_margin(z1, zk1, BAND_HALF * (zk1 - z1[0]) / K))
        z2 = zz2.get(p, np.zeros(0))
        sat = float(np.sum(ll2[p][z2 <= lo])) if p in ll2 else 0.0
        act = resolve_action(z2, lo, hi, sat)
        out[p] = dict(action=act, lo=lo, hi=hi, c=int(np.sum(z2 <= lo)), b=int(np.sum((z2 > lo) & (z2 <= hi))),
                      n=len(z2), zk=z2[K - 1] if len(z2) >= K else math.inf,
                      tie_at_cut=len(z2) > K and z2[K - 1] == z2[K])
    return out, worst
