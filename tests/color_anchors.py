"""Hand-derived known answers for the hard-Phong colour render (reference smal_fitter/p3d_renderer.py:41-59,70-72:
pytorch3d 0.2.5 RasterizationSettings(blur_radius 0, faces_per_pixel 1) + HardPhongShader with PointLights(location (0,0,3)),
a constant vertex colour, white background, no perspective correction, no back-face culling).

The arbiter between the HIP kernels (tests/test_gpu_color.py) and the oracle's restatement (tests/test_color_anchors_cpu.py):
nothing here calls rendering code.  Every scene is a handful of faces whose winning face per pixel is known from its
construction, and a pixel's colour is the formula below, written out once in float64:

    w          screen-space barycentrics of the pixel centre in the projected triangle (raster_anchors.barycentric),
               times area / (area + kEpsilon) as pytorch3d forms them
    pos        sum_k w_k v_k                              (world positions, NOT perspective-corrected)
    n          normalise(sum_k w_k n_k),   n_k = normalise(sum over the faces at vertex k of (v1 - v0) x (v2 - v0))
    l, v       normalise(light - pos), normalise(camera - pos),   light (0,0,3), camera (0,0,2.7)
    cos        n . l
    alpha      max(v . (2 cos n - l), 0) where cos > 0, else 0
    colour     (0.5 + 0.3 max(cos, 0)) c + 0.2 alpha^64

`shade` takes the quantities a wrong implementation would change as arguments, so that a case can name its wrong answers:
another shininess, another light, perspective-corrected weights, weights given to the wrong vertices, unweighted or flat
normals.  Camera and pixel centres are those of tests/raster_anchors.py.
"""
import dataclasses
import itertools

import numpy as np

from tests import raster_anchors as ra

LIGHT = (0.0, 0.0, 3.0)
CAMERA = (0.0, 0.0, ra.CAM_DIST)
AMBIENT, DIFFUSE, SPECULAR, SHININESS = 0.5, 0.3, 0.2, 64.0
DEVICE_BAR = 1e-4                     # tests/test_gpu_color.py: absolute, per channel
REGIME = 10.0 * DEVICE_BAR            # every named wrong answer is at least this far from the right one
WHITE = (1.0, 1.0, 1.0)


@dataclasses.dataclass
class Case:
    name: str
    verts: np.ndarray                 # (frames, V, 3) float64 world
    faces: np.ndarray                 # (F, 3)
    S: int
    colour: tuple
    checks: list                      # [(frame, row, col, rgb (3,) float64)]
    wrong: dict = dataclasses.field(default_factory=dict)     # name -> [(frame, row, col, rgb)] at pixels of `checks`
    white_frames: tuple = ()          # frames whose every pixel is exactly white
    covered_frames: tuple = ()        # frames without a white pixel
    exact: bool = False               # the expected values are float32-exact: the device matches them bit for bit


# ------------------------------------------------------------------------------------------------
# the formula
# ------------------------------------------------------------------------------------------------
def project(v):
    """world -> ((x_ndc, y_ndc), z_view), SURVEY App. A.2"""
    zv = ra.CAM_DIST - v[2]
    return (-ra.S_CAM * v[0] / zv, ra.S_CAM * v[1] / zv), zv


def _unit(x):
    return x / np.linalg.norm(x)


def face_cross(verts, face):
    v0, v1, v2 = (verts[i] for i in face)
    return np.cross(v1 - v0, v2 - v0)           # length = twice the area


def corner_normals(verts, faces, f, normals="area"):
    """the three vertex normals of face f.  area: sum of the incident faces' cross products (pytorch3d); unweighted: sum of
    their unit normals; flat: the face's own normal at all three"""
    if normals == "flat":
        return [_unit(face_cross(verts, faces[f]))] * 3
    out = []
    for v in faces[f]:
        acc = np.zeros(3)
        for g in faces:
            if v in g:
                c = face_cross(verts, g)
                acc += c if normals == "area" else _unit(c)
        out.append(_unit(acc))
    return out


K_EPSILON = 1e-8                      # pytorch3d's kEpsilon


def weights(verts, face, row, col, S, bary="screen"):
    """pytorch3d divides the three edge functions by (area + kEpsilon), area = E(c; a, b) = (c - a) x (b - a) with its sign: the
    weights are the barycentrics times area / (area + kEpsilon) and sum to that, not to 1 (1e-8 .. 1e-7 below or above it here)"""
    tri, zv = zip(*(project(verts[i]) for i in face))
    (ax, ay), (bx, by), (cx, cy) = tri
    area = (cx - ax) * (by - ay) - (cy - ay) * (bx - ax)
    w = np.array(ra.barycentric(ra.pixel_centre(row, col, S), tri)) * (area / (area + K_EPSILON))
    if bary == "perspective":                    # pytorch3d's perspective_correct = True, which the reference leaves off
        w = w / np.array(zv)
        w = w / w.sum()
    return w, np.array(zv)


def shade(verts, faces, f, row, col, S, colour, shininess=SHININESS, light=LIGHT, bary="screen", order=(0, 1, 2),
          normals="area"):
    """the colour of pixel (row, col) if face f wins it.  order: weight order[k] goes to vertex k of the face"""
    faces = [tuple(int(i) for i in g) for g in faces]
    w, _ = weights(verts, faces[f], row, col, S, bary)
    w = w[list(order)]
    vn = corner_normals(verts, faces, f, normals)
    pos = sum(w[k] * verts[faces[f][k]] for k in range(3))
    n = _unit(sum(w[k] * vn[k] for k in range(3)))
    ldir = _unit(np.asarray(light, np.float64) - pos)
    vdir = _unit(np.asarray(CAMERA, np.float64) - pos)
    cos = float(n @ ldir)
    alpha = max(float(vdir @ (2.0 * cos * n - ldir)), 0.0) if cos > 0 else 0.0
    return (AMBIENT + DIFFUSE * max(cos, 0.0)) * np.asarray(colour, np.float64) + SPECULAR * alpha ** shininess


def depth(verts, face, row, col, S):
    """(interpolated view depth, smallest weight) of the face at the pixel"""
    w, zv = weights(verts, face, row, col, S)
    return float(w @ zv), float(w.min())


def interior_pixels(verts, face, S, margin=0.06, count=8):
    """up to `count` pixels spread over the face's interior: every weight above `margin`, on screen"""
    px = [(r, c) for r in range(S) for c in range(S) if depth(verts, face, r, c, S)[1] > margin]
    if count is None:
        return px
    assert len(px) >= count, len(px)
    return [px[(2 * i + 1) * len(px) // (2 * count)] for i in range(count)]


def _tri(ndc, z_view):
    return np.stack([ra.world_from_ndc(x, y, z) for (x, y), z in zip(ndc, z_view)])


def _variants(verts, faces, f, pixels, S, colour, frame=0, **named):
    """name -> [(frame, row, col, rgb)] for shade(..., **kwargs) of every named kwargs"""
    return {name: [(frame, r, c, shade(verts, faces, f, r, c, S, colour, **kw)) for r, c in pixels] for name, kw in named.items()}


ONE_FACE = np.array([[0, 1, 2]])
TWO_FACES = np.array([[0, 1, 2], [3, 4, 5]])
PERMUTATIONS = {"weights_%d%d%d" % p: dict(order=p) for p in itertools.permutations(range(3)) if p != (0, 1, 2)}


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------
FACING_NDC = [(0.75, -0.7), (-0.75, -0.7), (0.0, 0.85)]


def case_facing(S=33, colour=(0.9, 0.3, 0.6)):
    """a triangle at constant view depth 2 facing the camera, odd image size: the centre pixel lies on the optical axis, where
    normal, light direction, reflection and view direction coincide -- cos = alpha = 1, colour 0.8 c + 0.2, the specular peak.
    Off the axis alpha^64 falls off within a few pixels; there shininess 32 and a light at the camera are other colours."""
    verts = _tri(FACING_NDC, [2.0] * 3)
    assert face_cross(verts, (0, 1, 2))[2] > 0 and S % 2 == 1
    h = S // 2
    assert ra.pixel_centre(h, h, S) == (0.0, 0.0)
    peak = AMBIENT + DIFFUSE, SPECULAR
    axis = peak[0] * np.asarray(colour) + peak[1]
    assert np.abs(shade(verts, ONE_FACE, 0, h, h, S, colour) - axis).max() < 1e-15
    off = [(h, h + 3), (h, h - 4), (h - 3, h), (h + 5, h), (h - 2, h + 2), (h + 3, h - 3), (h - 4, h - 1)]
    assert all(depth(verts, (0, 1, 2), r, c, S)[1] > 0.05 for r, c in off)
    checks = [(0, h, h, axis)] + [(0, r, c, shade(verts, ONE_FACE, 0, r, c, S, colour)) for r, c in off]
    wrong = _variants(verts, ONE_FACE, 0, off, S, colour, shininess_32=dict(shininess=32.0), light_at_camera=dict(light=CAMERA))
    return Case("facing", verts[None], ONE_FACE, S, colour, checks, wrong)


TILTED_NDC, TILTED_Z = [(0.85, -0.75), (-0.8, -0.5), (0.05, 0.85)], [1.4, 2.3, 3.2]


def case_tilted(S=64, colour=(0.2, 0.7, 0.95)):
    """three different view depths, large on screen: the world position under a pixel comes from the screen-space weights.
    Perspective-corrected weights, or the weights given to other vertices, put it elsewhere"""
    verts = _tri(TILTED_NDC, TILTED_Z)
    assert face_cross(verts, (0, 1, 2))[2] > 0
    px = interior_pixels(verts, (0, 1, 2), S, margin=0.1)
    checks = [(0, r, c, shade(verts, ONE_FACE, 0, r, c, S, colour)) for r, c in px]
    wrong = _variants(verts, ONE_FACE, 0, px, S, colour, perspective_correct=dict(bary="perspective"), **PERMUTATIONS)
    return Case("tilted", verts[None], ONE_FACE, S, colour, checks, wrong)


def case_back_facing(S=33, colour=(0.9, 0.3, 0.6)):
    """case_facing with the winding reversed: the normal points away from the light.  The face is drawn (no culling) with
    ambient light only: 0.5 c, no diffuse, no specular -- on the device exactly float32(0.5) * float32(c)"""
    verts = _tri(FACING_NDC, [2.0] * 3)[[0, 2, 1]]
    assert face_cross(verts, (0, 1, 2))[2] < 0
    px = interior_pixels(verts, (0, 1, 2), S)
    half = AMBIENT * np.asarray(colour, np.float64)
    for r, c in px:
        assert np.array_equal(shade(verts, ONE_FACE, 0, r, c, S, colour), half)
    return Case("back_facing", verts[None], ONE_FACE, S, colour, [(0, r, c, half) for r, c in px], exact=True)


TENT_FACES = np.array([[0, 1, 2], [1, 0, 3]])


def case_tent(S=64, colour=(0.8, 0.5, 0.1)):
    """two faces over the ridge 0-1, in different planes, areas 3.3 : 1.  The ridge vertices' normals are the area-weighted sum
    of both faces' normals; pixels inside either face see them interpolated with the face's own normal at the third vertex"""
    verts = np.array([[0.0, -0.5, 0.3], [0.0, 0.5, 0.3], [-0.9, 0.0, 0.0], [0.25, 0.0, 0.15]])
    ca, cb = face_cross(verts, TENT_FACES[0]), face_cross(verts, TENT_FACES[1])
    assert ca[2] > 0 and cb[2] > 0 and np.linalg.norm(ca) >= 3.0 * np.linalg.norm(cb)
    assert _unit(ca) @ _unit(cb) < 0.75                                   # different planes
    checks, wrong = [], {"unweighted_normals": [], "flat_normals": []}
    for f, count in ((0, 6), (1, 4)):
        # near the ridge, where the ridge normals weigh most: the weight of the face's own third vertex stays under a half
        px = [p for p in interior_pixels(verts, TENT_FACES[f], S, margin=0.1, count=None)
              if weights(verts, TENT_FACES[f], p[0], p[1], S)[0][2] < 0.5]
        px = px[::max(1, len(px) // count)][:count]
        assert len(px) == count
        checks += [(0, r, c, shade(verts, TENT_FACES, f, r, c, S, colour)) for r, c in px]
        for name, v in _variants(verts, TENT_FACES, f, px, S, colour, unweighted_normals=dict(normals="unweighted"),
                                 flat_normals=dict(normals="flat")).items():
            wrong[name] += v
    return Case("tent", verts[None], TENT_FACES, S, colour, checks, wrong)


def case_depth_order(S=64, colour=(0.3, 0.9, 0.5)):
    """two overlapping triangles of different tilt, the steeper one nearer over the pixels checked; frame 0 has the nearer one
    as face 0, frame 1 as face 1.  The nearer face's colour wins"""
    near = _tri([(0.7, -0.6), (-0.7, -0.6), (0.0, 0.8)], [1.6, 2.2, 1.9])
    far = _tri([(0.8, 0.6), (0.0, -0.85), (-0.8, 0.6)], [2.6, 2.4, 3.1])
    assert face_cross(near, (0, 1, 2))[2] > 0 and face_cross(far, (0, 1, 2))[2] > 0
    frames = np.stack([np.concatenate([near, far]), np.concatenate([far, near])])
    checks, other = [], []
    for n, (fn, ff) in enumerate(((0, 1), (1, 0))):
        v = frames[n]
        px = [p for p in interior_pixels(v, TWO_FACES[fn], S, margin=0.1, count=None) if depth(v, TWO_FACES[ff], p[0], p[1], S)[1] > 0.1]
        assert len(px) >= 6
        px = px[::len(px) // 6][:6]
        for r, c in px:
            assert depth(v, TWO_FACES[fn], r, c, S)[0] < depth(v, TWO_FACES[ff], r, c, S)[0] - 0.1
            checks.append((n, r, c, shade(v, TWO_FACES, fn, r, c, S, colour)))
            other.append((n, r, c, shade(v, TWO_FACES, ff, r, c, S, colour)))
    return Case("depth_order", frames, TWO_FACES, S, colour, checks, {"other_face": other})


def case_depth_tie(S=64, colour=(0.3, 0.9, 0.5)):
    """two coplanar triangles at the same constant view depth that share no vertex: face 1 is face 0 mirrored in the plane
    x = 0, which reverses its winding and leaves coordinates, edge vectors and area equal up to sign -- so the interpolated
    depths are the same number in any arithmetic that is symmetric under negation (with the area above 0.25 the + kEpsilon of
    the denominator is below half a unit in the last place of float32).  Equal depth: the lower face index wins"""
    a = _tri([(0.5, -0.6), (-0.7, -0.5), (-0.1, 0.7)], [2.0] * 3)
    b = a * np.array([-1.0, 1.0, 1.0])
    v = np.concatenate([a, b])
    (pa, _), (pb, _), (pc, _) = (project(x) for x in a)
    area = (pc[0] - pa[0]) * (pb[1] - pa[1]) - (pc[1] - pa[1]) * (pb[0] - pa[0])      # E(c; a, b) of pytorch3d and the kernels
    assert area > 0.25            # positive: over (area + kEpsilon) face 0 is also the (2e-8) nearer one in exact arithmetic
    px = [p for p in interior_pixels(v, TWO_FACES[0], S, margin=0.1, count=None) if depth(v, TWO_FACES[1], p[0], p[1], S)[1] > 0.1]
    assert len(px) >= 6
    px = px[::len(px) // 6][:6]
    checks = [(0, r, c, shade(v, TWO_FACES, 0, r, c, S, colour)) for r, c in px]
    other = [(0, r, c, shade(v, TWO_FACES, 1, r, c, S, colour)) for r, c in px]
    return Case("depth_tie", v[None], TWO_FACES, S, colour, checks, {"other_face": other})


def case_camera_plane(S=64, colour=(0.6, 0.2, 0.9)):
    """raster_anchors.case_behind_camera's face, one vertex behind the camera plane: drawn where the depth interpolated with the
    screen-space weights is >= 0 (frame 0: one pixel coloured by the formula, one exactly white); the same face moved wholly
    behind the camera (frame 1) leaves the image white"""
    world, faces, S, ra_checks = ra.case_behind_camera(S)
    (r0, c0, s0), (r1, c1, s1) = ra_checks
    assert s0 > 0.5 and s1 == 0.0
    pz0, wmin0 = depth(world, (0, 1, 2), r0, c0, S)
    pz1, wmin1 = depth(world, (0, 1, 2), r1, c1, S)
    assert pz0 > 0.05 and wmin0 > 0.02 and pz1 < -0.05 and wmin1 > 0.02
    behind = world + np.array([0.0, 0.0, 2.0])
    assert (ra.CAM_DIST - behind[:, 2] < 0).all()
    checks = [(0, r0, c0, shade(world, faces, 0, r0, c0, S, colour)), (0, r1, c1, np.array(WHITE))]
    return Case("camera_plane", np.stack([world, behind]), ONE_FACE, S, colour, checks, white_frames=(1,))


def case_culled(S=64, colour=(0.6, 0.2, 0.9)):
    """frame 0: raster_anchors.case_degenerate's sliver of area 4e-9 <= kEpsilon, culled as a whole; frame 1: a triangle wholly
    outside the image (beyond x_ndc = 1)"""
    (verts, faces, S, _), _ = ra.case_degenerate(S)
    outside = _tri([(1.2, -0.3), (1.9, -0.2), (1.5, 0.4)], [2.0] * 3)
    return Case("culled", np.stack([verts, outside]), ONE_FACE, S, colour, [], white_frames=(0, 1))


def case_covers_image(S=64, colour=(0.6, 0.2, 0.9)):
    """a tilted triangle whose projection contains the whole image (vertices far outside it: the pixel box of the face is clamped
    to the image): every pixel is coloured, the four corners included"""
    verts = _tri([(5.0, -3.0), (-5.0, -3.0), (0.0, 6.0)], [1.5, 2.5, 2.0])
    assert face_cross(verts, (0, 1, 2))[2] > 0
    px = [(0, 0), (0, S - 1), (S - 1, 0), (S - 1, S - 1), (S // 2, S // 2), (S // 3, S - 2), (S - 1, S // 2)]
    assert all(depth(verts, (0, 1, 2), r, c, S)[1] > 0.05 for r in (0, S - 1) for c in (0, S - 1))
    return Case("covers_image", verts[None], ONE_FACE, S, colour, [(0, r, c, shade(verts, ONE_FACE, 0, r, c, S, colour)) for r, c in px],
                covered_frames=(0,))


def specular_term(verts, faces, f, row, col, S):
    """0.2 alpha^64 alone: the colour of a black mesh"""
    return float(shade(verts, faces, f, row, col, S, (0.0, 0.0, 0.0))[0])


def case_colour_argument(S=33, colour=(0.0, 0.35, 0.8)):
    """three distinct channels, red zero: the red channel is the specular term alone, the other two carry
    (0.5 + 0.3 cos) c on top of it"""
    verts = _tri(FACING_NDC, [2.0] * 3)
    h = S // 2
    px = [(h, h), (h, h + 2), (h - 3, h + 1), (h + 2, h - 4), (h + 6, h)]
    checks = [(0, r, c, shade(verts, ONE_FACE, 0, r, c, S, colour)) for r, c in px]
    for (_, r, c, rgb) in checks:
        assert rgb[0] == specular_term(verts, ONE_FACE, 0, r, c, S) and rgb[1] > rgb[0] and rgb[2] > rgb[1]
    assert abs(checks[0][3][0] - SPECULAR) < 1e-15 and 1e-3 < checks[-1][3][0] < 0.1
    return Case("colour_argument", verts[None], ONE_FACE, S, colour, checks)


def case_frames(S=64, colour=(0.2, 0.7, 0.95)):
    """three frames in one call, each another placement of the one triangle: the tilted triangle, the same moved and turned over
    (back-facing), and a small facing one in a corner.  A wrong frame stride of the z-buffer, the normals or the image shows the
    wrong frame's pixels"""
    t = _tri(TILTED_NDC, TILTED_Z)
    back = _tri([(0.6, 0.7), (-0.8, 0.6), (-0.1, -0.8)], [2.8, 2.2, 1.9])
    small = _tri([(-0.2, 0.2), (-0.9, 0.25), (-0.5, 0.9)], [2.0, 2.1, 1.8])
    assert face_cross(back, (0, 1, 2))[2] < 0 and face_cross(small, (0, 1, 2))[2] > 0
    frames = np.stack([t, back, small])
    checks = []
    for n in range(3):
        px = interior_pixels(frames[n], (0, 1, 2), S, margin=0.1, count=6)
        checks += [(n, r, c, shade(frames[n], ONE_FACE, 0, r, c, S, colour)) for r, c in px]
    # ... and pixels that only one frame covers: white in the others
    for n, m in ((0, 2), (2, 0), (1, 2)):
        px = [p for p in interior_pixels(frames[n], (0, 1, 2), S, margin=0.1, count=None) if depth(frames[m], (0, 1, 2), p[0], p[1], S)[1] < -0.2]
        assert px
        checks.append((m, px[0][0], px[0][1], np.array(WHITE)))
    return Case("frames", frames, ONE_FACE, S, colour, checks)


CASES = (case_facing, case_tilted, case_back_facing, case_tent, case_depth_order, case_depth_tie, case_camera_plane, case_culled,
         case_covers_image, case_colour_argument, case_frames)


def all_cases(_cache={}):
    if not _cache:
        _cache.update((c.name, c) for c in (f() for f in CASES))
    return _cache
