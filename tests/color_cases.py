"""Whole-mesh inputs of the colour render's per-pixel scoring (tests/test_gpu_color.py; tests/test_color_anchors_cpu.py proves
on the oracle that every one of them leaves at most 3 % of its covered pixels undecided).  The mesh is the stand-in posed as
tests/test_visualisation_cpu.py::_posed_mesh poses it (translation z + 1.0), seen four ways, and the `valence` variant of
tests/model_forms.py from the front.  A mesh at or through the camera plane is not among them: there a quarter to two thirds
of the pixels are undecided, and the closed forms of tests/color_anchors.py cover that regime."""
import numpy as np
import torch

from oracle import smal_oracle as so
from smalify_amd import synthetic

COLOUR = (0.85, 0.4, 0.15)            # not config.MESH_COLOR
SIZES = (50, 128)                     # 50: no multiple of 16, 2500 pixels no multiple of 256; 128: faces of several pixels
DECIDED_SHARE = 0.97
ROT_Y180 = np.diag([-1.0, 1.0, -1.0])

_CACHE = {}


def posed_mesh(md, n):
    """(n,V,3) float64: test_visualisation_cpu._posed_mesh on any model"""
    om = so.OracleModel(md)
    sp = synthetic.synthetic_shape_prior()
    gt = synthetic.ground_truth_params(n, seed=7, mean_betas=sp[1][:20], mean_logscale=sp[1][20:26])
    gt["trans"][:, 2] += 1.0
    theta = np.concatenate([gt["global_rotation"][:, None], gt["joint_rotations"]], 1)
    with torch.no_grad():
        vo, _, _, _ = so.smal_forward(om, torch.from_numpy(np.tile(gt["betas"], (n, 1))).double(), torch.from_numpy(theta).double(),
                                      torch.from_numpy(np.tile(gt["log_beta_scales"], (n, 1))).double())
    return (vo + torch.from_numpy(gt["trans"]).double()[:, None]).numpy()


def model(name):
    if name not in _CACHE:
        if name == "standin":
            _CACHE[name] = synthetic.synthetic_model(seed=0, shape_family_id=1)
        else:
            from tests import model_forms as mf
            _CACHE[name] = mf.variant(name)
    return _CACHE[name]


# view -> (model, frames of the call)
VIEWS = {"front": ("standin", 3), "turned": ("standin", 2), "shifted": ("standin", 1), "far": ("standin", 2),
         "valence_front": ("valence", 2)}
INPUTS = [(v, S) for v in ("front", "turned", "shifted", "far") for S in SIZES] + [("valence_front", 128)]


def view(name):
    """-> (model description, verts (frames,V,3) float64)"""
    key = ("view", name)
    if key not in _CACHE:
        mname, n = VIEWS[name]
        md = model(mname)
        v = posed_mesh(md, n)
        if name == "turned":                       # the collage's fifth panel: about the mesh's centre, seen from behind
            c = v.mean(1, keepdims=True)
            v = (v - c) @ ROT_Y180.T
        elif name == "shifted":                    # half off screen
            v = v + np.array([0.9, 0.3, 0.0])
        elif name == "far":                        # a few dozen pixels
            v = v - np.array([0.0, 0.0, 6.0])
        _CACHE[key] = (md, np.ascontiguousarray(v.astype(np.float32).astype(np.float64)))      # what the device is given
    return _CACHE[key]


def scoring(name, S):
    """the float64 image, the float32 oracle's image and hard_phong_winners' maps of one input, computed once"""
    key = ("scoring", name, S)
    if key not in _CACHE:
        md, v = view(name)
        faces = np.asarray(md.faces)
        _CACHE[key] = dict(f64=so.hard_phong_render(v, faces, S, COLOUR), f32=so.hard_phong_render(v, faces, S, COLOUR, dtype=np.float32),
                           **so.hard_phong_winners(v, faces, S))
    return _CACHE[key]


def decided_share(w):
    """per frame: decided pixels / covered pixels (covered: the relaxed set, which contains the exact one, is not empty)"""
    covered = w["exact"] | w["relaxed"]
    return w["decided"].reshape(len(covered), -1).sum(1) / np.maximum(covered.reshape(len(covered), -1).sum(1), 1), covered
