"""Which kernel forms the host picks for an LBS evaluation of M frames -- a restatement of the launch rules, so that the
GPU tests can name the frame counts that reach each form without a compiler, and tests/test_lbs_forms_cpu.py can check both
that the chosen lists cover every form and that the restatement answers like the host's own functions.  Nothing here needs a
GPU.

  skinning forward   smalfit_plan.h: skin_form(M, Vp), padded_verts(V) (run_lbs_forward launches what it returns)
      M > 4 and (Vp / 64) * ceil(M / 16) >= 256  -> skin_mfma_kernel        (64 vertices x 16 frames per workgroup)
      M > 4 otherwise                            -> skin_mfma_split_kernel  (tiles of 16 frames, contraction over 4 waves)
      M <= 4                                     -> skin_kernel<8>
  pose-blend adjoint kernels_lbs_backward.inc:280 (mid_pb_ids): lbs_bwd_mid_kernel takes frames in chunks of
      PBM_TILES tiles of 16 frames, one chunk per ceil(ceil(M / 16) / PBM_TILES)
"""
from __future__ import annotations

NUM_VERTS = 3889                      # the synthetic stand-in's vertex count (and SMAL's)
PBM_TILES = 4                         # smalfit_plan.h: constexpr int PBM_SPLITS = 24, PBM_TILES = 4


def padded_verts(V=NUM_VERTS):
    """Vp: vertex count rounded up to a multiple of 256 (smalfit_model_create)"""
    return (V + 255) // 256 * 256


def frame_tiles(M):
    return (M + 15) // 16


def skin_form(M, V=NUM_VERTS):
    """'plain' (skin_kernel<8>), 'split' (skin_mfma_split_kernel) or 'wide' (skin_mfma_kernel)"""
    if M > 4 and (padded_verts(V) // 64) * frame_tiles(M) >= 256:
        return "wide"
    if M > 4:
        return "split"
    return "plain"


def pose_blend_chunks(M):
    """frame chunks of lbs_bwd_mid_kernel's pose-blend part (tchunk = 0 .. chunks - 1)"""
    return (frame_tiles(M) + PBM_TILES - 1) // PBM_TILES


def ragged_tile(M):
    """the last 16-frame tile is only partly filled"""
    return M % 16 != 0


def same_forms(M1, M2, V=NUM_VERTS):
    """two frame counts that run the same skinning form and the same number of pose-blend chunks"""
    return skin_form(M1, V) == skin_form(M2, V) and pose_blend_chunks(M1) == pose_blend_chunks(M2)


# frame counts of tests/test_gpu_frame_counts.py
LBS_FRAMES = (1, 4, 5, 16, 17, 48, 49, 57, 64, 65, 100, 130)
FIT_FRAMES = (17, 49, 65, 130)
# (M1, M2): frames [0, M1) of an M2-frame call equal an M1-frame call bit for bit (same forms, rows independent)
PREFIX_PAIRS = ((1, 4), (5, 48), (49, 64), (65, 100))
# one frame count per skinning form for the dense-weight and SMAL.__call__-option cases
ONE_PER_FORM = (3, 17, 65)
BETA_COUNTS = (1, 10, 20, 21, 32, 33, 41)
