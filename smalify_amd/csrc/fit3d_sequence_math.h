// Per-element maths of the scan-sequence block of the 3-D fitter (include/smalfit.h, "scan sequences"): the shared shape's row
// sum, the temporal terms' gradient and loss.  One definition each, shared by fit3d_sequence_kernel (kernels_mesh3d.inc) and by
// the test-only host shim (tests/host_sequence_shim.cpp).  SMALFIT_HD as in smalfit_math.h.  Every multiply-add is an explicit
// fmaf and no other expression here holds a product next to a sum, so the host (built without contraction) and the device give
// the same bits.
//
// Reference behaviour restated here: smal_fitter/smal_fitter.py:177-190 (get_temporal)
//   F.mse_loss(x[n], x[n + 1]) * w, summed over the pairs   -> temporal_pair_sq / temporal_loss / temporal_grad
#pragma once
#include <math.h>
#include <stddef.h>

#include "smalfit_math.h"

namespace smalfit {

constexpr int kSeqJointLen = 102, kSeqGlobalLen = 3, kSeqTransLen = 3;   // L of the three temporal terms: elements per mesh
constexpr int kSeqThetaCols = 105;                                        // a row of d theta: global_rot | joint_rot

// the shared shape: column `col` of rows start .. start + len - 1 of a row-major [.][stride] array, summed in ascending row order:
// the first row, then one addition per further row (len = 1: the row's own bits)
SMALFIT_HD float sequence_row_sum(const float* g, int stride, int col, int start, int len) {
  float s = g[(size_t)start * stride + col];
  for (int r = 1; r < len; ++r) s += g[(size_t)(start + r) * stride + col];
  return s;
}

// c of the gradient: (2 w) / L, formed once on the host (2 w is exact)
inline float temporal_grad_scale(float w, int L) { return (2.0f * w) / (float)L; }

// one element's gradient with the temporal term's added: the operand order of the two-neighbour form is (x - prev) + (x - next)
SMALFIT_HD float temporal_grad(float g, float c, float x, float prev, float next, bool has_prev, bool has_next) {
  if (has_prev && has_next) return fmaf(c, (x - prev) + (x - next), g);
  if (has_prev) return fmaf(c, x - prev, g);
  if (has_next) return fmaf(c, x - next, g);
  return g;
}

// one pair's element added to a running sum of squared differences
SMALFIT_HD float temporal_pair_sq(float acc, float x, float next) {
  const float d = next - x;
  return fmaf(d, d, acc);
}

// a term's loss from its sum S of squared differences over all pairs and elements
SMALFIT_HD float temporal_loss(float w, float S, int L) { return w * (S / (float)L); }

// the fourth entry of `losses`
SMALFIT_HD float temporal_total(float joint, float global, float trans) { return (joint + global) + trans; }

}  // namespace smalfit
