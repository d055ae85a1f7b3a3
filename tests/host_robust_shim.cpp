// The host side of the robust kernel as C functions for tests/test_robust_cpu.py: mesh3d_math.h (robust_gm, the weighted owner
// gather of the two chamfer scans) and smalfit_plan.h (the block's rules, its plan, the staging constants).  Built by g++
// (tests/host_robust.py), no HIP: the kernels and this shim evaluate the same code.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

#include "../smalify_amd/csrc/mesh3d_math.h"
#include "../smalify_amd/csrc/smalfit_plan.h"

using namespace smalfit;

extern "C" {
// robust_gm on `count` squared distances under s2
void hrb_gm(int count, const float* d2, float s2, float* rho, float* w) {
  for (int i = 0; i < count; ++i) robust_gm(d2[i], s2, rho[i], w[i]);
}
// the float32 square the host forms, and whether the scale is on
float hrb_scale_sq(float sigma) { return robust_scale_sq(sigma); }
int hrb_scale_on(float sigma) { return robust_scale_on(sigma) ? 1 : 0; }
static RobustFacts facts_of(const int* f) { return RobustFacts{f[0] != 0, f[1] != 0, f[2] != 0, f[3] != 0, f[4] != 0}; }
// the block is laid out by the caller (the ctypes mirror of smalify_amd/_lib.py); facts: chamfer_call, surface_call, chamfer_on,
// point_dir, vert_dir; nullptr = accepted
const char* hrb_refusal(const smalfit_robust_args* r, const int* facts) { return robust_args_refusal(r, facts_of(facts)); }
// out_i: chamfer, surface_point, surface_vert, any; out_f: the four s2.  r may be NULL
void hrb_plan(const smalfit_robust_args* r, const int* facts, int* out_i, float* out_f) {
  const RobustPlan p = plan_robust(r, facts_of(facts));
  out_i[0] = p.chamfer; out_i[1] = p.surface_point; out_i[2] = p.surface_vert; out_i[3] = p.any();
  out_f[0] = p.s2_chamfer_point; out_f[1] = p.s2_chamfer_vert; out_f[2] = p.s2_surface_point; out_f[3] = p.s2_surface_vert;
}
// the vertices' side of the ungated robust chamfer kernel for one query: the points staged kChamChunk at a time with their
// weights beside them, a chunk split in quarters over four waves, the partial sums added in wave order
// -> gather[3] = sum over owner[j] == self of wt[j] (q - x_j); returns the nearest point's index
int hrb_weighted_gather(const float* q, int self, int num_points, const float* x, const int* owner, const float* wt, float* gather,
                        float* best_out) {
  constexpr int kChunk = 1024;
  std::vector<ScanPoint> sp(kChunk);
  std::vector<float> sw(kChunk);
  float best[4] = {INFINITY, INFINITY, INFINITY, INFINITY}, g[4][3] = {};
  int idx[4] = {0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff};
  for (int base = 0; base < num_points; base += kChunk) {
    const int cnt = std::min(kChunk, num_points - base);
    for (int j = 0; j < cnt; ++j) {
      sp[j] = ScanPoint{x[3 * (size_t)(base + j)], x[3 * (size_t)(base + j) + 1], x[3 * (size_t)(base + j) + 2], owner[base + j]};
      sw[j] = wt[base + j];
    }
    for (int w = 0; w < 4; ++w) {
      const Span s = quarter_span(w, cnt);
      scan_records<true, true>(q[0], q[1], q[2], 0.f, 0.f, 0.f, 0.f, sp.data(), s.b, s.e, base, best[w], idx[w], self, g[w], sw.data());
    }
  }
  for (int w = 1; w < 4; ++w) {
    nearest_merge(best[0], idx[0], best[w], idx[w]);
    for (int k = 0; k < 3; ++k) g[0][k] += g[w][k];
  }
  for (int k = 0; k < 3; ++k) gather[k] = g[0][k];
  *best_out = best[0];
  return idx[0];
}
void hrb_constants(int* out) { out[0] = kChamRobustLdsBytes; out[1] = kChamGateLdsBytes; out[2] = kChamGateChunk; }
int hrb_sizeof_args() { return (int)sizeof(smalfit_robust_args); }
// offsets in the order of the declaration; returns how many
int hrb_offsets(int* out) {
#define OFF(f) offsetof(smalfit_robust_args, f)
  const size_t o[] = {OFF(struct_size), OFF(sigma_chamfer_point), OFF(sigma_chamfer_vert), OFF(sigma_surface_point),
                      OFF(sigma_surface_vert), OFF(chamfer_weight_sums), OFF(surface_weight_sums), OFF(chamfer_point_weights),
                      OFF(chamfer_vert_weights), OFF(surface_point_weights), OFF(surface_vert_weights)};
#undef OFF
  const int n = (int)(sizeof(o) / sizeof(o[0]));
  for (int i = 0; i < n; ++i) out[i] = (int)o[i];
  return n;
}
}
