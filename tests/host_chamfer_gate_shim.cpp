// The host side of the gated chamfer term as C functions for tests/test_chamfer_gate_cpu.py and tests/test_gpu_chamfer_gate.py:
// mesh3d_math.h (GatedScanPoint, quarter_span, scan_records, nearest_merge, chamfer_match, the compatibility predicate) and smalfit_plan.h
// (the gate block's rules, its plan, the staging constants).  Built by g++ (tests/host_chamfer_gate.py), no HIP: the kernels and
// this shim evaluate the same code.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "../smalify_amd/csrc/mesh3d_math.h"
#include "../smalify_amd/csrc/smalfit_plan.h"

using namespace smalfit;

static_assert(sizeof(GatedScanPoint) == kChamGateRecordBytes, "smalfit_plan.h sizes the gated chunk for this record");

extern "C" {
// every query against the scanned set as mesh3d_chamfer_kernel<ROLE, true> does it: the set staged kChamGateChunk records at a
// time, every chunk split in quarters over four waves, each wave with its own running minimum; the four meet through nearest_merge
// and chamfer_match<true, false> decides once.  qn / xn may be NULL (use_cos == 0: nothing is read, c = -inf), xb NULL (no boundary rule), owner
// NULL (no gather).  index: the winner or -1; kept; d2: the winner's d^2 (+inf when none); gather (Q,3): sum (q - x_j) over owner[j] == query
void hcg_scan(int num_queries, const float* q, const float* qn, int num_scanned, const float* x, const float* xn,
              const unsigned char* xb, const int* owner, int use_cos, float c, float tau2, int* index, unsigned char* kept, float* d2,
              float* gather) {
  const float cc = use_cos ? c : -INFINITY;
  std::vector<GatedScanPoint> sp(kChamGateChunk);
  for (int i = 0; i < num_queries; ++i) {
    float best[4], g[4][3];
    int tag[4];
    for (int w = 0; w < 4; ++w) {
      best[w] = INFINITY;
      tag[w] = kNoTag;
      g[w][0] = g[w][1] = g[w][2] = 0.f;
    }
    const float ux = use_cos ? qn[3 * i] : 0.f, uy = use_cos ? qn[3 * i + 1] : 0.f, uz = use_cos ? qn[3 * i + 2] : 0.f;
    for (int base = 0; base < num_scanned; base += kChamGateChunk) {
      const int cnt = std::min(kChamGateChunk, num_scanned - base);
      for (int j = 0; j < cnt; ++j) {
        GatedScanPoint s;
        s.x = x[3 * (size_t)(base + j)]; s.y = x[3 * (size_t)(base + j) + 1]; s.z = x[3 * (size_t)(base + j) + 2];
        s.owner = owner ? owner[base + j] : 0;
        s.nx = s.ny = s.nz = 0.f;
        if (use_cos) { s.nx = xn[3 * (size_t)(base + j)]; s.ny = xn[3 * (size_t)(base + j) + 1]; s.nz = xn[3 * (size_t)(base + j) + 2]; }
        s.tag = gated_tag(base + j, xb ? xb[base + j] : 0);
        sp[j] = s;
      }
      for (int w = 0; w < 4; ++w) {
        const Span s = quarter_span(w, cnt);
        if (owner) scan_records<true, false>(q[3 * i], q[3 * i + 1], q[3 * i + 2], ux, uy, uz, cc, sp.data(), s.b, s.e, base, best[w], tag[w], i, g[w], nullptr);
        else scan_records<false, false>(q[3 * i], q[3 * i + 1], q[3 * i + 2], ux, uy, uz, cc, sp.data(), s.b, s.e, base, best[w], tag[w], i, g[w], nullptr);
      }
    }
    for (int w = 1; w < 4; ++w) {
      nearest_merge(best[0], tag[0], best[w], tag[w]);
      for (int k = 0; k < 3; ++k) g[0][k] += g[w][k];
    }
    const ChamferMatch m = chamfer_match<true, false>(best[0], tag[0], tau2, xb != nullptr, 0.f, true);
    index[i] = m.index;
    kept[i] = m.kept ? 1 : 0;
    d2[i] = best[0];
    if (gather)
      for (int k = 0; k < 3; ++k) gather[3 * (size_t)i + k] = g[0][k];
  }
}
// count independent pairs of unit normals: the float32 dot product and whether they are compatible with c
void hcg_compatible(int count, const float* a, const float* b, float c, float* dot, int* ok) {
  for (int i = 0; i < count; ++i) {
    const size_t o = 3 * (size_t)i;
    dot[i] = dot3(a[o], a[o + 1], a[o + 2], b[o], b[o + 1], b[o + 2]);
    ok[i] = unit_normals_compatible(a[o], a[o + 1], a[o + 2], b[o], b[o + 1], b[o + 2], c) ? 1 : 0;
  }
}
// gated_match alone: -> index, *kept
int hcg_match(float best, int tag, float tau2, int reject, int* kept) {
  const GatedMatch m = gated_match(best, tag, tau2, reject);
  *kept = m.kept ? 1 : 0;
  return m.index;
}
int hcg_tag(int index, int boundary) { return gated_tag(index, boundary); }
// the block is laid out by the caller (the ctypes mirror of smalify_amd/_lib.py); nullptr = accepted
const char* hcg_refusal(const smalfit_chamfer_gate_args* g, int chamfer_on, int step, int step_has_points) {
  return chamfer_gate_args_refusal(g, ChamferGateFacts{chamfer_on != 0, step != 0, step_has_points != 0});
}
// out_i: gated_point, gated_vert, cos_point, cos_vert, boundary, vert_normals, point_normals, point_boundary;
// out_f: c_point, c_vert, tau2_point, tau2_vert.  g may be NULL
void hcg_plan(const smalfit_chamfer_gate_args* g, int chamfer_on, int* out_i, float* out_f) {
  const ChamferGatePlan p = plan_chamfer_gates(g, chamfer_on != 0);
  const bool bi[] = {p.gated_point, p.gated_vert, p.cos_point, p.cos_vert, p.boundary, p.vert_normals, p.point_normals, p.point_boundary};
  for (int i = 0; i < 8; ++i) out_i[i] = bi[i];
  out_f[0] = p.c_point; out_f[1] = p.c_vert; out_f[2] = p.tau2_point; out_f[3] = p.tau2_vert;
}
// chunk, record bytes, LDS bytes of a gated block, the ungated chunk's bytes
void hcg_constants(int* out) {
  out[0] = kChamGateChunk; out[1] = kChamGateRecordBytes; out[2] = kChamGateLdsBytes; out[3] = (int)sizeof(ScanPoint);
}
int hcg_sizeof_args() { return (int)sizeof(smalfit_chamfer_gate_args); }
int hcg_sizeof_surface_gate_args() { return (int)sizeof(smalfit_surface_gate_args); }
int hcg_sizeof_term_args() { return (int)sizeof(smalfit_surface_term_args); }
int hcg_sizeof_fit3d_args() { return (int)sizeof(smalfit_fit3d_args); }
// offsets in the order of the declaration; returns how many
int hcg_offsets(int* out) {
#define OFF(f) offsetof(smalfit_chamfer_gate_args, f)
  const size_t o[] = {OFF(struct_size), OFF(max_dist_point), OFF(max_dist_vert), OFF(min_cos_point), OFF(min_cos_vert),
                      OFF(reject_boundary), OFF(point_normals), OFF(point_boundary), OFF(kept), OFF(point_kept), OFF(vert_kept),
                      OFF(point_nn), OFF(vert_nn)};
#undef OFF
  const int n = (int)(sizeof(o) / sizeof(o[0]));
  for (int i = 0; i < n; ++i) out[i] = (int)o[i];
  return n;
}
}
