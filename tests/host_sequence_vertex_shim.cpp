// The host side of the temporal terms on posed vertices as C functions for tests/test_fit3d_sequence_vertex_cpu.py:
// fit3d_sequence_vertex_math.h (the stencils, the element's total, the losses) and smalfit_plan.h (the block's rules, its plan and
// its grid).  Built by g++ without contraction (tests/host_sequence_vertex.py), no HIP: the kernels and this shim evaluate the
// same code, and the sums run in the kernels' order.
#include <cstddef>
#include <vector>

#include "../smalify_amd/csrc/fit3d_sequence_vertex_math.h"
#include "../smalify_amd/csrc/smalfit_plan.h"

using namespace smalfit;

namespace {
// block_sum of 256 lanes: the 64 lanes of a wave by a butterfly (xor 32 .. 1), the four waves in wave order
float block_sum_256(const float* v) {
  float lane[256], next[256];
  for (int l = 0; l < 256; ++l) lane[l] = v[l];
  for (int o = 32; o > 0; o >>= 1) {
    for (int l = 0; l < 256; ++l) next[l] = lane[l] + lane[(l & ~63) | ((l & 63) ^ o)];
    for (int l = 0; l < 256; ++l) lane[l] = next[l];
  }
  float t = 0.f;
  for (int w = 0; w < 4; ++w) t += lane[64 * w];
  return t;
}
}  // namespace

extern "C" {
// smalfit_scan_sequence_vertex_term on host arrays (clip_lengths sum to N; q->losses is a host pointer here); dverts and dtrans
// may be null
void hsv_term(int N, int G, const int* clip_lengths, const smalfit_sequence_vertex_args* q, int V, const float* verts, float* dverts,
              float* dtrans) {
  std::vector<int> mesh_start(N), mesh_len(N);
  int longest = 0, s0 = 0;
  for (int c = 0; c < G; ++c) {
    for (int n = s0; n < s0 + clip_lengths[c]; ++n) { mesh_start[n] = s0; mesh_len[n] = clip_lengths[c]; }
    longest = clip_lengths[c] > longest ? clip_lengths[c] : longest;
    s0 += clip_lengths[c];
  }
  const SequenceVertexPlan p = plan_sequence_vertex(q, longest);
  float* losses = q->losses;
  for (int i = 0; i < 3; ++i) losses[i] = 0.f;
  if (!p.launch) {
    if (dverts) for (size_t i = 0; i < (size_t)N * V * 3; ++i) dverts[i] = 0.f;
    if (dtrans) for (int i = 0; i < 3 * N; ++i) dtrans[i] = 0.f;
    return;
  }
  const Grid2 g = sequence_vertex_grid(V, N);
  const int L = sequence_vertex_len(V);
  const float c_vel = p.vel ? temporal_grad_scale(q->w_temp_vert_vel, L) : 0.f;
  const float c_acc = p.acc ? temporal_grad_scale(q->w_temp_vert_acc, L) : 0.f;
  std::vector<float> parts(sequence_vertex_partials(V, N));
  const size_t stride = (size_t)V * 3;
  // fit3d_sequence_vertex_kernel: block (b, n), lane = thread
  for (int n = 0; n < g.y; ++n) {
    const SeqVertexPlace pl = sequence_vertex_place(n, mesh_start[n], mesh_len[n]);
    for (int b = 0; b < g.x; ++b) {
      float lanes[kSeqVertexSums][kSeqVertexBlock];
      for (int l = 0; l < kSeqVertexBlock; ++l) {
        const int v = b * kSeqVertexBlock + l;
        float t[3] = {0.f, 0.f, 0.f}, sv = 0.f, sa = 0.f;
        if (v < V) {
          const size_t o = ((size_t)n * V + v) * 3;
          const float* x0 = verts + o;
          for (int k = 0; k < 3; ++k) {
            const float x = x0[k];
            const float xm1 = pl.has_m1 ? x0[k - (ptrdiff_t)stride] : 0.f;
            const float xp1 = pl.has_p1 ? x0[k + stride] : 0.f;
            float D = 0.f, A = 0.f;
            if (p.vel) {
              D = vertex_vel_stencil(x, xm1, xp1, pl.has_m1, pl.has_p1);
              if (pl.has_p1) sv = temporal_pair_sq(sv, x, xp1);
            }
            if (p.acc) {
              const float xm2 = pl.has_m2 ? x0[k - 2 * (ptrdiff_t)stride] : 0.f;
              const float xp2 = pl.has_p2 ? x0[k + 2 * stride] : 0.f;
              A = vertex_acc_stencil5(pl, xm2, xm1, x, xp1, xp2);
              if (pl.centre_0) sa = vertex_accel_sq(sa, vertex_accel(xm1, x, xp1));
            }
            t[k] = vertex_term_grad(c_acc, A, c_vel, D);
            if (dverts) dverts[o + k] = t[k];
          }
        }
        lanes[0][l] = sv; lanes[1][l] = sa; lanes[2][l] = t[0]; lanes[3][l] = t[1]; lanes[4][l] = t[2];
      }
      for (int s = 0; s < kSeqVertexSums; ++s) parts[((size_t)s * N + n) * g.x + b] = block_sum_256(lanes[s]);
    }
  }
  // fit3d_sequence_vertex_finish_kernel: ascending mesh order, then ascending block order
  float S[2] = {0.f, 0.f};
  for (int s = 0; s < 2; ++s)
    for (int i = 0; i < N * g.x; ++i) S[s] += parts[(size_t)s * N * g.x + i];
  if (dtrans)
    for (int n = 0; n < N; ++n)
      for (int k = 0; k < 3; ++k) {
        float d = 0.f;
        for (int b = 0; b < g.x; ++b) d += parts[((size_t)(2 + k) * N + n) * g.x + b];
        dtrans[3 * n + k] = d;
      }
  losses[0] = p.vel ? temporal_loss(q->w_temp_vert_vel, S[0], L) : 0.f;
  losses[1] = p.acc ? temporal_loss(q->w_temp_vert_acc, S[1], L) : 0.f;
  losses[2] = vertex_term_total(losses[0], losses[1]);
}
float hsv_step_total(float base, float parameter_terms, float vertex_terms) { return vertex_step_total(base, parameter_terms, vertex_terms); }
// facts: step, num_verts, verts, handle_meshes, num_meshes.  q may be NULL
const char* hsv_refusal(const smalfit_sequence_vertex_args* q, const int* f) {
  return sequence_vertex_args_refusal(q, SequenceVertexFacts{f[0] != 0, f[1], f[2] != 0, f[3], f[4]});
}
// out: launch, vel, acc, grid x, grid y, the partials' float count (the last three 0 when nothing is launched).  q may be NULL
void hsv_plan(const smalfit_sequence_vertex_args* q, int longest, int V, int N, int* out) {
  const SequenceVertexPlan p = plan_sequence_vertex(q, longest);
  const Grid2 g = sequence_vertex_grid(V, N);
  out[0] = p.launch; out[1] = p.vel; out[2] = p.acc;
  out[3] = p.launch ? g.x : 0; out[4] = p.launch ? g.y : 0; out[5] = p.launch ? (int)sequence_vertex_partials(V, N) : 0;
}
int hsv_sizeof_args() { return (int)sizeof(smalfit_sequence_vertex_args); }
int hsv_sizeof_sequence_args() { return (int)sizeof(smalfit_sequence_args); }
// offsets in the order of the declaration; returns how many
int hsv_offsets(int* out) {
#define OFF(f) offsetof(smalfit_sequence_vertex_args, f)
  const size_t o[] = {OFF(w_temp_vert_vel), OFF(w_temp_vert_acc), OFF(losses), OFF(step_total)};
#undef OFF
  const int n = (int)(sizeof(o) / sizeof(o[0]));
  for (int i = 0; i < n; ++i) out[i] = (int)o[i];
  return n;
}
}
