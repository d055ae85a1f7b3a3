// The host side of the scan-sequence block as C functions for tests/test_fit3d_sequence_cpu.py: fit3d_sequence_math.h (the row sum,
// the temporal gradient, the loss) and smalfit_plan.h (the block's rules and its plan).  Built by g++ without contraction
// (tests/host_sequence.py), no HIP: the kernel and this shim evaluate the same code, the loss sums in the kernel's order.
#include <cstddef>
#include <vector>

#include "../smalify_amd/csrc/fit3d_sequence_math.h"
#include "../smalify_amd/csrc/smalfit_plan.h"

using namespace smalfit;

namespace {
struct Clips {
  std::vector<int> start, len, mesh_start, mesh_len;
  bool any_long = false;
  Clips(int N, int G, const int* lengths) : start(G), len(G), mesh_start(N), mesh_len(N) {
    int s = 0;
    for (int c = 0; c < G; ++c) {
      start[c] = s; len[c] = lengths[c];
      for (int n = s; n < s + lengths[c]; ++n) { mesh_start[n] = s; mesh_len[n] = lengths[c]; }
      any_long = any_long || lengths[c] > 1;
      s += lengths[c];
    }
  }
};

// S of one term in the order include/smalfit.h words: 256 lanes, lane l taking the elements l, l + 256, ... in ascending order, the
// 64 lanes of a wave by a butterfly (xor 32 .. 1), the four waves in wave order
float term_sum(const Clips& k, int N, int L, const float* x) {
  float lane[256];
  for (int l = 0; l < 256; ++l) {
    float s = 0.f;
    for (int i = l; i < N * L; i += 256) {
      const int n = i / L;
      if (n + 1 < k.mesh_start[n] + k.mesh_len[n]) s = temporal_pair_sq(s, x[i], x[i + L]);
    }
    lane[l] = s;
  }
  for (int o = 32; o > 0; o >>= 1) {
    float next[256];
    for (int l = 0; l < 256; ++l) next[l] = lane[l] + lane[(l & ~63) | ((l & 63) ^ o)];
    for (int l = 0; l < 256; ++l) lane[l] = next[l];
  }
  float t = 0.f;
  for (int w = 0; w < 4; ++w) t += lane[64 * w];
  return t;
}

// one term on x [N][L]: the gradient into g (row stride `stride`, first column `col0`; null: not formed) -> S
float term(const Clips& k, int N, int L, const float* x, float w, float* g, int stride, int col0) {
  const float c = temporal_grad_scale(w, L);
  const float S = term_sum(k, N, L, x);
  for (int n = 0; n < N; ++n) {
    const bool has_prev = n > k.mesh_start[n], has_next = n + 1 < k.mesh_start[n] + k.mesh_len[n];
    for (int e = 0; e < L; ++e) {
      const size_t i = (size_t)n * L + e;
      if (g) {
        float& ge = g[(size_t)n * stride + col0 + e];
        ge = temporal_grad(ge, c, x[i], has_prev ? x[i - L] : 0.f, has_next ? x[i + L] : 0.f, has_prev, has_next);
      }
    }
  }
  return S;
}
}  // namespace

extern "C" {
// smalfit_scan_sequence_couple on host arrays (clip_lengths sum to N; q->losses is a host pointer here); any gradient may be null
void hsq_couple(int N, int G, const int* clip_lengths, const smalfit_sequence_args* q, int nb, const float* grot, const float* jrot,
                const float* trans, float* g_betas, float* g_theta, float* g_trans) {
  const Clips k(N, G, clip_lengths);
  const SequencePlan p = plan_sequence(q, k.any_long, g_betas != nullptr);
  float* losses = q->losses;
  for (int i = 0; i < 4; ++i) losses[i] = 0.f;
  if (!p.launch) return;
  if (p.share) {
    for (int c = 0; c < G; ++c) {
      if (k.len[c] < 2) continue;
      for (int col = 0; col < nb; ++col) {
        const float s = sequence_row_sum(g_betas, nb, col, k.start[c], k.len[c]);
        for (int r = 0; r < k.len[c]; ++r) g_betas[(size_t)(k.start[c] + r) * nb + col] = s;
      }
    }
  }
  if (p.joint) losses[0] = temporal_loss(q->w_temp_joint, term(k, N, kSeqJointLen, jrot, q->w_temp_joint, g_theta, kSeqThetaCols, kSeqGlobalLen), kSeqJointLen);
  if (p.global) losses[1] = temporal_loss(q->w_temp_global, term(k, N, kSeqGlobalLen, grot, q->w_temp_global, g_theta, kSeqThetaCols, 0), kSeqGlobalLen);
  if (p.trans) losses[2] = temporal_loss(q->w_temp_trans, term(k, N, kSeqTransLen, trans, q->w_temp_trans, g_trans, kSeqTransLen, 0), kSeqTransLen);
  losses[3] = temporal_total(losses[0], losses[1], losses[2]);
}
float hsq_row_sum(const float* g, int stride, int col, int start, int len) { return sequence_row_sum(g, stride, col, start, len); }
float hsq_grad(float g, float w, int L, float x, float prev, float next, int has_prev, int has_next) {
  return temporal_grad(g, temporal_grad_scale(w, L), x, prev, next, has_prev != 0, has_next != 0);
}
float hsq_loss(float w, float S, int L) { return temporal_loss(w, S, L); }
const char* hsq_create_refusal(int given, int N, int G, const int* lengths) { return sequence_create_refusal(given != 0, N, G, lengths); }
// facts: handle_meshes, lengths_sum, num_meshes, step, global_rot, joint_rot, trans
const char* hsq_refusal(const smalfit_sequence_args* q, const int* f) {
  return sequence_args_refusal(q, SequenceFacts{f[0], f[1], f[2], f[3] != 0, f[4] != 0, f[5] != 0, f[6] != 0});
}
// out: launch, share, joint, global, trans, blocks (for N meshes in G clips and nb betas).  q may be NULL
void hsq_plan(const smalfit_sequence_args* q, int any_long, int betas_given, int N, int G, int nb, int* out) {
  const SequencePlan p = plan_sequence(q, any_long != 0, betas_given != 0);
  out[0] = p.launch; out[1] = p.share; out[2] = p.joint; out[3] = p.global; out[4] = p.trans;
  out[5] = p.launch ? sequence_blocks(p, N, G, nb) : 0;
}
int hsq_sizeof_args() { return (int)sizeof(smalfit_sequence_args); }
// offsets in the order of the declaration; returns how many
int hsq_offsets(int* out) {
#define OFF(f) offsetof(smalfit_sequence_args, f)
  const size_t o[] = {OFF(share_shape), OFF(w_temp_joint), OFF(w_temp_global), OFF(w_temp_trans), OFF(losses), OFF(step_total)};
#undef OFF
  const int n = (int)(sizeof(o) / sizeof(o[0]));
  for (int i = 0; i < n; ++i) out[i] = (int)o[i];
  return n;
}
}
