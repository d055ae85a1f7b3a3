// Host-side tables of one SMAL model, built once from a smalfit_model_desc that model_desc_refusal accepts: planar bases, the
// sparse forms of the skin weights and of the joint regressor, the rest joints as an affine map of beta, the internal face order
// with the vertex -> corner adjacency, the limb-scale index table.  Every kernel of the library reads them; smalfit_model_create
// copies them to the device in the order of model_tables.  Pure C++ (no HIP): also compiled by the test-only host shim
// (tests/host_plan_shim.cpp), which tests/test_model_pack_cpu.py calls.
#pragma once
#include <algorithm>
#include <array>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/smalfit.h"
#include "smalfit_plan.h"

namespace smalfit {

static const int kDefaultLandmarks[6] = {1863, 26, 2124, 150, 3055, 1097};            // smal_torch.py:176-184

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// host-side staging buffer that later becomes one device allocation
struct Blob {
  std::vector<unsigned char> bytes;
  size_t add(const void* src, size_t n) {
    const size_t off = align_up(bytes.size(), 256);
    bytes.resize(off + n);
    if (src) std::memcpy(bytes.data() + off, src, n);
    return off;
  }
};

struct ModelPackHost {
  int V = 0, Vp = 0, F = 0, NB = 0;
  int Kw = 0, Kj = 0;                        // entries per vertex of the two ELL forms (the largest row count, at least 1)
  std::vector<float> vt, sd, pd;             // planar bases [3][Vp], [NB][3][Vp], [306][3][Vp], zero padded
  std::vector<int> w_j;                      // skin weights, ELL by vertex [Kw][Vp] ...
  std::vector<float> w_val;
  std::vector<int> wc_off, wc_v;             // ... and CSC by joint: [36] offsets, vertices in ascending order
  std::vector<float> wc_val;
  std::vector<int> jr_off, jr_v;             // joint regressor, CSC by joint ...
  std::vector<float> jr_val;
  std::vector<int> jrv_j;                    // ... and ELL by vertex [Kj][Vp]
  std::vector<float> jrv_val;
  std::vector<float> Jt, JS;                 // rest joints = Jt [105] + JS [105][NB] beta
  std::vector<int> faces_int;                // [F][3] in the internal face order
  std::vector<int> vf_off, vf_idx;           // vertex -> its corners (3 face + corner, internal ids) [V+1], [3F + 1]
  std::vector<int> sidx;                     // limb-scale index per (joint, axis), -1: none [105]
};

inline ModelPackHost pack_smal_model(const smalfit_model_desc* d) {
  ModelPackHost p;
  const int V = p.V = d->num_verts, F = p.F = d->num_faces, NB = p.NB = d->num_betas;
  const int Vp = p.Vp = padded_verts(V);
  // planar bases
  std::vector<float>&vt = p.vt, &sd = p.sd, &pd = p.pd;
  vt.assign((size_t)3 * Vp, 0.f); sd.assign((size_t)NB * 3 * Vp, 0.f); pd.assign((size_t)306 * 3 * Vp, 0.f);
  for (int v = 0; v < V; ++v)
    for (int a = 0; a < 3; ++a) vt[(size_t)a * Vp + v] = d->v_template[v * 3 + a];
  for (int k = 0; k < NB; ++k)
    for (int v = 0; v < V; ++v)
      for (int a = 0; a < 3; ++a) sd[((size_t)k * 3 + a) * Vp + v] = d->shapedirs[(size_t)k * 3 * V + 3 * v + a];
  for (int k = 0; k < 306; ++k)
    for (int v = 0; v < V; ++v)
      for (int a = 0; a < 3; ++a) pd[((size_t)k * 3 + a) * Vp + v] = d->posedirs[(size_t)k * 3 * V + 3 * v + a];
  // sparse forms of weights and regressor
  auto build = [&](const float* dense, int& K, std::vector<int>& ell_j, std::vector<float>& ell_v,
                   std::vector<int>& off, std::vector<int>& cv, std::vector<float>& cval) {
    K = 1;
    for (int v = 0; v < V; ++v) {
      int c = 0;
      for (int j = 0; j < 35; ++j) c += dense[v * 35 + j] != 0.f;
      K = std::max(K, c);
    }
    ell_j.assign((size_t)K * Vp, 0);
    ell_v.assign((size_t)K * Vp, 0.f);
    for (int v = 0; v < V; ++v) {
      int c = 0;
      for (int j = 0; j < 35; ++j)
        if (dense[v * 35 + j] != 0.f) { ell_j[(size_t)c * Vp + v] = j; ell_v[(size_t)c * Vp + v] = dense[v * 35 + j]; ++c; }
    }
    off.assign(36, 0);
    cv.clear(); cval.clear();
    for (int j = 0; j < 35; ++j) {
      for (int v = 0; v < V; ++v)
        if (dense[v * 35 + j] != 0.f) { cv.push_back(v); cval.push_back(dense[v * 35 + j]); }
      off[j + 1] = (int)cv.size();
    }
    if (cv.empty()) { cv.push_back(0); cval.push_back(0.f); }
  };
  build(d->weights, p.Kw, p.w_j, p.w_val, p.wc_off, p.wc_v, p.wc_val);
  build(d->J_regressor, p.Kj, p.jrv_j, p.jrv_val, p.jr_off, p.jr_v, p.jr_val);
  // rest joints as an affine function of beta (float64 accumulation)
  const std::vector<int>&jr_off = p.jr_off, &jr_v = p.jr_v;
  const std::vector<float>& jr_val = p.jr_val;
  std::vector<double> Jt64(105, 0.0), JS64((size_t)105 * NB, 0.0);
  for (int j = 0; j < 35; ++j)
    for (int i = jr_off[j]; i < jr_off[j + 1]; ++i) {
      const int v = jr_v[i];
      const double c = jr_val[i];
      for (int a = 0; a < 3; ++a) {
        Jt64[j * 3 + a] += c * d->v_template[v * 3 + a];
        for (int k = 0; k < NB; ++k) JS64[(size_t)(j * 3 + a) * NB + k] += c * d->shapedirs[(size_t)k * 3 * V + 3 * v + a];
      }
    }
  std::vector<float>&Jt = p.Jt, &JS = p.JS;
  Jt.resize(105); JS.resize((size_t)105 * NB);
  for (int i = 0; i < 105; ++i) Jt[i] = (float)Jt64[i];
  for (size_t i = 0; i < JS.size(); ++i) JS[i] = (float)JS64[i];
  // internal face order: Morton order of the template's face centroids, so that consecutive faces are
  // neighbours on the surface (hence on screen, in any pose) -- the rasteriser's sweep blocks rely on it.
  // Face ids never leave the library (gradients are gathered per vertex), so the order is free to choose.
  std::vector<int>& faces_int = p.faces_int;
  faces_int.resize((size_t)F * 3);
  {
    float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {-1e30f, -1e30f, -1e30f};
    std::vector<float> cen((size_t)F * 3);
    for (int f = 0; f < F; ++f)
      for (int a = 0; a < 3; ++a) {
        const float c = (d->v_template[d->faces[f * 3] * 3 + a] + d->v_template[d->faces[f * 3 + 1] * 3 + a] +
                         d->v_template[d->faces[f * 3 + 2] * 3 + a]) / 3.0f;
        cen[(size_t)f * 3 + a] = c;
        lo[a] = std::min(lo[a], c); hi[a] = std::max(hi[a], c);
      }
    std::vector<std::pair<unsigned long long, int>> keyed(F);
    for (int f = 0; f < F; ++f) {
      unsigned long long code = 0;
      for (int a = 0; a < 3; ++a) {
        const float span = hi[a] - lo[a];
        const unsigned q = span > 0.f ? (unsigned)std::min(1023.0f, (cen[(size_t)f * 3 + a] - lo[a]) / span * 1023.0f) : 0u;
        for (int bit = 0; bit < 10; ++bit) code |= (unsigned long long)((q >> bit) & 1u) << (3 * bit + a);
      }
      keyed[f] = {code, f};
    }
    std::stable_sort(keyed.begin(), keyed.end());
    for (int f = 0; f < F; ++f)
      for (int k = 0; k < 3; ++k) faces_int[(size_t)f * 3 + k] = d->faces[keyed[f].second * 3 + k];
  }
  // vertex -> (face, corner) adjacency (internal face ids).  vf_idx ends with one zero entry past the 3 F corners: vertex_bwd_kernel's
  // clamped unconditional loads read vf_idx[vf_off[V]] when the last vertices have no incident face
  std::vector<int>&vf_off = p.vf_off, &vf_idx = p.vf_idx;
  vf_off.assign(V + 1, 0); vf_idx.assign((size_t)F * 3 + 1, 0);
  for (int i = 0; i < F * 3; ++i) vf_off[faces_int[i] + 1]++;
  for (int v = 0; v < V; ++v) vf_off[v + 1] += vf_off[v];
  {
    std::vector<int> cur(vf_off.begin(), vf_off.end() - 1);
    for (int i = 0; i < F * 3; ++i) vf_idx[cur[faces_int[i]]++] = i;
  }
  // limb-scale index per (joint, axis)   (batch_lbs.py:107-121)
  std::vector<int>& sidx = p.sidx;
  sidx.assign(105, -1);
  auto set = [&](int j, int a, int c) { sidx[j * 3 + a] = c; };
  for (int j = 7; j < 25; ++j) {
    if (j == 15 || j == 16) continue;
    set(j, 2, 0); set(j, 0, 1); set(j, 1, 1);
  }
  for (int j = 25; j < 32; ++j) { set(j, 0, 2); set(j, 1, 3); set(j, 2, 3); }
  for (int j = 33; j < 35; ++j) { set(j, 1, 4); set(j, 2, 5); }
  return p;
}

// The tables in the order they lie in the model's device blob (each at the next multiple of 256 bytes: Blob::add), the caller's
// parent table among them.  smalfit_model_create adds them in this order and points ModelDev at the offsets by these names
enum ModelTable { kT_vt, kT_sd, kT_pd, kT_w_j, kT_w_val, kT_wc_off, kT_wc_v, kT_wc_val, kT_jr_off, kT_jr_v, kT_jr_val, kT_jrv_j, kT_jrv_val,
                  kT_Jt, kT_JS, kT_parents, kT_faces, kT_vf_off, kT_vf_idx, kT_sidx, kModelTables };
struct TableRef { const void* data; size_t bytes; };
inline std::array<TableRef, kModelTables> model_tables(const ModelPackHost& p, const int* parents) {
  auto ref = [](const auto& v) { return TableRef{v.data(), v.size() * sizeof(v[0])}; };
  return {{ref(p.vt), ref(p.sd), ref(p.pd), ref(p.w_j), ref(p.w_val), ref(p.wc_off), ref(p.wc_v), ref(p.wc_val), ref(p.jr_off), ref(p.jr_v),
           ref(p.jr_val), ref(p.jrv_j), ref(p.jrv_val), ref(p.Jt), ref(p.JS), TableRef{parents, 35 * sizeof(int)}, ref(p.faces_int),
           ref(p.vf_off), ref(p.vf_idx), ref(p.sidx)}};
}

}  // namespace smalfit
