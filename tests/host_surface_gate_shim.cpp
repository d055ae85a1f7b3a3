// The host side of the gated surface term as C functions for tests/test_surface_gate_cpu.py and tests/test_gpu_surface_gate.py:
// mesh3d_topology.h (boundary_flags, the vertex -> face CSR), mesh3d_math.h (the compatibility predicate, the compatible scan, the
// boundary rule, the closest point with its winner, the query normals) and smalfit_plan.h (the gate block's rules and plan).
// Built by g++ (tests/host_surface_gate.py), no HIP: the kernels and this shim evaluate the same code.
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "../smalify_amd/csrc/mesh3d_math.h"
#include "../smalify_amd/csrc/mesh3d_topology.h"
#include "../smalify_amd/csrc/smalfit_plan.h"

using namespace smalfit;

extern "C" {
// one byte per face; returns 0, or 1 when the mesh is refused
int hsg_boundary_flags(int V, int F, const int* faces, unsigned char* out) {
  try {
    const std::vector<uint8_t> fl = boundary_flags(V, F, faces);
    std::memcpy(out, fl.data(), fl.size());
  } catch (const std::exception&) {
    return 1;
  }
  return 0;
}
// off (V + 1), vf (3 F) of build_mesh_topology
int hsg_vertex_faces(int V, int F, const int* faces, int* off, int* vf) {
  try {
    const MeshTopologyHost t = build_mesh_topology(V, F, faces);
    std::memcpy(off, t.vf_off.data(), t.vf_off.size() * sizeof(int));
    std::memcpy(vf, t.vf.data(), t.vf.size() * sizeof(int));
  } catch (const std::exception&) {
    return 1;
  }
  return 0;
}
// count independent (unit normal, triangle) pairs: the signed squared cosine and whether the pair is compatible with c
void hsg_compatible(int count, const float* u, const float* a, const float* b, const float* c, float thr, float* ssc, int* ok) {
  const float cc = cos_threshold(thr);
  for (int i = 0; i < count; ++i) {
    const size_t o = 3 * (size_t)i;
    const ScanTri t = make_scan_tri(a + o, b + o, c + o);
    ssc[i] = signed_sq_cos(u[o], u[o + 1], u[o + 2], t.nx, t.ny, t.nz, t.inv_nn);
    ok[i] = normal_compatible(u[o], u[o + 1], u[o + 2], t.nx, t.ny, t.nz, t.inv_nn, cc) ? 1 : 0;
  }
}
int hsg_boundary_match(unsigned flags, int winner, float t) { return boundary_match(flags, winner, t) ? 1 : 0; }
// count independent pairs: point_scan_tri_closest_where (d2, bary, r, winner, t) and point_triangle_closest beside it (d2p, baryp, rp)
void hsg_closest_where(int count, const float* p, const float* a, const float* b, const float* c, float* d2, float* bary, float* r,
                       int* winner, float* t, float* d2p, float* baryp, float* rp) {
  for (int i = 0; i < count; ++i) {
    const size_t o = 3 * (size_t)i;
    const TriHitWhere w = point_scan_tri_closest_where(p[o], p[o + 1], p[o + 2], make_scan_tri(a + o, b + o, c + o));
    const TriHit h = point_triangle_closest(p + o, a + o, b + o, c + o);
    d2[i] = w.h.d2; winner[i] = w.winner; t[i] = w.t; d2p[i] = h.d2;
    for (int k = 0; k < 3; ++k) {
      bary[o + k] = w.h.b[k]; r[o + k] = w.h.r[k];
      baryp[o + k] = h.b[k]; rp[o + k] = h.r[k];
    }
  }
}
// every query against the mesh as the gated kernels do it: the compatible scan in `slices` spans meeting in the 64-bit key, then
// truncation and (flags != NULL) the boundary rule on the face the key names.  use_cos == 0: the ungated scan.
// face -1 / kept 0 / d2, bary, r zero for a dropped query
void hsg_nearest_gated(int num_queries, const float* q, const float* u, const float* verts, int num_faces, const int* faces, int slices,
                       int use_cos, float thr, float tau2, const unsigned char* flags, int* face, unsigned char* kept, float* d2,
                       float* bary, float* r) {
  const int span = surface_slice_span(num_faces, slices);
  const float cc = cos_threshold(thr);
  for (int i = 0; i < num_queries; ++i) {
    const float* p = q + 3 * (size_t)i;
    unsigned long long key = ~0ull;
    for (int z = 0; z < slices; ++z) {
      float best = INFINITY;
      int bidx = 0x7fffffff;
      for (int f = z * span; f < num_faces && f < (z + 1) * span; ++f) {
        const ScanTri t = make_scan_tri(verts + 3 * (size_t)faces[3 * f], verts + 3 * (size_t)faces[3 * f + 1],
                                        verts + 3 * (size_t)faces[3 * f + 2]);
        if (use_cos) surface_scan_nearest_compatible(p[0], p[1], p[2], u[3 * i], u[3 * i + 1], u[3 * i + 2], cc, &t, 0, 1, f, best, bidx);
        else surface_scan_nearest(p[0], p[1], p[2], &t, 0, 1, f, best, bidx);
      }
      if (bidx == 0x7fffffff) continue;
      unsigned bits;
      std::memcpy(&bits, &best, 4);
      const unsigned long long k = ((unsigned long long)bits << 32) | (unsigned)bidx;
      if (k < key) key = k;
    }
    bool keep = key != ~0ull;
    const int f = keep ? (int)(unsigned)(key & 0xFFFFFFFFull) : 0;
    const TriHitWhere w = point_scan_tri_closest_where(
        p[0], p[1], p[2], make_scan_tri(verts + 3 * (size_t)faces[3 * f], verts + 3 * (size_t)faces[3 * f + 1], verts + 3 * (size_t)faces[3 * f + 2]));
    const unsigned bits = (unsigned)(key >> 32);
    float dd;
    std::memcpy(&dd, &bits, 4);
    keep = keep && !(dd > tau2);
    if (flags != nullptr) keep = keep && !boundary_match(flags[f], w.winner, w.t);
    face[i] = keep ? f : -1;
    kept[i] = keep ? 1 : 0;
    d2[i] = keep ? dd : 0.f;
    for (int k = 0; k < 3; ++k) {
      bary[3 * (size_t)i + k] = keep ? w.h.b[k] : 0.f;
      r[3 * (size_t)i + k] = keep ? w.h.r[k] : 0.f;
    }
  }
}
// (V,3) unit normals of the vertices over the CSR of build_mesh_topology
int hsg_vertex_normals(int V, const float* verts, int F, const int* faces, float* out) {
  try {
    const MeshTopologyHost t = build_mesh_topology(V, F, faces);
    for (int v = 0; v < V; ++v) vertex_normal(verts, faces, t.vf_off.data(), t.vf.data(), v, out + 3 * (size_t)v);
  } catch (const std::exception&) {
    return 1;
  }
  return 0;
}
void hsg_face_unit_normals(const float* verts, int F, const int* faces, float* out) {
  for (int f = 0; f < F; ++f)
    face_unit_normal(verts + 3 * (size_t)faces[3 * f], verts + 3 * (size_t)faces[3 * f + 1], verts + 3 * (size_t)faces[3 * f + 2],
                     out + 3 * (size_t)f);
}
// the blocks are laid out by the caller (ctypes mirrors of smalify_amd/_lib.py); nullptr = accepted
const char* hsg_refusal(const smalfit_surface_gate_args* g, const smalfit_surface_term_args* a, int targets, int step, int step_has_points) {
  return surface_gate_args_refusal(g, a, SurfaceGateFacts{targets != 0, step != 0, step_has_points != 0});
}
// out_i: any, cos_point, cos_vert, boundary; out_f: cc_point, cc_vert, tau2_point, tau2_vert.  g may be NULL
void hsg_plan(const smalfit_surface_gate_args* g, int point_dir, int vert_dir, int* out_i, float* out_f) {
  const SurfaceGatePlan p = plan_surface_gates(g, point_dir != 0, vert_dir != 0);
  out_i[0] = p.any; out_i[1] = p.cos_point; out_i[2] = p.cos_vert; out_i[3] = p.boundary;
  out_f[0] = p.cc_point; out_f[1] = p.cc_vert; out_f[2] = p.tau2_point; out_f[3] = p.tau2_vert;
}
int hsg_sizeof_args() { return (int)sizeof(smalfit_surface_gate_args); }
int hsg_sizeof_term_args() { return (int)sizeof(smalfit_surface_term_args); }
int hsg_sizeof_fit3d_args() { return (int)sizeof(smalfit_fit3d_args); }
// offsets in the order of the declaration; returns how many
int hsg_offsets(int* out) {
#define OFF(f) offsetof(smalfit_surface_gate_args, f)
  const size_t o[] = {OFF(struct_size), OFF(max_dist_point), OFF(max_dist_vert), OFF(min_cos_point), OFF(min_cos_vert),
                      OFF(reject_boundary), OFF(point_normals), OFF(kept), OFF(point_kept), OFF(vert_kept), OFF(vert_normals)};
#undef OFF
  const int n = (int)(sizeof(o) / sizeof(o[0]));
  for (int i = 0; i < n; ++i) out[i] = (int)o[i];
  return n;
}
}
