// smalify_amd/csrc/mesh3d_grid.h (the scan index: sizing, binning, the ring bound, the stopping rule, the fallback) with
// mesh3d_math.h and smalfit_plan.h as C functions for tests/test_scan_index_cpu.py and tests/test_gpu_scan_index.py.  Built by g++
// (tests/host_scan_index.py), no HIP.  The builder is the library's; the walker below is the host's restatement of grid_nearest of
// kernels_mesh3d.inc, one query at a time, and takes every decision from the header's own functions -- scan_cell, scan_ring_boxes,
// scan_ring_cell, scan_block, scan_ring_bound, scan_box_dist, scan_slack, scan_walk_done, scan_take, scan_key_written,
// scan_max_rings -- so a fault in any of them shows against the linear scan here, without a GPU.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../smalify_amd/csrc/mesh3d_grid.h"
#include "../smalify_amd/csrc/mesh3d_math.h"
#include "../smalify_amd/csrc/smalfit_plan.h"

using namespace smalfit;

namespace {
struct Index {
  ScanGridHost h;
  std::vector<ScanTri> tris;
};
const unsigned long long kNoKey = ~0ull;
unsigned long long make_key(float d2, int face) {
  uint32_t bits;
  std::memcpy(&bits, &d2, 4);
  return ((unsigned long long)bits << 32) | (unsigned)face;
}
}  // namespace

extern "C" {
// -> the refusal's text (the handle stays null), or nullptr with *out set
const char* hsi_create(const float* verts, int V, const int* faces, int F, float scale, void** out) {
  *out = nullptr;
  Index* ix = new Index();
  const char* why = build_scan_grid(verts, V, faces, F, scale > 0.f ? scale : kScanCellScale, ix->h);
  if (why) {
    delete ix;
    return why;
  }
  ix->tris.resize((size_t)F);
  for (int f = 0; f < F; ++f)
    ix->tris[f] = make_scan_tri(verts + 3 * (size_t)faces[3 * f], verts + 3 * (size_t)faces[3 * f + 1], verts + 3 * (size_t)faces[3 * f + 2]);
  *out = ix;
  return nullptr;
}
void hsi_destroy(void* p) { delete (Index*)p; }
// dims[3], cells, occupied, entries, oversize, largest -> out[8]; bytes as the library counts them
unsigned long long hsi_stats(const void* p, int* out) {
  const ScanGridHost& h = ((const Index*)p)->h;
  out[0] = h.g.dims[0]; out[1] = h.g.dims[1]; out[2] = h.g.dims[2];
  out[3] = h.g.cells; out[4] = h.occupied; out[5] = (int)h.cell_face.size(); out[6] = (int)h.oversize.size(); out[7] = h.largest;
  return sizeof(ScanGrid) + (h.cell_off.size() + h.cell_face.size() + h.oversize.size()) * sizeof(int);
}
float hsi_cell_edge(const void* p) { return ((const Index*)p)->h.g.h; }
void hsi_box(const void* p, float* lo, float* hi) {
  const ScanGrid& g = ((const Index*)p)->h.g;
  for (int k = 0; k < 3; ++k) { lo[k] = g.lo[k]; hi[k] = g.hi[k]; }
}
void hsi_csr(const void* p, int* cell_off, int* cell_face, int* oversize) {
  const ScanGridHost& h = ((const Index*)p)->h;
  std::copy(h.cell_off.begin(), h.cell_off.end(), cell_off);
  std::copy(h.cell_face.begin(), h.cell_face.end(), cell_face);
  std::copy(h.oversize.begin(), h.oversize.end(), oversize);
}

// the linear scan's key of every query: surface_scan_nearest / surface_scan_nearest_compatible over ALL records
void hsi_linear_keys(const void* p, int nq, const float* q, const float* u, int gated, float cc, unsigned long long* keys) {
  const Index& ix = *(const Index*)p;
  const int F = (int)ix.tris.size();
#pragma omp parallel for schedule(dynamic, 64)
  for (int i = 0; i < nq; ++i) {
    float best = INFINITY;
    int face = kScanNoFace;
    const float* x = q + 3 * (size_t)i;
    if (gated) surface_scan_nearest_compatible(x[0], x[1], x[2], u[3 * (size_t)i], u[3 * (size_t)i + 1], u[3 * (size_t)i + 2], cc, ix.tris.data(), 0, F, 0, best, face);
    else surface_scan_nearest(x[0], x[1], x[2], ix.tris.data(), 0, F, 0, best, face);
    keys[i] = face == kScanNoFace ? kNoKey : make_key(best, face);
  }
}

// the walk's key of every query; how[i]: rings walked (1 .. scan_max_rings(faces) + 1) + 100 when it fell back to the linear scan,
// + 1000 when rule (2) of scan_walk_done -- the truncation -- ended it
void hsi_walk_keys(const void* p, int nq, const float* q, const float* u, int gated, float cc, float tau2, unsigned long long* keys,
                   int* how) {
  const Index& ix = *(const Index*)p;
  const ScanGridHost& h = ix.h;
  const ScanGrid& g = h.g;
  const int F = (int)ix.tris.size();
#pragma omp parallel for schedule(dynamic, 64)
  for (int i = 0; i < nq; ++i) {
    const float qx = q[3 * (size_t)i], qy = q[3 * (size_t)i + 1], qz = q[3 * (size_t)i + 2];
    keys[i] = kNoKey;
    how[i] = 0;
    if (!(std::isfinite(qx) && std::isfinite(qy) && std::isfinite(qz))) continue;
    float best = INFINITY;
    int face = kScanNoFace;
    auto test = [&](int f) {
      const ScanTri& t = ix.tris[f];
      const float d2 = point_scan_tri_dist2(qx, qy, qz, t);
      const bool ok = !gated || normal_compatible(u[3 * (size_t)i], u[3 * (size_t)i + 1], u[3 * (size_t)i + 2], t.nx, t.ny, t.nz, t.inv_nn, cc);
      if (ok) scan_take(best, face, d2, f);
    };
    for (int f : h.oversize) test(f);
    const float L = scan_extent(g, qx, qy, qz), slack = scan_slack(L), box = scan_box_dist(g, qx, qy, qz, L);
    const int c[3] = {scan_cell(qx, g.lo[0], g.inv_h, g.dims[0]), scan_cell(qy, g.lo[1], g.inv_h, g.dims[1]),
                      scan_cell(qz, g.lo[2], g.inv_h, g.dims[2])};
    bool done = false;
    int rings = 0;
    const int last = scan_max_rings(F);
    for (int r = 0; r <= last; ++r) {
      const ScanRing ring = scan_ring_boxes(g, c, r);
      for (int k = 0; k < ring.start[6]; ++k) {
        const int ci = scan_ring_cell(g, ring, k);
        for (int e = h.cell_off[ci]; e < h.cell_off[ci + 1]; ++e) test(h.cell_face[e]);
      }
      rings = r + 1;
      const ScanBlock b = scan_block(g, c, r);
      if (scan_block_whole(g, b)) { done = true; break; }
      const float bound = fmaxf(scan_ring_bound(g, b, qx, qy, qz, L), box);
      if (scan_walk_done(best, bound, slack, tau2)) {
        if (!scan_walk_done(best, bound, slack, INFINITY)) how[i] += 1000;
        done = true;
        break;
      }
    }
    how[i] += rings;
    if (!done) {
      how[i] += 100;
      for (int f = 0; f < F; ++f) test(f);
    }
    if (scan_key_written(best, face, tau2)) keys[i] = make_key(best, face);
  }
}

// the cells of ring r round cell c, in the walker's order -> out (at most (2 r + 1)^3), returns how many
int hsi_ring_cells(const void* p, const int* c, int r, int* out) {
  const ScanGrid& g = ((const Index*)p)->h.g;
  const ScanRing ring = scan_ring_boxes(g, c, r);
  for (int k = 0; k < ring.start[6]; ++k) out[k] = scan_ring_cell(g, ring, k);
  return ring.start[6];
}
void hsi_query_cell(const void* p, const float* q, int* c) {
  const ScanGrid& g = ((const Index*)p)->h.g;
  for (int k = 0; k < 3; ++k) c[k] = scan_cell(q[k], g.lo[k], g.inv_h, g.dims[k]);
}
float hsi_grid_dims(const float* extent, double area, int faces, float scale, int* dims) { return scan_grid_dims(extent, area, faces, scale, dims); }
int hsi_max_rings(int faces) { return scan_max_rings(faces); }
void hsi_constants(float* f, int* i) {
  f[0] = kScanCellScale; f[1] = kScanSlackUlps; f[2] = kScanBoundUlps;
  i[0] = kScanMaxDim; i[1] = kScanMaxCells; i[2] = kScanOversizeCells; i[3] = kScanMaxRings; i[4] = kScanGridQueries;
}
void hsi_launch_grids(int V, int N, int* out) {
  const Grid2 a = scan_grid_near_grid(V, N), b = scan_grid_dist_grid(V, N);
  out[0] = a.x; out[1] = a.y; out[2] = b.x; out[3] = b.y;
}
const char* hsi_args_refusal(const smalfit_scan_index_args* a, const float* verts, long long num_floats) {
  return scan_index_args_refusal(a, ScanIndexFacts{verts, (size_t)num_floats});
}
const char* hsi_stats_refusal(const smalfit_scan_index_stats* out, int has_index, int mesh, int num_meshes) {
  return scan_index_stats_refusal(out, has_index != 0, mesh, num_meshes);
}
int hsi_sizeof_args() { return (int)sizeof(smalfit_scan_index_args); }
int hsi_sizeof_stats() { return (int)sizeof(smalfit_scan_index_stats); }
int hsi_sizeof_grid() { return (int)sizeof(ScanGrid); }
int hsi_offsets(int* out) {
  const size_t o[] = {offsetof(smalfit_scan_index_args, struct_size), offsetof(smalfit_scan_index_args, cell_scale),
                      offsetof(smalfit_scan_index_stats, struct_size), offsetof(smalfit_scan_index_stats, dims),
                      offsetof(smalfit_scan_index_stats, cells), offsetof(smalfit_scan_index_stats, occupied_cells),
                      offsetof(smalfit_scan_index_stats, entries), offsetof(smalfit_scan_index_stats, oversize),
                      offsetof(smalfit_scan_index_stats, largest_cell), offsetof(smalfit_scan_index_stats, bytes)};
  const int n = (int)(sizeof(o) / sizeof(o[0]));
  for (int i = 0; i < n; ++i) out[i] = (int)o[i];
  return n;
}
}
