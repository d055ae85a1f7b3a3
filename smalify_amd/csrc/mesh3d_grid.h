// The scan index of the surface term's vertex -> surface direction (smalfit_mesh_targets_build_index; worded in include/smalfit.h):
// one uniform grid per target mesh over that mesh's bounding box, built once on the host, walked by grid_nearest of
// kernels_mesh3d.inc and by the host walker of tests/host_scan_index_shim.cpp.  Host + device, SMALFIT_HD as in mesh3d_math.h.
// The index changes no result: a walk ends on the 64-bit key the linear scan forms -- the least float32 point_scan_tri_dist2
// over ALL records of the mesh, the lowest face among equal values -- because it stops only when nothing it has not seen can
// reach or tie that key (scan_walk_done below), and falls back to the linear scan where it cannot show that.
//
// One definition each: sizing (scan_grid_dims), the cell of a coordinate (scan_cell: the builder bins with it, the walker starts
// with it), the cells of a ring (scan_ring_boxes), the lower bound on everything unseen (scan_ring_bound, scan_box_dist), the
// slack (scan_slack), the stopping rule (scan_walk_done), the candidate rule (scan_take), the fallback (scan_max_rings).
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "mesh3d_math.h"

namespace smalfit {

// cell edge h = kScanCellScale sqrt(surface area / faces): a cell is about kScanCellScale^2 faces' worth of surface.  ONE constant;
// EXPERIMENTS.md has what was tried (entries per occupied cell, duplication, device timing)
constexpr float kScanCellScale = 2.0f;
constexpr int kScanMaxDim = 512;              // cells per axis at most
constexpr int kScanMaxCells = 1 << 22;        // cells per mesh at most: 16 MB of offsets
constexpr int kScanOversizeCells = 64;        // a triangle whose box overlaps more cells goes on the mesh's oversize list
constexpr int kScanMaxRings = 48;             // no walk goes past this ring, whatever the mesh (97^3 cells)
constexpr int kScanRingBudget = 2;            // ... nor past a block of kScanRingBudget x the mesh's faces cells: scan_max_rings
// The slack of the stopping rule, in ulp(L) = 2^-23 L, L the largest absolute coordinate of the grid box and the query.  The
// float32 point_scan_tri_dist2 of an unseen triangle may undercut its true distance; tests/test_mesh_score_cpu.py holds the
// distance function to 64 ulp(L) on its 2 M near-surface sliver pairs, and this is four times that bar
constexpr float kScanSlackUlps = 256.f;
// what "rounded down" means for a bound: the cell planes and the differences to the query are float32 values of magnitude <= 2 L,
// some six roundings of at most ulp(L) each (the argument is in DESIGN.md f13); the bound is lowered by this many ulp(L)
constexpr float kScanBoundUlps = 16.f;
constexpr int kScanNoFace = 0x7fffffff;

// one mesh's grid: 64 bytes, read with wave-uniform loads.  Offsets are into the index's shared arrays
struct ScanGrid {
  float lo[3]; float inv_h;     // least corner of the box | 1 / h (0: a degenerate target, one cell)
  float hi[3]; float h;         // greatest corner | cell edge
  int dims[3]; int cells;       // cells per axis | their product
  int cell_base;                // cell_off[cell_base .. cell_base + cells] : CSR offsets into cell_face, absolute
  int entry_base;               // (first entry of this mesh; cell_off[cell_base] == entry_base)
  int over_base, over_count;    // oversize[over_base .. + over_count)
};
static_assert(sizeof(ScanGrid) == 64, "a grid is four 16-byte rows");

SMALFIT_HD float scan_ulp(float L) { return L * 1.1920928955078125e-7f; }   // 2^-23 L
SMALFIT_HD float scan_slack(float L) { return kScanSlackUlps * scan_ulp(L); }

// the cell of a coordinate along one axis.  Monotone in x (a difference, a product with a value >= 0, floor and a clamp are), which
// is all the bound below asks of it; the clamp takes a query outside the box to the border cell and a huge value to no overflow
SMALFIT_HD int scan_cell(float x, float lo, float inv_h, int dim) {
  const float v = floorf((x - lo) * inv_h);
  return (int)fminf(fmaxf(v, 0.f), (float)(dim - 1));   // (fmaxf(NaN, 0) = 0: inf x 0 on a degenerate grid)
}
SMALFIT_HD int scan_cell_index(const ScanGrid& g, int x, int y, int z) { return (z * g.dims[1] + y) * g.dims[0] + x; }

// The last ring a walk over a mesh of `faces` triangles visits before it falls back to the linear scan: the largest r <= kScanMaxRings
// whose block, (2 r + 1)^3 cells, stays within kScanRingBudget x faces.  Reading a cell's offsets costs a lane about half a pair
// test, so the walk gives up about where it has cost what the linear scan will: the worst case stays near the linear scan's cost
// for a small mesh and a dense one alike (measured with a constant 8 rings: a 124 k-face target lost the far state and a 498 k-face
// one the near state to single waves scanning the whole mesh)
SMALFIT_HD int scan_max_rings(int faces) {
  int r = 0;
  while (r < kScanMaxRings && (long long)(2 * r + 3) * (2 * r + 3) * (2 * r + 3) <= (long long)kScanRingBudget * faces) ++r;
  return r;
}

// L of the slack: the largest absolute coordinate of the grid box and the query
SMALFIT_HD float scan_extent(const ScanGrid& g, float qx, float qy, float qz) {
  float L = fmaxf(fabsf(qx), fmaxf(fabsf(qy), fabsf(qz)));
#pragma unroll
  for (int k = 0; k < 3; ++k) L = fmaxf(L, fmaxf(fabsf(g.lo[k]), fabsf(g.hi[k])));
  return L;
}

// the block of cells visited after ring r round cell c: Chebyshev distance <= r, clipped to the grid (inclusive ranges)
struct ScanBlock { int lo[3], hi[3]; };
SMALFIT_HD ScanBlock scan_block(const ScanGrid& g, const int c[3], int r) {
  ScanBlock b;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    b.lo[k] = c[k] - r > 0 ? c[k] - r : 0;
    b.hi[k] = c[k] + r < g.dims[k] - 1 ? c[k] + r : g.dims[k] - 1;
  }
  return b;
}
SMALFIT_HD bool scan_block_whole(const ScanGrid& g, const ScanBlock& b) {
  return b.lo[0] == 0 && b.lo[1] == 0 && b.lo[2] == 0 && b.hi[0] == g.dims[0] - 1 && b.hi[1] == g.dims[1] - 1 && b.hi[2] == g.dims[2] - 1;
}

// Lower bound on the distance from the query to any triangle NOT listed in a cell of block b.  Such a triangle's cell range
// misses the block's in some axis direction in which the block has not reached the grid's border; scan_cell is monotone, so all
// of it lies beyond the plane where the cell index steps past the block there; the clamp of the start cell puts the query on the
// inner side of every such plane.  The minimum over those directions of the query's distance to the plane, lowered by
// kScanBoundUlps ulp(L); +inf when the block is the whole grid
SMALFIT_HD float scan_ring_bound(const ScanGrid& g, const ScanBlock& b, float qx, float qy, float qz, float L) {
  const float q[3] = {qx, qy, qz};
  float bound = INFINITY;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float rel = q[k] - g.lo[k];
    if (b.lo[k] > 0) bound = fminf(bound, rel - (float)b.lo[k] / g.inv_h);
    if (b.hi[k] < g.dims[k] - 1) bound = fminf(bound, (float)(b.hi[k] + 1) / g.inv_h - rel);
  }
  return bound - kScanBoundUlps * scan_ulp(L);
}
// every triangle lies in the grid box: the query's distance to the box, lowered the same way, is a bound too (0 inside)
SMALFIT_HD float scan_box_dist(const ScanGrid& g, float qx, float qy, float qz, float L) {
  const float q[3] = {qx, qy, qz};
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float d = fmaxf(fmaxf(g.lo[k] - q[k], q[k] - g.hi[k]), 0.f);
    s = fmaf(d, d, s);
  }
  return sqrtf(s) - kScanBoundUlps * scan_ulp(L);
}

// The stopping rule, both conditions strict.  (1) sqrt(best d^2) + slack < bound: every unseen triangle's float32 d^2 is above
// best, so none can win or tie.  (2) tau2 finite and (bound - slack)^2 > tau2: every unseen triangle's d^2 is above tau2, and
// mesh3d_surface_hit_kernel<0, true> drops such a match whichever it is
SMALFIT_HD bool scan_walk_done(float best, float bound, float slack, float tau2) {
  if (sqrtf(best) + slack < bound) return true;
  const float b = bound - slack;
  return b > 0.f && b * b > tau2;
}
// whether a finished walk has a key to write: a face was found, and its d^2 is not above tau2 (the hit kernel drops it either way)
SMALFIT_HD bool scan_key_written(float best, int face, float tau2) { return face != kScanNoFace && !(best > tau2); }

// a candidate in any order, met any number of times: the lexicographic (d^2, face) minimum over finite d^2 -- what the linear
// scan's strict '<' over ascending faces arrives at (+inf and NaN never win there either)
SMALFIT_HD void scan_take(float& best, int& face, float d2, int f) {
  if (d2 < best || (d2 == best && d2 != INFINITY && f < face)) {
    best = d2;
    face = f;
  }
}

// the cells of ring r round c, clipped: at most six boxes (the two z slabs, the two y slabs between them, the two x slabs between
// those), box s holding start[s + 1] - start[s] cells in x-fastest order.  Ring 0 is the one cell
struct ScanRing {
  int x0[6], y0[6], z0[6], nx[6], ny[6];
  int start[7];
};
SMALFIT_HD ScanRing scan_ring_boxes(const ScanGrid& g, const int c[3], int r) {
  ScanRing o;
  const ScanBlock b = scan_block(g, c, r);
  // inner ranges: Chebyshev distance < r along that axis
  const int iy0 = c[1] - r + 1 > 0 ? c[1] - r + 1 : 0, iy1 = c[1] + r - 1 < g.dims[1] - 1 ? c[1] + r - 1 : g.dims[1] - 1;
  const int iz0 = c[2] - r + 1 > 0 ? c[2] - r + 1 : 0, iz1 = c[2] + r - 1 < g.dims[2] - 1 ? c[2] + r - 1 : g.dims[2] - 1;
  const int fx = b.hi[0] - b.lo[0] + 1, fy = b.hi[1] - b.lo[1] + 1;
  const int my = iy1 - iy0 + 1, mz = iz1 - iz0 + 1;
  int count[6];
#pragma unroll
  for (int s = 0; s < 6; ++s) {
    const bool far = (s & 1) != 0;                       // the slab at c - r | c + r
    const int axis = 2 - (s >> 1);                       // z, z, y, y, x, x
    const int at = far ? c[axis] + r : c[axis] - r;
    const bool in = r == 0 ? s == 0 : (at >= 0 && at < g.dims[axis]);
    o.x0[s] = axis == 0 ? at : b.lo[0];
    o.y0[s] = axis == 1 ? at : (axis == 2 ? b.lo[1] : iy0);
    o.z0[s] = axis == 2 ? at : iz0;
    o.nx[s] = axis == 0 ? 1 : fx;
    o.ny[s] = axis == 1 ? 1 : (axis == 2 ? fy : my);
    const int nz = axis == 2 ? 1 : mz;
    count[s] = in ? o.nx[s] * o.ny[s] * nz : 0;
  }
  o.start[0] = 0;
#pragma unroll
  for (int s = 0; s < 6; ++s) o.start[s + 1] = o.start[s] + count[s];
  return o;
}
// cell i of the ring (0 <= i < start[6]) -> its index in the grid (selects over the six boxes: no indexed register array)
SMALFIT_HD int scan_ring_cell(const ScanGrid& g, const ScanRing& o, int i) {
  int x0 = o.x0[0], y0 = o.y0[0], z0 = o.z0[0], nx = o.nx[0], ny = o.ny[0], first = 0;
#pragma unroll
  for (int s = 1; s < 6; ++s) {
    const bool here = i >= o.start[s];
    x0 = here ? o.x0[s] : x0;
    y0 = here ? o.y0[s] : y0;
    z0 = here ? o.z0[s] : z0;
    nx = here ? o.nx[s] : nx;
    ny = here ? o.ny[s] : ny;
    first = here ? o.start[s] : first;
  }
  // (an empty box has start[s] == start[s + 1]: a later box with the same start replaces it)
  const unsigned l = (unsigned)(i - first);
  const unsigned row = l / (unsigned)nx, x = l - row * (unsigned)nx;
  const unsigned z = row / (unsigned)ny, y = row - z * (unsigned)ny;
  return scan_cell_index(g, x0 + (int)x, y0 + (int)y, z0 + (int)z);
}

// ---- sizing and binning: host only -----------------------------------------------------------------------------------------------
// dims per axis for a box of these extents holding F faces of this total area: h = scale sqrt(area / F); dims = ceil(extent / h)
// in [1, kScanMaxDim] (a zero extent gives 1); h grows until no axis needs more than kScanMaxDim cells and the product fits
// kScanMaxCells.  A target without area (h = 0) takes its largest extent, or 1, for h.  -> h
inline float scan_grid_dims(const float extent[3], double area, int faces, float scale, int dims[3]) {
  const double emax = std::max((double)extent[0], std::max((double)extent[1], (double)extent[2]));
  double h = (double)scale * std::sqrt(area / (double)std::max(faces, 1));
  if (!(h > 0.0) || !std::isfinite(h)) h = emax > 0.0 ? emax : 1.0;
  h = std::max(h, emax / (double)kScanMaxDim);
  for (;;) {
    const double hf = (double)(float)h;   // the float32 edge the grid keeps: the dims are its own
    long long cells = 1;
    for (int k = 0; k < 3; ++k) {
      const double n = std::ceil((double)extent[k] / hf);
      dims[k] = n < 1.0 ? 1 : (n > (double)kScanMaxDim ? kScanMaxDim : (int)n);
      cells *= dims[k];
    }
    if (cells <= (long long)kScanMaxCells) break;
    h *= 1.0625;
  }
  return (float)h;
}

struct ScanGridHost {
  ScanGrid g{};
  std::vector<int> cell_off;    // [cells + 1], relative to this mesh's first entry
  std::vector<int> cell_face;   // faces ascending inside a cell
  std::vector<int> oversize;    // faces ascending
  int occupied = 0, largest = 0;
};

// the grid of one mesh (verts (V,3) finite, faces (F,3) in range: the callers have checked both).  -> why not, or nullptr
inline const char* build_scan_grid(const float* verts, int V, const int* faces, int F, float scale, ScanGridHost& out) {
  ScanGrid& g = out.g;
  for (int k = 0; k < 3; ++k) g.lo[k] = g.hi[k] = verts[k];
  for (int v = 1; v < V; ++v)
    for (int k = 0; k < 3; ++k) {
      g.lo[k] = std::min(g.lo[k], verts[3 * (size_t)v + k]);
      g.hi[k] = std::max(g.hi[k], verts[3 * (size_t)v + k]);
    }
  double area = 0.0;
  for (int f = 0; f < F; ++f) {
    const float *a = verts + 3 * (size_t)faces[3 * (size_t)f], *b = verts + 3 * (size_t)faces[3 * (size_t)f + 1],
                *c = verts + 3 * (size_t)faces[3 * (size_t)f + 2];
    const double e0[3] = {(double)b[0] - a[0], (double)b[1] - a[1], (double)b[2] - a[2]};
    const double e1[3] = {(double)c[0] - a[0], (double)c[1] - a[1], (double)c[2] - a[2]};
    const double n[3] = {e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]};
    area += 0.5 * std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
  }
  const float extent[3] = {g.hi[0] - g.lo[0], g.hi[1] - g.lo[1], g.hi[2] - g.lo[2]};
  g.h = scan_grid_dims(extent, area, F, scale, g.dims);
  g.inv_h = 1.0f / g.h;
  if (!(g.h > 0.f) || !std::isfinite(g.inv_h) || !std::isfinite(extent[0]) || !std::isfinite(extent[1]) || !std::isfinite(extent[2])) {
    g.inv_h = 0.f;   // every coordinate falls in the one cell
    g.dims[0] = g.dims[1] = g.dims[2] = 1;
  }
  g.cells = g.dims[0] * g.dims[1] * g.dims[2];
  // the cell ranges of every triangle's float32 box: conservative, no triangle / box test
  auto range = [&](int f, int lo[3], int hi[3]) {
    const float *a = verts + 3 * (size_t)faces[3 * (size_t)f], *b = verts + 3 * (size_t)faces[3 * (size_t)f + 1],
                *c = verts + 3 * (size_t)faces[3 * (size_t)f + 2];
    long long n = 1;
    for (int k = 0; k < 3; ++k) {
      lo[k] = scan_cell(std::min(a[k], std::min(b[k], c[k])), g.lo[k], g.inv_h, g.dims[k]);
      hi[k] = scan_cell(std::max(a[k], std::max(b[k], c[k])), g.lo[k], g.inv_h, g.dims[k]);
      n *= hi[k] - lo[k] + 1;
    }
    return n;
  };
  std::vector<long long> count((size_t)g.cells + 1, 0);
  out.oversize.clear();
  long long entries = 0;
  for (int f = 0; f < F; ++f) {
    int lo[3], hi[3];
    const long long n = range(f, lo, hi);
    if (n > kScanOversizeCells) { out.oversize.push_back(f); continue; }
    entries += n;
    for (int z = lo[2]; z <= hi[2]; ++z)
      for (int y = lo[1]; y <= hi[1]; ++y)
        for (int x = lo[0]; x <= hi[0]; ++x) ++count[(size_t)scan_cell_index(g, x, y, z)];
  }
  if (entries > 0x7fffffffLL) return "scan index needs more than 2^31 - 1 entries";
  out.cell_off.assign((size_t)g.cells + 1, 0);
  out.occupied = out.largest = 0;
  for (int c = 0; c < g.cells; ++c) {
    out.cell_off[(size_t)c + 1] = out.cell_off[c] + (int)count[c];
    out.occupied += count[c] > 0 ? 1 : 0;
    out.largest = std::max(out.largest, (int)count[c]);
  }
  out.cell_face.assign((size_t)entries, 0);
  std::vector<int> fill(out.cell_off.begin(), out.cell_off.end() - 1);
  for (int f = 0; f < F; ++f) {   // faces in ascending order: ascending inside every cell
    int lo[3], hi[3];
    if (range(f, lo, hi) > kScanOversizeCells) continue;
    for (int z = lo[2]; z <= hi[2]; ++z)
      for (int y = lo[1]; y <= hi[1]; ++y)
        for (int x = lo[0]; x <= hi[0]; ++x) out.cell_face[(size_t)fill[(size_t)scan_cell_index(g, x, y, z)]++] = f;
  }
  g.cell_base = g.entry_base = g.over_base = 0;
  g.over_count = (int)out.oversize.size();
  return nullptr;
}

}  // namespace smalfit
