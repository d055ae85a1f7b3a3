// Host side of the 3D mesh-fitting objective (SURVEY.md §8f row 3): topology upload, target meshes + sampler,
// kernel sequencing, C-ABI.  Included at the end of smalfit_kernels.hip after smalfit_launch.inc.  The tables are built by
// mesh3d_topology.h; which arguments are refused, the grids, the shape of a fit3d step (plan_fit3d) and what its opt-in blocks
// share (plan_fit3d_riders) are smalfit_plan.h; here are the pointers, the allocations, the copies and the launches.
#include "mesh3d_topology.h"

static_assert(kMeshQueries == kChamQueries && kMeshThreads == kMeshBlock, "smalfit_plan.h sizes the grids of the mesh3d kernels");
static_assert(sizeof(ScanTri) == 64 && kSurfaceChunk * sizeof(ScanTri) == 32768, "smalfit_plan.h sizes kSurfaceChunk for 64-byte records");

struct smalfit_mesh_objective {
  Mesh3dTables t{};
  void* tables = nullptr;     // one allocation behind t.*
  void* work = nullptr;       // one allocation behind the work buffers below
  const int* faces = nullptr; // [F][3] as given to create, in the tables' allocation (smalfit_mesh_score scans them)
  int num_faces = 0;
  int max_meshes = 0, max_points = 0;
  int bx = 0, by = 0, bv = 0, bp = 0;
  float* verts = nullptr;
  int* nn_idx = nullptr;
  float *gcham = nullptr, *gedge = nullptr, *lap_unit = nullptr, *gpair = nullptr;
  float *part_cx = nullptr, *part_cy = nullptr, *part_edge = nullptr, *part_lap = nullptr, *part_normal = nullptr,
        *part_dtr = nullptr;
  // smalfit_fit3d_step only: sampled points, gradients handed to Adam
  float *points = nullptr, *dverts = nullptr, *dtrans = nullptr, *gbetas = nullptr;
  // smalfit_mesh_score only: the distances when the caller does not ask for them
  float *vert_dist = nullptr, *point_dist = nullptr;
  // the surface term only: keys [N][V] then [N][S] (one memset), the points' hits, the vertices' residuals, per-block partials
  unsigned long long* surf_keys = nullptr;
  SurfaceHit* surf_hits = nullptr;
  float *surf_res = nullptr, *surf_part_ps = nullptr, *surf_part_vs = nullptr, *surf_part_dtr = nullptr;
  // its gates only: vertex -> incident faces of the fitted topology (in the tables' allocation), the query normals of both
  // directions, per-block kept counts
  const int *vf_off = nullptr, *vf = nullptr;
  float *surf_vnorm = nullptr, *surf_pnorm = nullptr;
  int *surf_part_kp = nullptr, *surf_part_kv = nullptr;
  // the gates of the chamfer term only: the sampled points' boundary bytes, per-block kept counts (the normals are the two above)
  unsigned char* cham_pbound = nullptr;
  int *part_kx = nullptr, *part_ky = nullptr;
  // the robust kernel only: the points' chamfer weights, per-block sums of w of both terms
  float *cham_w = nullptr, *part_wx = nullptr, *part_wy = nullptr, *surf_part_wp = nullptr, *surf_part_wv = nullptr;
};

struct smalfit_mesh_targets {
  MeshTargetsDev d{};
  void* blob = nullptr;
  const ScanTri* tris = nullptr;   // packed [sum F]: the staged records of the surface term's vertex -> surface scan, in the blob
  int max_faces = 0;               // of the largest mesh: what that scan's slice count is sized by
  const unsigned char* bflags = nullptr;   // packed [sum F]: boundary_flags of every mesh, beside the records
  // the scan index (smalfit_mesh_targets_build_index), or none: one allocation of its own, the grids and their shared arrays in it
  void* index = nullptr;
  ScanIndexDev ix{};
  std::vector<smalfit_scan_index_stats> index_stats;   // per mesh, kept for smalfit_mesh_targets_index_stats
};

// (gated, robust) -> the template instantiation: f is called with the two flags as std::bool_constant
template <typename F>
static void with_flags(bool gated, bool robust, F&& f) {
  if (gated && robust) f(std::true_type{}, std::true_type{});
  else if (gated) f(std::true_type{}, std::false_type{});
  else if (robust) f(std::false_type{}, std::true_type{});
  else f(std::false_type{}, std::false_type{});
}
// one dispatcher per templated kernel
template <int ROLE>
static void launch_chamfer(bool gated, bool robust, int blocks, hipStream_t st, const Mesh3dArgs& a) {
  with_flags(gated, robust, [&](auto g, auto r) { mesh3d_chamfer_kernel<ROLE, g.value, r.value><<<dim3(blocks, a.N), 256, 0, st>>>(a); });
}
template <int ROLE>
static void launch_surface_near(bool gated, const Grid3& g3, hipStream_t st, const SurfaceTermArgs& k) {
  with_flags(gated, false, [&](auto g, auto) { mesh3d_surface_near_kernel<ROLE, g.value><<<dim3(g3.x, g3.y, g3.z), 256, 0, st>>>(k); });
}
template <int ROLE>
static void launch_surface_hit(bool gated, bool robust, const Grid2& g2, hipStream_t st, const SurfaceTermArgs& k) {
  with_flags(gated, robust, [&](auto g, auto r) { mesh3d_surface_hit_kernel<ROLE, g.value, r.value><<<dim3(g2.x, g2.y), kMeshBlock, 0, st>>>(k); });
}

// the vertex direction over targets with a scan index: what the walk reads of the term's arguments
static void launch_surface_near_grid(bool gated, const smalfit_mesh_targets* t, hipStream_t st, const SurfaceTermArgs& k) {
  SurfaceGridArgs a{};
  a.N = k.N; a.V = k.V; a.verts = k.verts; a.t = k.t; a.target_tris = k.target_tris; a.ix = t->ix;
  a.keys_v = k.keys_v; a.normals_v = k.normals_v; a.cc_v = k.cc_v; a.tau2_v = k.tau2_v;
  const Grid2 g = scan_grid_near_grid(k.V, k.N);
  if (gated) mesh3d_surface_near_grid_kernel<true><<<dim3(g.x, g.y), 64 * kScanGridQueries, 0, st>>>(a);
  else mesh3d_surface_near_grid_kernel<false><<<dim3(g.x, g.y), 64 * kScanGridQueries, 0, st>>>(a);
}

// one run of the surface term: the block (validated by the callers), what it is evaluated on, and what rides along
struct SurfaceTermRun {
  const smalfit_surface_term_args* term = nullptr;
  const float *verts = nullptr, *points = nullptr;     // [N][V][3] | [N][S][3]
  int num_points = 0;
  // in a step the term's gradient is ADDED to the step's d verts, its planar copy (stride Vp) and d trans, after
  // run_mesh_objective has written them: one float32 addition per coordinate, the addition Stage.step_unfused performs on the
  // stand-alone call's outputs -- the two paths form the same bits
  float *acc_dverts = nullptr, *acc_planar = nullptr, *acc_dtrans = nullptr;
  int Vp = 0;
  const float* step_losses = nullptr;                  // [5] of the step, or null: term->step_total is not written
  const smalfit_surface_gate_args* gate = nullptr;     // validated by the callers; plan_surface_gates says what it switches on
  const smalfit_robust_args* robust = nullptr;         // validated by the callers; plan_robust says what it switches on
  const float* point_normals = nullptr;                // the caller's or the sampler's
  const float* ready_vert_normals = nullptr;           // the step's chamfer gates have gathered them: no gather here
};
// the launches of the surface term.  With no gate block, or every gate off, and no robust block, or its scales off, the launches
// are those of the plain term (the reduce then reads the kept counts and weight sums, if asked for, off the query counts)
static int run_surface_term(smalfit_mesh_objective* m, const smalfit_mesh_targets* t, hipStream_t st, const SurfaceTermRun& r) {
  const smalfit_surface_term_args* a = r.term;
  const smalfit_surface_gate_args* gate = r.gate;
  SurfaceTermArgs k{};
  k.N = a->num_meshes; k.V = m->t.V; k.F = m->num_faces;
  k.w_ps = mesh_weight(a->w_point_surface); k.w_vs = mesh_weight(a->w_vert_surface);
  k.S = k.w_ps > 0.f ? r.num_points : 1;
  k.verts = r.verts; k.points = r.points; k.faces = m->faces;
  if (k.w_vs > 0.f) { k.t = t->d; k.target_tris = t->tris; }
  k.keys_v = m->surf_keys; k.keys_p = m->surf_keys + (size_t)k.N * k.V;
  k.hits = m->surf_hits; k.res_v = m->surf_res;
  k.point_face = a->point_face; k.point_bary = a->point_bary; k.vert_face = a->vert_face; k.vert_bary = a->vert_bary;
  k.point_residual = a->point_residual; k.vert_residual = a->vert_residual;
  k.part_ps = m->surf_part_ps; k.part_vs = m->surf_part_vs; k.part_dtr = m->surf_part_dtr;
  const Grid2 hv = surface_hit_grid(k.V, k.N), hp = surface_hit_grid(k.S, k.N), gg = surface_grad_grid(k.V, k.N);
  k.hv = hv.x; k.hp = hp.x; k.gv = gg.x;
  k.acc_dverts = r.acc_dverts; k.acc_planar = r.acc_planar; k.Vp = r.Vp; k.acc_dtrans = r.acc_dtrans;
  k.dverts = a->dverts; k.dtrans = a->dtrans; k.losses = a->losses; k.rows = a->rows;
  k.step_losses = r.step_losses; k.step_total = r.step_losses ? a->step_total : nullptr;
  const SurfaceGatePlan gp = plan_surface_gates(gate, k.w_ps > 0.f, k.w_vs > 0.f);
  k.cc_v = gp.cc_vert; k.cc_p = gp.cc_point; k.tau2_v = gp.tau2_vert; k.tau2_p = gp.tau2_point;
  k.vf_off = m->vf_off; k.vf = m->vf;
  if (gate) k.kept = gate->kept;
  if (gp.any) {
    if (k.w_vs > 0.f) { k.part_kv = m->surf_part_kv; k.vert_kept = gate->vert_kept; }
    if (k.w_ps > 0.f) { k.part_kp = m->surf_part_kp; k.point_kept = gate->point_kept; }
    if (gp.boundary) k.bflags = t->bflags;
    if (gp.cos_vert) { k.normals_out = gate->vert_normals ? gate->vert_normals : m->surf_vnorm; k.normals_v = r.ready_vert_normals ? r.ready_vert_normals : k.normals_out; }
    if (gp.cos_point) k.normals_p = r.point_normals;
  }
  const RobustPlan rp = plan_robust(r.robust, RobustFacts{false, true, false, k.w_ps > 0.f, k.w_vs > 0.f});
  k.s2_v = rp.s2_surface_vert; k.s2_p = rp.s2_surface_point;
  if (r.robust) k.weight_sums = r.robust->surface_weight_sums;
  if (rp.surface_vert) { k.part_wv = m->surf_part_wv; k.vert_w = r.robust->surface_vert_weights; }
  if (rp.surface_point) { k.part_wp = m->surf_part_wp; k.point_w = r.robust->surface_point_weights; }
  // the keys of the directions that run, all ones: the vertices' come first, the points' behind them
  unsigned long long* first = k.w_vs > 0.f ? k.keys_v : k.keys_p;
  const size_t keys = (size_t)k.N * ((k.w_vs > 0.f ? (size_t)k.V : 0) + (k.w_ps > 0.f ? (size_t)k.S : 0));
  if (keys > 0) HIP_OK(hipMemsetAsync(first, 0xFF, keys * sizeof(unsigned long long), st));
  if (k.w_vs > 0.f) {
    if (gp.cos_vert && !r.ready_vert_normals) {
      const Grid2 gn = vertex_normal_grid(k.V, k.N);
      mesh3d_vertex_normal_kernel<<<dim3(gn.x, gn.y), kMeshBlock, 0, st>>>(k);
      LAUNCH_OK("mesh3d_vertex_normal_kernel");
    }
    if (t->index) {   // the targets carry a scan index: the same keys by the walk over it
      launch_surface_near_grid(gp.cos_vert, t, st, k);
      LAUNCH_OK("mesh3d_surface_near_grid_kernel");
    } else {
      launch_surface_near<0>(gp.cos_vert, surface_near_grid(k.V, t->max_faces, k.N), st, k);
      LAUNCH_OK("mesh3d_surface_near_kernel<0>");
    }
    launch_surface_hit<0>(gp.any, rp.surface_vert, hv, st, k);
    LAUNCH_OK("mesh3d_surface_hit_kernel<0>");
  }
  if (k.w_ps > 0.f) {
    launch_surface_near<1>(gp.cos_point, surface_near_grid(k.S, k.F, k.N), st, k);
    LAUNCH_OK("mesh3d_surface_near_kernel<1>");
    launch_surface_hit<1>(gp.any, rp.surface_point, hp, st, k);
    LAUNCH_OK("mesh3d_surface_hit_kernel<1>");
  }
  mesh3d_surface_grad_kernel<<<dim3(gg.x, gg.y), 64 * kSurfaceGradWaves, 0, st>>>(k);
  LAUNCH_OK("mesh3d_surface_grad_kernel");
  mesh3d_surface_reduce_kernel<<<1, 256, 0, st>>>(k);
  LAUNCH_OK("mesh3d_surface_reduce_kernel");
  return 0;
}

// one evaluation of the objective: inputs, outputs, the opt-in blocks (validated by the callers) and what rides along
struct MeshObjectiveRun {
  int num_meshes = 0, num_points = 0;
  const float* lbs_verts = nullptr;      // [N][V][3], or ...
  const float* lbs_planar = nullptr;     // ... [N][3][Vp]: the engine's planar vertices, read in place
  int Vp = 0;
  const float *trans = nullptr, *deform_verts = nullptr, *points = nullptr;
  const float* weights = nullptr;        // host [4]
  float* verts_out = nullptr;            // or null: the objective's own buffer
  float *losses = nullptr, *dverts = nullptr, *dtrans = nullptr;
  float* dverts_planar = nullptr;        // [N][3][Vp] or null: a second copy where the LBS adjoint reads it
  const smalfit_chamfer_gate_args* gate = nullptr;   // plan_chamfer_gates says what it switches on
  const smalfit_robust_args* robust = nullptr;       // plan_robust says what it switches on
  const float* point_normals = nullptr;              // the caller's or the sampler's
  const unsigned char* point_boundary = nullptr;
  float* vert_normals = nullptr;                     // where the fitted vertex normals go when a compatibility test asks for them
};
// the 6 launches of one evaluation.  Where plan_chamfer_gates / plan_robust switch a direction on, its chamfer launch is the GATED
// / ROBUST instantiation, and mesh3d_vertex_normal_kernel runs between compose and them when a compatibility test reads the
// vertex normals; with the blocks absent or everything off, the launches are those of the plain objective
static int run_mesh_objective(smalfit_mesh_objective* m, hipStream_t st, const MeshObjectiveRun& r) {
  const float wc = mesh_weight(r.weights[0]);
  Mesh3dArgs a{};
  a.N = r.num_meshes; a.V = m->t.V; a.S = mesh_points(wc, r.num_points);
  a.t = m->t;
  a.lbs_verts = r.lbs_verts; a.lbs_planar = r.lbs_planar; a.Vp = r.Vp; a.dverts_planar = r.dverts_planar;
  a.trans = r.trans; a.deform = r.deform_verts;
  a.verts = r.verts_out ? r.verts_out : m->verts;
  a.points = r.points; a.nn_idx = m->nn_idx;
  a.gcham = m->gcham; a.gedge = m->gedge; a.lap_unit = m->lap_unit; a.gpair = m->gpair;
  a.dverts = r.dverts; a.dtrans = r.dtrans; a.losses = r.losses;
  a.w_chamfer = wc; a.w_edge = mesh_weight(r.weights[1]); a.w_normal = mesh_weight(r.weights[2]);
  a.w_laplacian = mesh_weight(r.weights[3]);
  a.part_cx = m->part_cx; a.part_cy = m->part_cy; a.part_edge = m->part_edge; a.part_lap = m->part_lap;
  a.part_normal = m->part_normal; a.part_dtr = m->part_dtr;
  a.bx = mesh_query_blocks(a.S); a.by = m->by; a.bv = m->bv; a.bp = m->bp;
  const smalfit_chamfer_gate_args* gate = r.gate;
  const ChamferGatePlan gp = plan_chamfer_gates(gate, wc > 0.f);
  a.cos_p = gp.c_point; a.cos_v = gp.c_vert; a.tau2_p = gp.tau2_point; a.tau2_v = gp.tau2_vert;
  if (gate) a.kept = gate->kept;
  if (gp.gated_point) { a.part_kx = m->part_kx; a.point_kept = gate->point_kept; a.point_nn = gate->point_nn; }
  if (gp.gated_vert) { a.part_ky = m->part_ky; a.vert_kept = gate->vert_kept; a.vert_nn = gate->vert_nn; }
  if (gp.point_boundary) a.bound_p = r.point_boundary;
  if (gp.vert_normals) { a.normals_v = r.vert_normals; a.normals_p = r.point_normals; }
  const RobustPlan rp = plan_robust(r.robust, RobustFacts{true, false, wc > 0.f, false, false});
  a.s2_p = rp.s2_chamfer_point; a.s2_v = rp.s2_chamfer_vert;
  if (r.robust) a.weight_sums = r.robust->chamfer_weight_sums;
  if (rp.chamfer) {
    a.wts = m->cham_w; a.part_wx = m->part_wx; a.part_wy = m->part_wy;
    a.point_w = r.robust->chamfer_point_weights; a.vert_w = r.robust->chamfer_vert_weights;
  }
  mesh3d_compose_kernel<<<dim3(mesh_compose_blocks(a.N, a.V)), 256, 0, st>>>(a);
  LAUNCH_OK("mesh3d_compose_kernel");
  if (gp.vert_normals) {
    SurfaceTermArgs k{};
    k.N = a.N; k.V = a.V; k.verts = a.verts; k.faces = m->faces; k.vf_off = m->vf_off; k.vf = m->vf; k.normals_out = r.vert_normals;
    const Grid2 gn = vertex_normal_grid(k.V, k.N);
    mesh3d_vertex_normal_kernel<<<dim3(gn.x, gn.y), kMeshBlock, 0, st>>>(k);
    LAUNCH_OK("mesh3d_vertex_normal_kernel");
  }
  if (wc > 0.f) {
    launch_chamfer<0>(gp.gated_point, rp.chamfer, a.bx, st, a);
    LAUNCH_OK("mesh3d_chamfer_kernel<0>");
    launch_chamfer<1>(gp.gated_vert, rp.chamfer, a.by, st, a);
    LAUNCH_OK("mesh3d_chamfer_kernel<1>");
  } else {
    HIP_OK(hipMemsetAsync(m->gcham, 0, (size_t)a.N * a.V * 3 * sizeof(float), st));
  }
  mesh3d_ring_kernel<<<dim3(a.bv + a.bp, a.N), kMeshBlock, 0, st>>>(a);
  LAUNCH_OK("mesh3d_ring_kernel");
  mesh3d_gather_kernel<<<dim3(a.bv, a.N), kMeshBlock, 0, st>>>(a);
  LAUNCH_OK("mesh3d_gather_kernel");
  mesh3d_reduce_kernel<<<1, 256, 0, st>>>(a);
  LAUNCH_OK("mesh3d_reduce_kernel");
  return 0;
}

// sample_points_from_meshes: num_points per target mesh into points (N,S,3)
// ... and, with `normals` (N,S,3) / `boundary` (N,S), the unit normal / the boundary byte of every point's face
static int launch_mesh_sampler(const smalfit_mesh_targets* t, hipStream_t st, int num_points, unsigned long long seed,
                               unsigned int iteration, float* points, float* normals = nullptr, unsigned char* boundary = nullptr) {
  const Grid2 grid = mesh_sample_grid(num_points, t->d.N);
  const uint32_t lo = (uint32_t)(seed & 0xFFFFFFFFull), hi = (uint32_t)(seed >> 32);
  if (normals || boundary)
    mesh3d_sample_kernel<true><<<dim3(grid.x, grid.y), 256, 0, st>>>(t->d, num_points, lo, hi, iteration, points, normals, boundary, t->bflags);
  else mesh3d_sample_kernel<false><<<dim3(grid.x, grid.y), 256, 0, st>>>(t->d, num_points, lo, hi, iteration, points, nullptr, nullptr, nullptr);
  LAUNCH_OK("mesh3d_sample_kernel");
  return 0;
}

// the body of every smalfit_fit3d_step*, defined behind them with the scan-sequence blocks it optionally takes
static int fit3d_step_run(const char* who, smalfit_engine* e, smalfit_mesh_objective* m, smalfit_mesh_targets* t, void* stream,
                          const smalfit_fit3d_args* a, const smalfit_surface_term_args* sf, const smalfit_surface_gate_args* gate,
                          const smalfit_chamfer_gate_args* cg, const smalfit_robust_args* rb, smalfit_scan_sequence* seq,
                          const smalfit_sequence_args* q, const smalfit_sequence_vertex_args* vq = nullptr);

extern "C" {

int smalfit_mesh_objective_create(int num_verts, int num_faces, const int* faces, int max_meshes, int max_points,
                                  smalfit_mesh_objective** out) {
  if (refused("smalfit_mesh_objective_create", mesh_objective_create_refusal(faces && out, max_meshes, max_points))) return 1;
  MeshTopologyHost h;
  try {
    h = build_mesh_topology(num_verts, num_faces, faces);
  } catch (const std::exception& ex) {
    return refused("smalfit_mesh_objective_create", ex.what());
  }
  Blob b;
  if (h.pairs.empty()) h.pairs.assign(4, 0);   // keep the carve non-empty; P stays 0
  if (h.inc.empty()) h.inc.assign(1, 0);
  const size_t o_no = b.add(h.nbr_off.data(), h.nbr_off.size() * sizeof(int));
  const size_t o_nb = b.add(h.nbr.data(), h.nbr.size() * sizeof(int));
  const size_t o_pr = b.add(h.pairs.data(), h.pairs.size() * sizeof(int));
  const size_t o_io = b.add(h.inc_off.data(), h.inc_off.size() * sizeof(int));
  const size_t o_in = b.add(h.inc.data(), h.inc.size() * sizeof(int));
  const size_t o_fc = b.add(faces, (size_t)num_faces * 3 * sizeof(int));   // (build_mesh_topology has checked every index)
  const size_t o_vo = b.add(h.vf_off.data(), h.vf_off.size() * sizeof(int));
  const size_t o_vf = b.add(h.vf.data(), h.vf.size() * sizeof(int));
  unsigned char* base = upload_blob(b, "smalfit_mesh_objective_create");
  if (!base) return 1;
  auto* m = new smalfit_mesh_objective();
  m->tables = base;
  m->t.V = h.V; m->t.E = h.E; m->t.P = h.P;
  m->t.nbr_off = (const int*)(base + o_no); m->t.nbr = (const int*)(base + o_nb);
  m->t.pairs = (const int*)(base + o_pr);
  m->t.inc_off = (const int*)(base + o_io); m->t.inc = (const int*)(base + o_in);
  m->faces = (const int*)(base + o_fc); m->num_faces = num_faces;
  m->vf_off = (const int*)(base + o_vo); m->vf = (const int*)(base + o_vf);
  m->max_meshes = max_meshes; m->max_points = max_points;
  const size_t N = max_meshes, V = h.V, P = std::max(h.P, 1), S = max_points;
  const MeshGrids grids = mesh_grids(max_points, h.V, h.P);   // (bx: the capacity; an evaluation's own follows its num_points)
  m->bx = grids.bx; m->by = grids.by; m->bv = grids.bv; m->bp = grids.bp;
  Carver w;
  w.field(m->verts, N * V * 3);
  w.field(m->nn_idx, N * S);
  w.field(m->gcham, N * V * 3);
  w.field(m->gedge, N * V * 3);
  w.field(m->lap_unit, N * V * 3);
  w.field(m->gpair, N * P * 12);
  w.field(m->part_cx, N * m->bx);
  w.field(m->part_cy, N * m->by);
  w.field(m->part_edge, N * m->bv);
  w.field(m->part_lap, N * m->bv);
  w.field(m->part_normal, N * std::max(m->bp, 1));
  w.field(m->part_dtr, N * m->bv * 3);
  w.field(m->points, N * S * 3);
  w.field(m->dverts, N * V * 3);
  w.field(m->dtrans, N * 3);
  w.field(m->gbetas, N * 64);
  w.field(m->vert_dist, N * V);
  w.field(m->point_dist, N * S);
  w.field(m->surf_keys, N * (V + S));
  w.field(m->surf_hits, N * S);
  w.field(m->surf_res, N * V * 3);
  w.field(m->surf_part_ps, N * (size_t)surface_hit_grid((int)S, 1).x);
  w.field(m->surf_part_vs, N * (size_t)surface_hit_grid((int)V, 1).x);
  w.field(m->surf_part_dtr, N * m->by * 3);
  w.field(m->surf_vnorm, N * V * 3);
  w.field(m->surf_pnorm, N * S * 3);
  w.field(m->surf_part_kp, N * (size_t)surface_hit_grid((int)S, 1).x);
  w.field(m->surf_part_kv, N * (size_t)surface_hit_grid((int)V, 1).x);
  w.field(m->cham_pbound, N * S);
  w.field(m->part_kx, N * m->bx);
  w.field(m->part_ky, N * m->by);
  w.field(m->cham_w, N * S);
  w.field(m->part_wx, N * m->bx);
  w.field(m->part_wy, N * m->by);
  w.field(m->surf_part_wp, N * (size_t)surface_hit_grid((int)S, 1).x);
  w.field(m->surf_part_wv, N * (size_t)surface_hit_grid((int)V, 1).x);
  auto bail = [&](const char* what) {
    smalfit_mesh_objective_destroy(m);
    return refused("smalfit_mesh_objective_create", what);
  };
  if (hipMalloc(&m->work, w.bytes) != hipSuccess) return bail("hipMalloc of the work buffers failed");
  if (hipMemset(m->work, 0, w.bytes) != hipSuccess) return bail("hipMemset failed");
  w.point(m->work);
  *out = m;
  return 0;
}

void smalfit_mesh_objective_destroy(smalfit_mesh_objective* m) {
  if (!m) return;
  if (m->tables) (void)hipFree(m->tables);
  if (m->work) (void)hipFree(m->work);
  delete m;
}

int smalfit_mesh_objective_counts(const smalfit_mesh_objective* m, int* num_edges, int* num_face_pairs) {
  if (refused("smalfit_mesh_objective_counts", null_handle_refusal(m != nullptr))) return 1;
  if (num_edges) *num_edges = m->t.E;
  if (num_face_pairs) *num_face_pairs = m->t.P;
  return 0;
}

int smalfit_mesh_objective_eval(smalfit_mesh_objective* m, void* stream, int num_meshes, const float* lbs_verts,
                                const float* trans, const float* deform_verts, const float* points, int num_points,
                                const float* weights /* host [4] */, float* verts_out, float* losses, float* dverts,
                                float* dtrans) {
  return smalfit_mesh_objective_eval_gated(m, stream, num_meshes, lbs_verts, trans, deform_verts, points, num_points, weights, verts_out,
                                           losses, dverts, dtrans, nullptr, nullptr);
}

int smalfit_mesh_objective_eval_gated(smalfit_mesh_objective* m, void* stream, int num_meshes, const float* lbs_verts,
                                      const float* trans, const float* deform_verts, const float* points, int num_points,
                                      const float* weights /* host [4] */, float* verts_out, float* losses, float* dverts,
                                      float* dtrans, smalfit_mesh_targets* t, const smalfit_chamfer_gate_args* g) {
  return smalfit_mesh_objective_eval_robust(m, stream, num_meshes, lbs_verts, trans, deform_verts, points, num_points, weights, verts_out,
                                            losses, dverts, dtrans, t, g, nullptr);
}

int smalfit_mesh_objective_eval_robust(smalfit_mesh_objective* m, void* stream, int num_meshes, const float* lbs_verts,
                                       const float* trans, const float* deform_verts, const float* points, int num_points,
                                       const float* weights /* host [4] */, float* verts_out, float* losses, float* dverts,
                                       float* dtrans, smalfit_mesh_targets* t, const smalfit_chamfer_gate_args* g,
                                       const smalfit_robust_args* rb) {
  const char* who = rb ? "smalfit_mesh_objective_eval_robust" : g ? "smalfit_mesh_objective_eval_gated" : "smalfit_mesh_objective_eval";
  if (refused(who, null_argument_refusal(m && lbs_verts && trans && weights && losses && dverts && dtrans))) return 1;
  if (refused(who, mesh_eval_refusal(num_meshes, m->max_meshes, weights[0], points != nullptr, num_points, m->max_points))) return 1;
  if (g && refused(who, chamfer_gate_args_refusal(g, ChamferGateFacts{weights[0] > 0.f, false, false}))) return 1;
  if (g && t && t->d.N != num_meshes) return refused(who, "number of target meshes differs from num_meshes");
  if (rb && refused(who, robust_args_refusal(rb, RobustFacts{true, false, weights[0] > 0.f, false, false}))) return 1;
  MeshObjectiveRun r;
  r.num_meshes = num_meshes; r.lbs_verts = lbs_verts; r.trans = trans; r.deform_verts = deform_verts;
  r.points = points; r.num_points = num_points; r.weights = weights;
  r.verts_out = verts_out; r.losses = losses; r.dverts = dverts; r.dtrans = dtrans;
  r.gate = g; r.robust = rb;
  if (g) { r.point_normals = g->point_normals; r.point_boundary = g->point_boundary; }
  r.vert_normals = m->surf_vnorm;
  return run_mesh_objective(m, (hipStream_t)stream, r);
}

int smalfit_mesh_targets_create(int num_meshes, const int* vert_counts, const int* face_counts, const float* verts,
                                const int* faces, smalfit_mesh_targets** out) {
  if (refused("smalfit_mesh_targets_create", mesh_targets_create_refusal(vert_counts && face_counts && verts && faces && out, num_meshes,
                                                                         vert_counts, face_counts)))
    return 1;
  std::vector<int> voff(num_meshes + 1, 0), foff(num_meshes + 1, 0);
  for (int n = 0; n < num_meshes; ++n) {
    voff[n + 1] = voff[n] + vert_counts[n];
    foff[n + 1] = foff[n] + face_counts[n];
  }
  std::vector<uint32_t> thr((size_t)foff[num_meshes]);
  try {
    for (int n = 0; n < num_meshes; ++n) {
      const std::vector<uint32_t> t = area_thresholds(vert_counts[n], verts + 3 * (size_t)voff[n], face_counts[n],
                                                      faces + 3 * (size_t)foff[n]);
      std::copy(t.begin(), t.end(), thr.begin() + foff[n]);
    }
  } catch (const std::exception& ex) {
    return refused("smalfit_mesh_targets_create", ex.what());
  }
  // the surface term's vertex -> surface scan reads the targets' triangles every iteration: they never move, so their records
  // are staged here, once
  std::vector<ScanTri> tris((size_t)foff[num_meshes]);
  int max_faces = 0;
  for (int n = 0; n < num_meshes; ++n) {
    max_faces = std::max(max_faces, face_counts[n]);
    const float* base = verts + 3 * (size_t)voff[n];
    for (int f = foff[n]; f < foff[n + 1]; ++f)   // (area_thresholds has checked every index)
      tris[f] = make_scan_tri(base + 3 * (size_t)faces[3 * f], base + 3 * (size_t)faces[3 * f + 1], base + 3 * (size_t)faces[3 * f + 2]);
  }
  // where every target ends, for the boundary rule of the gated term (area_thresholds has checked every index)
  std::vector<uint8_t> bflags((size_t)foff[num_meshes]);
  for (int n = 0; n < num_meshes; ++n) {
    const std::vector<uint8_t> fl = boundary_flags(vert_counts[n], face_counts[n], faces + 3 * (size_t)foff[n]);
    std::copy(fl.begin(), fl.end(), bflags.begin() + foff[n]);
  }
  Blob b;
  const size_t o_vo = b.add(voff.data(), voff.size() * sizeof(int));
  const size_t o_fo = b.add(foff.data(), foff.size() * sizeof(int));
  const size_t o_v = b.add(verts, (size_t)voff[num_meshes] * 3 * sizeof(float));
  const size_t o_f = b.add(faces, (size_t)foff[num_meshes] * 3 * sizeof(int));
  const size_t o_t = b.add(thr.data(), thr.size() * sizeof(uint32_t));
  const size_t o_s = b.add(tris.data(), tris.size() * sizeof(ScanTri));
  const size_t o_b = b.add(bflags.data(), bflags.size());
  unsigned char* base = upload_blob(b, "smalfit_mesh_targets_create");
  if (!base) return 1;
  auto* t = new smalfit_mesh_targets();
  t->blob = base;
  t->d.N = num_meshes;
  t->d.voff = (const int*)(base + o_vo); t->d.foff = (const int*)(base + o_fo);
  t->d.verts = (const float*)(base + o_v); t->d.faces = (const int*)(base + o_f);
  t->d.thr = (const uint32_t*)(base + o_t);
  t->tris = (const ScanTri*)(base + o_s); t->max_faces = max_faces;
  t->bflags = (const unsigned char*)(base + o_b);
  *out = t;
  return 0;
}

void smalfit_mesh_targets_destroy(smalfit_mesh_targets* t) {
  if (!t) return;
  if (t->blob) (void)hipFree(t->blob);
  if (t->index) (void)hipFree(t->index);
  delete t;
}

// ---- the scan index: a grid per target mesh, built on the host ----------------------------------------------------------------
// The handle keeps no host copy of its meshes: the builder reads offsets, vertices and faces back from the device, once per
// build.  The grids, every mesh's CSR and the oversize lists go up as one blob of their own; the handle changes only after all
// of it is in place
int smalfit_mesh_targets_build_index(smalfit_mesh_targets* t, const smalfit_scan_index_args* a) {
  const char* who = "smalfit_mesh_targets_build_index";
  if (refused(who, null_argument_refusal(t && a))) return 1;
  const int N = t->d.N;
  std::vector<int> voff(N + 1), foff(N + 1);
  HIP_OK(hipMemcpy(voff.data(), t->d.voff, voff.size() * sizeof(int), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(foff.data(), t->d.foff, foff.size() * sizeof(int), hipMemcpyDeviceToHost));
  std::vector<float> verts((size_t)voff[N] * 3);
  std::vector<int> faces((size_t)foff[N] * 3);
  HIP_OK(hipMemcpy(verts.data(), t->d.verts, verts.size() * sizeof(float), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(faces.data(), t->d.faces, faces.size() * sizeof(int), hipMemcpyDeviceToHost));
  if (refused(who, scan_index_args_refusal(a, ScanIndexFacts{verts.data(), verts.size()}))) return 1;
  const float scale = a->cell_scale > 0.f ? a->cell_scale : kScanCellScale;
  std::vector<ScanGrid> grids(N);
  std::vector<int> cell_off, cell_face, oversize;
  std::vector<smalfit_scan_index_stats> stats(N);
  for (int n = 0; n < N; ++n) {
    ScanGridHost h;
    if (refused(who, build_scan_grid(verts.data() + 3 * (size_t)voff[n], voff[n + 1] - voff[n], faces.data() + 3 * (size_t)foff[n],
                                     foff[n + 1] - foff[n], scale, h)))
      return 1;
    if (cell_off.size() + h.cell_off.size() > 0x7fffffffull || cell_face.size() + h.cell_face.size() > 0x7fffffffull)
      return refused(who, "scan index needs more than 2^31 - 1 entries");
    h.g.cell_base = (int)cell_off.size();
    h.g.entry_base = (int)cell_face.size();
    h.g.over_base = (int)oversize.size();
    for (int off : h.cell_off) cell_off.push_back(h.g.entry_base + off);
    cell_face.insert(cell_face.end(), h.cell_face.begin(), h.cell_face.end());
    oversize.insert(oversize.end(), h.oversize.begin(), h.oversize.end());
    grids[n] = h.g;
    smalfit_scan_index_stats& s = stats[n];
    s.struct_size = (unsigned)sizeof(s);
    for (int k = 0; k < 3; ++k) s.dims[k] = h.g.dims[k];
    s.cells = h.g.cells; s.occupied_cells = h.occupied; s.entries = (int)h.cell_face.size();
    s.oversize = (int)h.oversize.size(); s.largest_cell = h.largest;
    s.bytes = sizeof(ScanGrid) + (h.cell_off.size() + h.cell_face.size() + h.oversize.size()) * sizeof(int);
  }
  if (cell_face.empty()) cell_face.push_back(0);   // keep every carve non-empty
  if (oversize.empty()) oversize.push_back(0);
  Blob b;
  const size_t o_g = b.add(grids.data(), grids.size() * sizeof(ScanGrid));
  const size_t o_o = b.add(cell_off.data(), cell_off.size() * sizeof(int));
  const size_t o_f = b.add(cell_face.data(), cell_face.size() * sizeof(int));
  const size_t o_v = b.add(oversize.data(), oversize.size() * sizeof(int));
  unsigned char* base = upload_blob(b, who);
  if (!base) return 1;
  if (t->index) {   // a rebuild: nothing may still be walking the old one
    (void)hipDeviceSynchronize();
    (void)hipFree(t->index);
  }
  t->index = base;
  t->ix.grids = (const ScanGrid*)(base + o_g); t->ix.cell_off = (const int*)(base + o_o);
  t->ix.cell_face = (const int*)(base + o_f); t->ix.oversize = (const int*)(base + o_v);
  t->index_stats = std::move(stats);
  return 0;
}

int smalfit_mesh_targets_index_stats(const smalfit_mesh_targets* t, int mesh, smalfit_scan_index_stats* out) {
  const char* who = "smalfit_mesh_targets_index_stats";
  if (refused(who, null_handle_refusal(t != nullptr))) return 1;
  if (refused(who, scan_index_stats_refusal(out, t->index != nullptr, mesh, t->d.N))) return 1;
  *out = t->index_stats[mesh];
  return 0;
}

int smalfit_mesh_targets_sample(smalfit_mesh_targets* t, void* stream, int num_points, unsigned long long seed,
                                unsigned int iteration, float* points) {
  if (refused("smalfit_mesh_targets_sample", mesh_sample_refusal(t && points, num_points))) return 1;
  return launch_mesh_sampler(t, (hipStream_t)stream, num_points, seed, iteration, points);
}

int smalfit_mesh_targets_sample_normals(smalfit_mesh_targets* t, void* stream, int num_points, unsigned long long seed,
                                        unsigned int iteration, float* points, float* normals) {
  if (refused("smalfit_mesh_targets_sample_normals", mesh_sample_refusal(t && points && normals, num_points))) return 1;
  return launch_mesh_sampler(t, (hipStream_t)stream, num_points, seed, iteration, points, normals);
}

int smalfit_mesh_targets_sample_attrs(smalfit_mesh_targets* t, void* stream, int num_points, unsigned long long seed,
                                      unsigned int iteration, float* points, float* normals, unsigned char* boundary) {
  if (refused("smalfit_mesh_targets_sample_attrs", mesh_sample_refusal(t && points, num_points))) return 1;
  return launch_mesh_sampler(t, (hipStream_t)stream, num_points, seed, iteration, points, normals, boundary);
}

// ---- how good a fit is: point-to-surface distances both ways, per mesh -------------------------------------------------
int smalfit_mesh_score(smalfit_mesh_objective* m, smalfit_mesh_targets* t, void* stream, const smalfit_mesh_score_args* a) {
  if (refused("smalfit_mesh_score", null_argument_refusal(m && t && a))) return 1;
  if (refused("smalfit_mesh_score", mesh_score_args_refusal(a, MeshScoreFacts{m->max_meshes, m->max_points, t->d.N}))) return 1;
  hipStream_t st = (hipStream_t)stream;
  MeshScoreArgs k{};
  k.N = a->num_meshes; k.V = m->t.V; k.S = a->points ? a->num_points : 0; k.F = m->num_faces;
  k.verts = a->verts; k.points = a->points; k.faces = m->faces; k.t = t->d;
  k.vert_dist = a->vert_dist ? a->vert_dist : m->vert_dist;
  k.point_dist = a->point_dist ? a->point_dist : m->point_dist;
  k.sums = a->sums; k.within = a->within; k.T = a->num_thresholds;
  for (int i = 0; i < k.T; ++i) k.thr[i] = a->thresholds[i];
  const Grid2 g0 = surface_dist_grid(k.V, k.N);
  if (t->index) {   // the targets carry a scan index: the same distances by the walk over it
    SurfaceGridArgs ga{};
    ga.N = k.N; ga.V = k.V; ga.verts = k.verts; ga.t = k.t; ga.ix = t->ix; ga.vert_dist = k.vert_dist; ga.tau2_v = INFINITY;
    const Grid2 gg = scan_grid_dist_grid(k.V, k.N);
    mesh3d_surface_dist_grid_kernel<<<dim3(gg.x, gg.y), 64 * kScanGridQueries, 0, st>>>(ga);
    LAUNCH_OK("mesh3d_surface_dist_grid_kernel");
  } else {
    mesh3d_surface_dist_kernel<0><<<dim3(g0.x, g0.y), 256, 0, st>>>(k);
    LAUNCH_OK("mesh3d_surface_dist_kernel<0>");
  }
  if (k.S > 0) {
    const Grid2 g1 = surface_dist_grid(k.S, k.N);
    mesh3d_surface_dist_kernel<1><<<dim3(g1.x, g1.y), 256, 0, st>>>(k);
    LAUNCH_OK("mesh3d_surface_dist_kernel<1>");
  }
  const Grid2 gr = score_reduce_grid(k.N);
  mesh3d_score_reduce_kernel<<<dim3(gr.x, gr.y), 256, 0, st>>>(k);
  LAUNCH_OK("mesh3d_score_reduce_kernel");
  return 0;
}

// ---- the surface term alone --------------------------------------------------------------------------------------------
int smalfit_mesh_surface_eval(smalfit_mesh_objective* m, smalfit_mesh_targets* t, void* stream, const smalfit_surface_term_args* a) {
  return smalfit_mesh_surface_eval_gated(m, t, stream, a, nullptr);
}

int smalfit_mesh_surface_eval_gated(smalfit_mesh_objective* m, smalfit_mesh_targets* t, void* stream, const smalfit_surface_term_args* a,
                                    const smalfit_surface_gate_args* g) {
  return smalfit_mesh_surface_eval_robust(m, t, stream, a, g, nullptr);
}

int smalfit_mesh_surface_eval_robust(smalfit_mesh_objective* m, smalfit_mesh_targets* t, void* stream, const smalfit_surface_term_args* a,
                                     const smalfit_surface_gate_args* g, const smalfit_robust_args* rb) {
  const char* who = rb ? "smalfit_mesh_surface_eval_robust" : g ? "smalfit_mesh_surface_eval_gated" : "smalfit_mesh_surface_eval";
  if (refused(who, null_argument_refusal(m && a))) return 1;
  if (refused(who, surface_term_args_refusal(a, SurfaceTermFacts{m->max_meshes, m->max_points, t != nullptr, t ? t->d.N : 0, false, 0, 0,
                                                                 false})))
    return 1;
  if (g && refused(who, surface_gate_args_refusal(g, a, SurfaceGateFacts{t != nullptr, false, false}))) return 1;
  if (rb && refused(who, robust_args_refusal(rb, RobustFacts{false, true, false, a->w_point_surface > 0.f, a->w_vert_surface > 0.f})))
    return 1;
  SurfaceTermRun r;
  r.term = a; r.verts = a->verts; r.points = a->points; r.num_points = a->num_points;
  r.gate = g; r.robust = rb;
  if (g) r.point_normals = g->point_normals;
  return run_surface_term(m, t, (hipStream_t)stream, r);
}

// ---- Stage.step in one call ------------------------------------------------------------------------------------------
int smalfit_fit3d_step(smalfit_engine* e, smalfit_mesh_objective* m, smalfit_mesh_targets* t, void* stream,
                       const smalfit_fit3d_args* a) {
  return smalfit_fit3d_step_surface(e, m, t, stream, a, nullptr);
}

int smalfit_fit3d_step_surface(smalfit_engine* e, smalfit_mesh_objective* m, smalfit_mesh_targets* t, void* stream,
                               const smalfit_fit3d_args* a, const smalfit_surface_term_args* sf) {
  return smalfit_fit3d_step_gated(e, m, t, stream, a, sf, nullptr);
}

int smalfit_fit3d_step_gated(smalfit_engine* e, smalfit_mesh_objective* m, smalfit_mesh_targets* t, void* stream,
                             const smalfit_fit3d_args* a, const smalfit_surface_term_args* sf, const smalfit_surface_gate_args* gate) {
  return smalfit_fit3d_step_partial(e, m, t, stream, a, sf, gate, nullptr);
}

int smalfit_fit3d_step_partial(smalfit_engine* e, smalfit_mesh_objective* m, smalfit_mesh_targets* t, void* stream,
                               const smalfit_fit3d_args* a, const smalfit_surface_term_args* sf, const smalfit_surface_gate_args* gate,
                               const smalfit_chamfer_gate_args* cg) {
  return smalfit_fit3d_step_robust(e, m, t, stream, a, sf, gate, cg, nullptr);
}

int smalfit_fit3d_step_robust(smalfit_engine* e, smalfit_mesh_objective* m, smalfit_mesh_targets* t, void* stream,
                              const smalfit_fit3d_args* a, const smalfit_surface_term_args* sf, const smalfit_surface_gate_args* gate,
                              const smalfit_chamfer_gate_args* cg, const smalfit_robust_args* rb) {
  const char* who = rb ? "smalfit_fit3d_step_robust" : cg ? "smalfit_fit3d_step_partial" : gate ? "smalfit_fit3d_step_gated" : sf ? "smalfit_fit3d_step_surface" : "smalfit_fit3d_step";
  return fit3d_step_run(who, e, m, t, stream, a, sf, gate, cg, rb, nullptr, nullptr);
}

}  // extern "C"

// ---- the scan-sequence block ---------------------------------------------------------------------------------------------
struct smalfit_scan_sequence {
  int N = 0, G = 0, lengths_sum = 0;
  bool any_long = false;       // some clip is longer than 1
  int* tables = nullptr;       // one device allocation: clip_start [G], clip_len [G], mesh_start [N], mesh_len [N]
  // the vertex terms only: the longest clip, the per-block partials (sequence_vertex_partials floats for the largest V seen)
  int longest = 0;
  float* vertex_parts = nullptr;
  size_t vertex_parts_count = 0;
};

// what fit3d_sequence_kernel is given beside the block: the parameters it reads, the gradients it updates (null: not formed), the
// totals step_total is formed from
struct SequenceRun {
  int num_betas = 0;
  const float *global_rot = nullptr, *joint_rot = nullptr, *trans = nullptr;
  float *g_betas = nullptr, *g_theta = nullptr, *g_trans = nullptr;
  bool add_global = false, add_joint = false;       // which column blocks of g_theta
  const float *base_total = nullptr, *surface_total = nullptr;
  const float* vertex_total = nullptr;      // a step with the vertex terms on: their sum and where their step_total goes
  float* vertex_step_total = nullptr;
};
static int launch_sequence(const smalfit_scan_sequence* s, hipStream_t st, const smalfit_sequence_args* q, const SequencePlan& p,
                           const SequenceRun& r) {
  Fit3dSequenceArgs k{};
  k.N = s->N; k.G = s->G; k.nb = r.num_betas;
  k.clip_start = s->tables; k.clip_len = s->tables + s->G; k.mesh_start = s->tables + 2 * s->G; k.mesh_len = s->tables + 2 * s->G + s->N;
  k.global_rot = r.global_rot; k.joint_rot = r.joint_rot; k.trans = r.trans;
  k.g_betas = r.g_betas; k.g_theta = r.g_theta; k.g_trans = r.g_trans;
  k.nshape = p.share && r.g_betas ? sequence_shape_elements(p, s->G, r.num_betas) : 0;
  k.joint = p.joint; k.global = p.global; k.trans_on = p.trans;
  k.add_joint = p.joint && r.g_theta && r.add_joint;
  k.add_global = p.global && r.g_theta && r.add_global;
  k.add_trans = p.trans && r.g_trans;
  k.w_joint = q->w_temp_joint; k.w_global = q->w_temp_global; k.w_trans = q->w_temp_trans;
  k.c_joint = temporal_grad_scale(q->w_temp_joint, kSeqJointLen);
  k.c_global = temporal_grad_scale(q->w_temp_global, kSeqGlobalLen);
  k.c_trans = temporal_grad_scale(q->w_temp_trans, kSeqTransLen);
  k.losses = q->losses;
  k.base_total = r.base_total; k.surface_total = r.surface_total; k.step_total = r.base_total ? q->step_total : nullptr;
  k.vertex_total = r.vertex_total; k.vertex_step_total = r.base_total && r.vertex_total ? r.vertex_step_total : nullptr;
  fit3d_sequence_kernel<<<sequence_blocks(p, s->N, s->G, r.num_betas), kSeqBlock, 0, st>>>(k);
  LAUNCH_OK("fit3d_sequence_kernel");
  return 0;
}

// what the two vertex kernels are given beside the block: the vertices, where t is added or written (null: not formed), the totals
// step_total is formed from
struct SequenceVertexRun {
  int num_verts = 0, Vp = 0;
  const float* verts = nullptr;
  float *acc_dverts = nullptr, *acc_planar = nullptr, *acc_dtrans = nullptr;    // a step: added to
  float *dverts = nullptr, *dtrans = nullptr;                                   // the stand-alone call: written
  const float *base_total = nullptr, *surface_total = nullptr;
  float* step_total = nullptr;      // formed by the finish kernel: only when fit3d_sequence_kernel does not run behind it
};
static int launch_sequence_vertex(smalfit_scan_sequence* s, hipStream_t st, const smalfit_sequence_vertex_args* q,
                                  const SequenceVertexPlan& p, const SequenceVertexRun& r) {
  const int V = r.num_verts;
  const size_t need = sequence_vertex_partials(V, s->N);
  if (need > s->vertex_parts_count) {       // the first call for this V, or V grew
    if (s->vertex_parts) (void)hipFree(s->vertex_parts);
    s->vertex_parts = nullptr; s->vertex_parts_count = 0;
    HIP_OK(hipMalloc((void**)&s->vertex_parts, need * sizeof(float)));
    s->vertex_parts_count = need;
  }
  const Grid2 g = sequence_vertex_grid(V, s->N);
  const int L = sequence_vertex_len(V);
  Fit3dSequenceVertexArgs k{};
  k.N = s->N; k.V = V; k.Vp = r.Vp; k.blocks = g.x;
  k.mesh_start = s->tables + 2 * s->G; k.mesh_len = s->tables + 2 * s->G + s->N;
  k.verts = r.verts;
  k.vel = p.vel; k.acc = p.acc;
  k.w_vel = q->w_temp_vert_vel; k.w_acc = q->w_temp_vert_acc;
  k.c_vel = p.vel ? temporal_grad_scale(q->w_temp_vert_vel, L) : 0.f;
  k.c_acc = p.acc ? temporal_grad_scale(q->w_temp_vert_acc, L) : 0.f;
  k.acc_dverts = r.acc_dverts; k.acc_planar = r.acc_planar; k.dverts = r.dverts;
  k.parts = s->vertex_parts;
  k.acc_dtrans = r.acc_dtrans; k.dtrans = r.dtrans;
  k.losses = q->losses;
  k.base_total = r.base_total; k.surface_total = r.surface_total; k.step_total = r.base_total ? r.step_total : nullptr;
  fit3d_sequence_vertex_kernel<<<dim3(g.x, g.y), kSeqVertexBlock, 0, st>>>(k);
  LAUNCH_OK("fit3d_sequence_vertex_kernel");
  fit3d_sequence_vertex_finish_kernel<<<1, kSeqVertexBlock, 0, st>>>(k);
  LAUNCH_OK("fit3d_sequence_vertex_finish_kernel");
  return 0;
}

// the body of every smalfit_fit3d_step*, of smalfit_scan_sequence_step and of smalfit_scan_sequence_vertex_step.  seq == nullptr
// (the five entry points of before): what they launched and the bits they wrote; vq == nullptr: likewise the sequence step's
static int fit3d_step_run(const char* who, smalfit_engine* e, smalfit_mesh_objective* m, smalfit_mesh_targets* t, void* stream,
                          const smalfit_fit3d_args* a, const smalfit_surface_term_args* sf, const smalfit_surface_gate_args* gate,
                          const smalfit_chamfer_gate_args* cg, const smalfit_robust_args* rb, smalfit_scan_sequence* seq,
                          const smalfit_sequence_args* q, const smalfit_sequence_vertex_args* vq) {
  if (refused(who, null_argument_refusal(e && m && a))) return 1;
  const ModelDev& md = e->model->dev;
  if (refused(who, fit3d_args_refusal(a, Fit3dFacts{e->maxM, md.V, md.NBall, m->max_meshes, m->max_points, m->t.V,
                                                    t != nullptr, t ? t->d.N : 0})))
    return 1;
  if (sf && refused(who, surface_term_args_refusal(sf, SurfaceTermFacts{m->max_meshes, m->max_points, t != nullptr, t ? t->d.N : 0, true,
                                                                        a->num_meshes, a->num_points, a->points != nullptr})))
    return 1;
  if (gate && !sf) return refused(who, "a gate block needs the surface block it gates");
  if (gate && refused(who, surface_gate_args_refusal(gate, sf, SurfaceGateFacts{t != nullptr, true, a->points != nullptr}))) return 1;
  if (cg && refused(who, chamfer_gate_args_refusal(cg, ChamferGateFacts{a->weights[0] > 0.f, true, a->points != nullptr}))) return 1;
  const bool surface = surface_term_on(sf);   // a block with both weights <= 0 is the step without it: nothing of it is launched or written
  if (rb && refused(who, robust_args_refusal(rb, RobustFacts{true, true, a->weights[0] > 0.f, surface && sf->w_point_surface > 0.f,
                                                             surface && sf->w_vert_surface > 0.f})))
    return 1;
  if (seq && refused(who, sequence_args_refusal(q, SequenceFacts{seq->N, seq->lengths_sum, a->num_meshes, true, true, true, true}))) return 1;
  if (vq && refused(who, sequence_vertex_args_refusal(vq, SequenceVertexFacts{true, md.V, true, seq->N, a->num_meshes}))) return 1;
  const Fit3dPlan plan = plan_fit3d(a, md.V, surface && sf->w_point_surface > 0.f);
  const int N = a->num_meshes, nb = a->num_betas, S = a->num_points;
  hipStream_t st = (hipStream_t)stream;
  // the vertex block: with its terms off nothing of it is launched, its losses read 0 and its step_total is the sequence step's
  // (formed where the sequence block's is: through a copy of that block when the caller asked it for none)
  const SequenceVertexPlan vp = vq ? plan_sequence_vertex(vq, seq->longest) : SequenceVertexPlan{};
  const bool vertex_off = vq && !vp.launch;
  const smalfit_sequence_args* q_given = q;
  smalfit_sequence_args q_total;
  if (vertex_off && vq->step_total && !q->step_total) {
    q_total = *q;
    q_total.step_total = vq->step_total;
    q = &q_total;
  }
  // the sequence block: a block that couples nothing launches nothing, its losses read 0 and its step_total is the step's own
  // total (formed by the surface term where that is on: through a copy of its block when the caller asked it for none)
  const SequencePlan sq = seq ? plan_sequence(q, seq->any_long, plan.need_beta) : SequencePlan{};
  smalfit_surface_term_args sf_total;
  if (seq && !sq.launch && q->step_total && surface && !sf->step_total) {
    sf_total = *sf;
    sf_total.step_total = q->step_total;
    sf = &sf_total;
  }
  auto couple_parameters = [&]() -> int {
    if (!seq) return 0;
    if (!sq.launch) {
      HIP_OK(hipMemsetAsync(q->losses, 0, 4 * sizeof(float), st));
      const float* total = surface ? sf->step_total : a->losses + 4;
      if (q->step_total && q->step_total != total) HIP_OK(hipMemcpyAsync(q->step_total, total, sizeof(float), hipMemcpyDeviceToDevice, st));
      return 0;
    }
    SequenceRun r;
    r.num_betas = nb;
    r.global_rot = a->global_rot; r.joint_rot = a->joint_rot; r.trans = a->trans;
    // a gradient joins only where its parameter is trained in this step
    r.g_betas = plan.need_beta ? m->gbetas : nullptr;
    r.add_global = a->lr_global_rot > 0.f; r.add_joint = a->lr_joint_rot > 0.f;
    r.g_theta = r.add_global || r.add_joint ? e->dtheta : nullptr;
    r.g_trans = a->lr_trans > 0.f ? m->dtrans : nullptr;
    r.base_total = a->losses + 4;
    r.surface_total = surface ? sf->losses + 2 : nullptr;
    // (the vertex terms ran before the LBS adjoint: this launch forms their step_total, as the last to know a term)
    if (vp.launch) { r.vertex_total = vq->losses + 2; r.vertex_step_total = vq->step_total; }
    return launch_sequence(seq, st, q, sq, r);
  };
  auto couple = [&]() -> int {
    if (couple_parameters()) return 1;
    // the vertex block's terms are off and the caller asked both blocks for a total: the sequence block's, copied
    if (vertex_off && vq->step_total && q_given->step_total && vq->step_total != q_given->step_total)
      HIP_OK(hipMemcpyAsync(vq->step_total, q_given->step_total, sizeof(float), hipMemcpyDeviceToDevice, st));
    return 0;
  };

  // SMAL3DFitter.forward: LBS on [global_rot | joint_rot] (theta is built inside the head kernel), untranslated
  HeadExtras ex;
  ex.grot = a->global_rot; ex.jrot = a->joint_rot; ex.gmask = e->ones; ex.rmask = e->ones;
  if (run_lbs_forward(e, st, N, a->betas, nb, nb, a->log_beta_scales, 6, e->zeros, nullptr, &ex)) return 1;

  // target points of this iteration, with what plan_fit3d_riders says the gates of both terms share
  const Fit3dRiders riders = plan_fit3d_riders(sf, gate, cg, a->weights[0], plan.points);
  const float* pts = a->points;
  if (plan.points == Fit3dPoints::SampleToCaller || plan.points == Fit3dPoints::SampleToObjective) {
    float* dst = plan.points == Fit3dPoints::SampleToCaller ? a->points_out : m->points;
    if (launch_mesh_sampler(t, st, S, a->seed, a->iteration, dst, riders.draw_normals ? m->surf_pnorm : nullptr,
                            riders.draw_boundary ? m->cham_pbound : nullptr)) return 1;
    pts = dst;
  } else if (plan.points == Fit3dPoints::CallersCopied) {
    HIP_OK(hipMemcpyAsync(a->points_out, a->points, (size_t)N * S * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
  }
  float* vnorm = riders.vert_normals == VertNormalsDest::SurfaceGateBlock ? gate->vert_normals : m->surf_vnorm;

  // Stage.forward and its gradient wrt the vertices
  // (the compose kernel reads the engine's planar vertices in place; the gather kernel leaves a planar copy of the
  // vertex gradient where the LBS adjoint expects it: no layout-conversion launches in between)
  MeshObjectiveRun ob;
  ob.num_meshes = N; ob.lbs_planar = e->verts; ob.Vp = md.Vp; ob.trans = a->trans; ob.deform_verts = a->deform_verts;
  ob.points = pts; ob.num_points = S; ob.weights = a->weights;
  ob.verts_out = a->verts_out; ob.losses = a->losses; ob.dverts = m->dverts; ob.dtrans = m->dtrans;
  ob.dverts_planar = plan.planar_vertex_grad ? e->dext : nullptr;
  ob.gate = cg; ob.robust = rb;
  ob.point_normals = riders.chamfer_normals == RiderSource::Drawn ? m->surf_pnorm : cg ? cg->point_normals : nullptr;
  ob.point_boundary = riders.chamfer_boundary == RiderSource::Drawn ? m->cham_pbound : cg ? cg->point_boundary : nullptr;
  ob.vert_normals = vnorm;
  if (run_mesh_objective(m, st, ob)) return 1;
  // the surface term at the vertices the objective composed; its gradient joins the step's in all three places it is read from
  if (surface) {
    SurfaceTermRun sr;
    sr.term = sf; sr.verts = a->verts_out ? a->verts_out : m->verts; sr.points = pts; sr.num_points = S;
    sr.acc_dverts = m->dverts; sr.acc_planar = ob.dverts_planar; sr.Vp = md.Vp; sr.acc_dtrans = m->dtrans;
    sr.step_losses = a->losses;
    sr.gate = gate; sr.robust = rb;
    sr.point_normals = riders.surface_normals == RiderSource::Drawn ? m->surf_pnorm : gate ? gate->point_normals : nullptr;
    sr.ready_vert_normals = riders.surface_reuses_vert_normals ? vnorm : nullptr;
    if (run_surface_term(m, t, st, sr)) return 1;
  }
  // (a step without the term skips both of its directions: their weight sums read 0)
  if (!surface && rb && rb->surface_weight_sums) HIP_OK(hipMemsetAsync(rb->surface_weight_sums, 0, (size_t)N * 2 * sizeof(float), st));
  // the temporal terms on the vertices the objective composed, behind the surface term's contribution; t joins a destination
  // only where that destination feeds a trained parameter
  if (vertex_off) HIP_OK(hipMemsetAsync(vq->losses, 0, 3 * sizeof(float), st));
  if (vp.launch) {
    SequenceVertexRun vr;
    vr.num_verts = md.V; vr.Vp = md.Vp;
    vr.verts = a->verts_out ? a->verts_out : m->verts;
    vr.acc_planar = ob.dverts_planar;
    vr.acc_dverts = a->lr_deform_verts > 0.f ? m->dverts : nullptr;
    vr.acc_dtrans = a->lr_trans > 0.f ? m->dtrans : nullptr;
    vr.base_total = a->losses + 4;
    vr.surface_total = surface ? sf->losses + 2 : nullptr;
    vr.step_total = sq.launch ? nullptr : vq->step_total;
    if (launch_sequence_vertex(seq, st, vq, vp, vr)) return 1;
  }
  if (!plan.any_trained) return couple();   // (nothing is trained: the blocks only report their losses)

  // back through the LBS (forward state is still in the engine)
  if (plan.need_pose || plan.need_beta) {
    if (run_lbs_backward(e, st, N, nb, 0, nullptr, nullptr, e->dext, true, plan.need_beta, false, nullptr, 105)) return 1;
    if (plan.need_beta && launch_frame_betas_assembly(e, st, N, nb, m->gbetas)) return 1;
  }
  // one shape per clip and the temporal terms' gradients, on the gradients Adam is about to read
  if (couple()) return 1;

  // torch.optim.Adam over the parameters of the scheme, one launch
  struct Tensor { float* p; const float* g; float* mm; float* vv; float lr; };
  const Tensor tr[kFit3dParams] = {{a->betas, m->gbetas, a->m_betas, a->v_betas, a->lr_betas},
                                   {a->global_rot, e->dtheta, a->m_global_rot, a->v_global_rot, a->lr_global_rot},
                                   {a->joint_rot, e->dtheta, a->m_joint_rot, a->v_joint_rot, a->lr_joint_rot},
                                   {a->trans, m->dtrans, a->m_trans, a->v_trans, a->lr_trans},
                                   {a->deform_verts, m->dverts, a->m_deform_verts, a->v_deform_verts, a->lr_deform_verts}};
  Fit3dAdamArgs ad{};
  ad.b1 = a->beta1; ad.b2 = a->beta2; ad.eps = a->eps;
  ad.nseg = plan.nseg;
  for (int s = 0; s < plan.nseg; ++s) {
    const Fit3dAdamGeometry& geo = plan.seg[s];
    const Tensor& x = tr[geo.tensor];
    Fit3dAdamSeg& sg = ad.seg[s];
    sg.p = x.p; sg.g = x.g; sg.m = x.mm; sg.v = x.vv;
    sg.count = geo.count; sg.row_len = geo.row_len; sg.g_stride = geo.g_stride; sg.g_offset = geo.g_offset;
    adam_bias_terms(x.lr, a->beta1, a->beta2, a->adam_t, sg.step_size, ad.bc2_sqrt);   // (bc2_sqrt: the same for every lr)
    sg.block0 = geo.block0;
  }
  fit3d_adam_kernel<<<plan.adam_blocks, 256, 0, st>>>(ad);
  LAUNCH_OK("fit3d_adam_kernel");
  return 0;
}

extern "C" {

int smalfit_scan_sequence_create(int num_meshes, int num_clips, const int* clip_lengths, smalfit_scan_sequence** out) {
  const char* who = "smalfit_scan_sequence_create";
  if (refused(who, sequence_create_refusal(out != nullptr, num_meshes, num_clips, clip_lengths))) return 1;
  auto* s = new smalfit_scan_sequence();
  s->N = num_meshes; s->G = num_clips;
  std::vector<int> host((size_t)2 * num_clips + 2 * num_meshes);
  int start = 0;
  for (int c = 0; c < num_clips; ++c) {
    const int len = clip_lengths[c];
    host[c] = start;
    host[num_clips + c] = len;
    for (int n = start; n < start + len; ++n) {
      host[2 * num_clips + n] = start;
      host[2 * num_clips + num_meshes + n] = len;
    }
    s->any_long = s->any_long || len > 1;
    s->longest = len > s->longest ? len : s->longest;
    start += len;
  }
  s->lengths_sum = start;
  auto bail = [&](const char* what) {
    smalfit_scan_sequence_destroy(s);
    return refused(who, what);
  };
  if (hipMalloc((void**)&s->tables, host.size() * sizeof(int)) != hipSuccess) {
    s->tables = nullptr;
    return bail("hipMalloc of the clip tables failed (no HIP device?)");
  }
  if (hipMemcpy(s->tables, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) return bail("hipMemcpy of the clip tables failed");
  *out = s;
  return 0;
}

void smalfit_scan_sequence_destroy(smalfit_scan_sequence* s) {
  if (!s) return;
  if (s->tables) (void)hipFree(s->tables);
  if (s->vertex_parts) (void)hipFree(s->vertex_parts);
  delete s;
}

int smalfit_scan_sequence_couple(smalfit_scan_sequence* s, void* stream, const smalfit_sequence_args* q, int num_betas,
                                 const float* global_rot, const float* joint_rot, const float* trans, float* g_betas, float* g_theta,
                                 float* g_trans) {
  const char* who = "smalfit_scan_sequence_couple";
  if (refused(who, null_argument_refusal(s && q))) return 1;
  if (refused(who, sequence_args_refusal(q, SequenceFacts{s->N, s->lengths_sum, s->N, false, global_rot != nullptr, joint_rot != nullptr,
                                                          trans != nullptr})))
    return 1;
  if (g_betas && q->share_shape && (num_betas <= 0 || num_betas > 64)) return refused(who, "num_betas out of range");
  hipStream_t st = (hipStream_t)stream;
  const SequencePlan p = plan_sequence(q, s->any_long, g_betas != nullptr);
  if (!p.launch) {
    HIP_OK(hipMemsetAsync(q->losses, 0, 4 * sizeof(float), st));
    return 0;
  }
  SequenceRun r;
  r.num_betas = num_betas;
  r.global_rot = global_rot; r.joint_rot = joint_rot; r.trans = trans;
  r.g_betas = g_betas; r.g_theta = g_theta; r.g_trans = g_trans;
  r.add_global = r.add_joint = g_theta != nullptr;
  return launch_sequence(s, st, q, p, r);
}

int smalfit_scan_sequence_step(smalfit_scan_sequence* s, smalfit_engine* e, smalfit_mesh_objective* m, smalfit_mesh_targets* t,
                               void* stream, const smalfit_fit3d_args* a, const smalfit_surface_term_args* sf,
                               const smalfit_surface_gate_args* gate, const smalfit_chamfer_gate_args* cg, const smalfit_robust_args* rb,
                               const smalfit_sequence_args* q) {
  const char* who = "smalfit_scan_sequence_step";
  if (refused(who, null_argument_refusal(s && q))) return 1;
  return fit3d_step_run(who, e, m, t, stream, a, sf, gate, cg, rb, s, q);
}

int smalfit_scan_sequence_vertex_term(smalfit_scan_sequence* s, void* stream, const smalfit_sequence_vertex_args* q, int num_verts,
                                      const float* verts, float* dverts, float* dtrans) {
  const char* who = "smalfit_scan_sequence_vertex_term";
  if (refused(who, null_argument_refusal(s != nullptr))) return 1;
  if (refused(who, sequence_vertex_args_refusal(q, SequenceVertexFacts{false, num_verts, verts != nullptr, s->N, s->N}))) return 1;
  hipStream_t st = (hipStream_t)stream;
  const SequenceVertexPlan p = plan_sequence_vertex(q, s->longest);
  if (!p.launch) {     // nothing is launched: the losses and the gradients the caller gave read 0
    HIP_OK(hipMemsetAsync(q->losses, 0, 3 * sizeof(float), st));
    if (dverts) HIP_OK(hipMemsetAsync(dverts, 0, (size_t)s->N * num_verts * 3 * sizeof(float), st));
    if (dtrans) HIP_OK(hipMemsetAsync(dtrans, 0, (size_t)s->N * 3 * sizeof(float), st));
    return 0;
  }
  SequenceVertexRun r;
  r.num_verts = num_verts;
  r.verts = verts; r.dverts = dverts; r.dtrans = dtrans;
  return launch_sequence_vertex(s, st, q, p, r);
}

int smalfit_scan_sequence_vertex_step(smalfit_scan_sequence* s, smalfit_engine* e, smalfit_mesh_objective* m, smalfit_mesh_targets* t,
                                      void* stream, const smalfit_fit3d_args* a, const smalfit_surface_term_args* sf,
                                      const smalfit_surface_gate_args* gate, const smalfit_chamfer_gate_args* cg,
                                      const smalfit_robust_args* rb, const smalfit_sequence_args* q,
                                      const smalfit_sequence_vertex_args* vq) {
  const char* who = "smalfit_scan_sequence_vertex_step";
  if (refused(who, null_argument_refusal(s && q))) return 1;
  if (!vq && refused(who, sequence_vertex_args_refusal(nullptr, SequenceVertexFacts{}))) return 1;
  return fit3d_step_run(who, e, m, t, stream, a, sf, gate, cg, rb, s, q, vq);
}

}  // extern "C"
