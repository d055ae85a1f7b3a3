// Host side of the 3D mesh-fitting objective (SURVEY.md §8f row 3): topology upload, target meshes + sampler,
// kernel sequencing, C-ABI.  Included at the end of smalfit_kernels.hip after smalfit_launch.inc.
#include "mesh3d_topology.h"

static_assert(kMeshQueries == kChamQueries && kMeshThreads == kMeshBlock, "smalfit_plan.h sizes the grids of the mesh3d kernels");

struct smalfit_mesh_objective {
  Mesh3dTables t{};
  void* tables = nullptr;     // one allocation behind t.*
  void* work = nullptr;       // one allocation behind the work buffers below
  int max_meshes = 0, max_points = 0;
  int bx = 0, by = 0, bv = 0, bp = 0;
  float* verts = nullptr;
  int* nn_idx = nullptr;
  float *gcham = nullptr, *gedge = nullptr, *lap_unit = nullptr, *gpair = nullptr;
  float *part_cx = nullptr, *part_cy = nullptr, *part_edge = nullptr, *part_lap = nullptr, *part_normal = nullptr,
        *part_dtr = nullptr;
  // smalfit_fit3d_step only: sampled points, gradients handed to Adam
  float *points = nullptr, *dverts = nullptr, *dtrans = nullptr, *gbetas = nullptr;
};

struct smalfit_mesh_targets {
  MeshTargetsDev d{};
  void* blob = nullptr;
};

// the 6 launches of one evaluation; arguments validated by the callers
static int run_mesh_objective(smalfit_mesh_objective* m, hipStream_t st, int num_meshes, const float* lbs_verts,
                              const float* trans, const float* deform_verts, const float* points, int num_points,
                              const float* weights, float* verts_out, float* losses, float* dverts, float* dtrans,
                              const float* lbs_planar = nullptr, int Vp = 0, float* dverts_planar = nullptr) {
  const float wc = mesh_weight(weights[0]);
  Mesh3dArgs a{};
  a.N = num_meshes; a.V = m->t.V; a.S = mesh_points(wc, num_points);
  a.t = m->t;
  a.lbs_verts = lbs_verts; a.lbs_planar = lbs_planar; a.Vp = Vp; a.dverts_planar = dverts_planar;
  a.trans = trans; a.deform = deform_verts;
  a.verts = verts_out ? verts_out : m->verts;
  a.points = points; a.nn_idx = m->nn_idx;
  a.gcham = m->gcham; a.gedge = m->gedge; a.lap_unit = m->lap_unit; a.gpair = m->gpair;
  a.dverts = dverts; a.dtrans = dtrans; a.losses = losses;
  a.w_chamfer = wc; a.w_edge = mesh_weight(weights[1]); a.w_normal = mesh_weight(weights[2]);
  a.w_laplacian = mesh_weight(weights[3]);
  a.part_cx = m->part_cx; a.part_cy = m->part_cy; a.part_edge = m->part_edge; a.part_lap = m->part_lap;
  a.part_normal = m->part_normal; a.part_dtr = m->part_dtr;
  a.bx = mesh_query_blocks(a.S); a.by = m->by; a.bv = m->bv; a.bp = m->bp;
  const size_t total = (size_t)a.N * a.V * 3;
  mesh3d_compose_kernel<<<dim3((unsigned)((total + 255) / 256)), 256, 0, st>>>(a);
  LAUNCH_OK("mesh3d_compose_kernel");
  if (wc > 0.f) {
    mesh3d_chamfer_kernel<0><<<dim3(a.bx, a.N), 256, 0, st>>>(a);
    LAUNCH_OK("mesh3d_chamfer_kernel<0>");
    mesh3d_chamfer_kernel<1><<<dim3(a.by, a.N), 256, 0, st>>>(a);
    LAUNCH_OK("mesh3d_chamfer_kernel<1>");
  } else {
    HIP_OK(hipMemsetAsync(m->gcham, 0, total * sizeof(float), st));
  }
  mesh3d_ring_kernel<<<dim3(a.bv + a.bp, a.N), kMeshBlock, 0, st>>>(a);
  LAUNCH_OK("mesh3d_ring_kernel");
  mesh3d_gather_kernel<<<dim3(a.bv, a.N), kMeshBlock, 0, st>>>(a);
  LAUNCH_OK("mesh3d_gather_kernel");
  mesh3d_reduce_kernel<<<1, 256, 0, st>>>(a);
  LAUNCH_OK("mesh3d_reduce_kernel");
  return 0;
}

extern "C" {

int smalfit_mesh_objective_create(int num_verts, int num_faces, const int* faces, int max_meshes, int max_points,
                                  smalfit_mesh_objective** out) {
  if (!faces || !out) return fail("smalfit_mesh_objective_create: null argument");
  if (max_meshes <= 0 || max_points <= 0) return fail("smalfit_mesh_objective_create: max_meshes and max_points must be positive");
  MeshTopologyHost h;
  try {
    h = build_mesh_topology(num_verts, num_faces, faces);
  } catch (const std::exception& ex) {
    return fail(std::string("smalfit_mesh_objective_create: ") + ex.what());
  }
  Blob b;
  if (h.pairs.empty()) h.pairs.assign(4, 0);   // keep the carve non-empty; P stays 0
  if (h.inc.empty()) h.inc.assign(1, 0);
  const size_t o_no = b.add(h.nbr_off.data(), h.nbr_off.size() * sizeof(int));
  const size_t o_nb = b.add(h.nbr.data(), h.nbr.size() * sizeof(int));
  const size_t o_pr = b.add(h.pairs.data(), h.pairs.size() * sizeof(int));
  const size_t o_io = b.add(h.inc_off.data(), h.inc_off.size() * sizeof(int));
  const size_t o_in = b.add(h.inc.data(), h.inc.size() * sizeof(int));
  auto* m = new smalfit_mesh_objective();
  auto bail = [&](const char* what) {
    if (m->tables) (void)hipFree(m->tables);
    if (m->work) (void)hipFree(m->work);
    delete m;
    return fail(std::string("smalfit_mesh_objective_create: ") + what);
  };
  if (hipMalloc(&m->tables, b.bytes.size()) != hipSuccess) return bail("hipMalloc failed (no HIP device?)");
  if (hipMemcpy(m->tables, b.bytes.data(), b.bytes.size(), hipMemcpyHostToDevice) != hipSuccess) return bail("hipMemcpy failed");
  unsigned char* base = (unsigned char*)m->tables;
  m->t.V = h.V; m->t.E = h.E; m->t.P = h.P;
  m->t.nbr_off = (const int*)(base + o_no); m->t.nbr = (const int*)(base + o_nb);
  m->t.pairs = (const int*)(base + o_pr);
  m->t.inc_off = (const int*)(base + o_io); m->t.inc = (const int*)(base + o_in);
  m->max_meshes = max_meshes; m->max_points = max_points;
  const int N = max_meshes, V = h.V, P = std::max(h.P, 1);
  const MeshGrids grids = mesh_grids(max_points, V, h.P);   // (bx: the capacity; an evaluation's own follows its num_points)
  m->bx = grids.bx; m->by = grids.by; m->bv = grids.bv; m->bp = grids.bp;
  size_t bytes = 0;
  auto carve = [&](size_t n) { const size_t o = align_up(bytes, 256); bytes = o + n; return o; };
  const size_t nv3 = (size_t)N * V * 3 * sizeof(float);
  const size_t w_verts = carve(nv3), w_nn = carve((size_t)N * max_points * sizeof(int)), w_gc = carve(nv3),
               w_ge = carve(nv3), w_lu = carve(nv3), w_gp = carve((size_t)N * P * 12 * sizeof(float)),
               w_cx = carve((size_t)N * m->bx * sizeof(float)), w_cy = carve((size_t)N * m->by * sizeof(float)),
               w_pe = carve((size_t)N * m->bv * sizeof(float)), w_pl = carve((size_t)N * m->bv * sizeof(float)),
               w_pn = carve((size_t)N * std::max(m->bp, 1) * sizeof(float)),
               w_pd = carve((size_t)N * m->bv * 3 * sizeof(float)),
               w_pt = carve((size_t)N * max_points * 3 * sizeof(float)), w_dv = carve(nv3),
               w_dt = carve((size_t)N * 3 * sizeof(float)), w_gb = carve((size_t)N * 64 * sizeof(float));
  if (hipMalloc(&m->work, bytes) != hipSuccess) return bail("hipMalloc of the work buffers failed");
  if (hipMemset(m->work, 0, bytes) != hipSuccess) return bail("hipMemset failed");
  unsigned char* wb = (unsigned char*)m->work;
  m->verts = (float*)(wb + w_verts); m->nn_idx = (int*)(wb + w_nn); m->gcham = (float*)(wb + w_gc);
  m->gedge = (float*)(wb + w_ge); m->lap_unit = (float*)(wb + w_lu); m->gpair = (float*)(wb + w_gp);
  m->part_cx = (float*)(wb + w_cx); m->part_cy = (float*)(wb + w_cy); m->part_edge = (float*)(wb + w_pe);
  m->part_lap = (float*)(wb + w_pl); m->part_normal = (float*)(wb + w_pn); m->part_dtr = (float*)(wb + w_pd);
  m->points = (float*)(wb + w_pt); m->dverts = (float*)(wb + w_dv);
  m->dtrans = (float*)(wb + w_dt); m->gbetas = (float*)(wb + w_gb);
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
  if (!m) return fail("smalfit_mesh_objective_counts: null handle");
  if (num_edges) *num_edges = m->t.E;
  if (num_face_pairs) *num_face_pairs = m->t.P;
  return 0;
}

int smalfit_mesh_objective_eval(smalfit_mesh_objective* m, void* stream, int num_meshes, const float* lbs_verts,
                                const float* trans, const float* deform_verts, const float* points, int num_points,
                                const float* weights /* host [4] */, float* verts_out, float* losses, float* dverts,
                                float* dtrans) {
  if (!m || !lbs_verts || !trans || !weights || !losses || !dverts || !dtrans)
    return fail("smalfit_mesh_objective_eval: null argument");
  if (num_meshes <= 0 || num_meshes > m->max_meshes) return fail("smalfit_mesh_objective_eval: num_meshes out of range");
  if (weights[0] > 0.f && (!points || num_points <= 0 || num_points > m->max_points))
    return fail("smalfit_mesh_objective_eval: the chamfer term needs 1 <= num_points <= max_points target points");
  return run_mesh_objective(m, (hipStream_t)stream, num_meshes, lbs_verts, trans, deform_verts, points, num_points, weights,
                            verts_out, losses, dverts, dtrans);
}

int smalfit_mesh_targets_create(int num_meshes, const int* vert_counts, const int* face_counts, const float* verts,
                                const int* faces, smalfit_mesh_targets** out) {
  if (!vert_counts || !face_counts || !verts || !faces || !out) return fail("smalfit_mesh_targets_create: null argument");
  if (num_meshes <= 0) return fail("smalfit_mesh_targets_create: no meshes");
  std::vector<int> voff(num_meshes + 1, 0), foff(num_meshes + 1, 0);
  for (int n = 0; n < num_meshes; ++n) {
    if (vert_counts[n] <= 0 || face_counts[n] <= 0) return fail("smalfit_mesh_targets_create: empty target mesh");
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
    return fail(std::string("smalfit_mesh_targets_create: ") + ex.what());
  }
  Blob b;
  const size_t o_vo = b.add(voff.data(), voff.size() * sizeof(int));
  const size_t o_fo = b.add(foff.data(), foff.size() * sizeof(int));
  const size_t o_v = b.add(verts, (size_t)voff[num_meshes] * 3 * sizeof(float));
  const size_t o_f = b.add(faces, (size_t)foff[num_meshes] * 3 * sizeof(int));
  const size_t o_t = b.add(thr.data(), thr.size() * sizeof(uint32_t));
  auto* t = new smalfit_mesh_targets();
  if (hipMalloc(&t->blob, b.bytes.size()) != hipSuccess) { delete t; return fail("smalfit_mesh_targets_create: hipMalloc failed (no HIP device?)"); }
  if (hipMemcpy(t->blob, b.bytes.data(), b.bytes.size(), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(t->blob); delete t; return fail("smalfit_mesh_targets_create: hipMemcpy failed");
  }
  unsigned char* base = (unsigned char*)t->blob;
  t->d.N = num_meshes;
  t->d.voff = (const int*)(base + o_vo); t->d.foff = (const int*)(base + o_fo);
  t->d.verts = (const float*)(base + o_v); t->d.faces = (const int*)(base + o_f);
  t->d.thr = (const uint32_t*)(base + o_t);
  *out = t;
  return 0;
}

void smalfit_mesh_targets_destroy(smalfit_mesh_targets* t) {
  if (!t) return;
  if (t->blob) (void)hipFree(t->blob);
  delete t;
}

int smalfit_mesh_targets_sample(smalfit_mesh_targets* t, void* stream, int num_points, unsigned long long seed,
                                unsigned int iteration, float* points) {
  if (!t || !points) return fail("smalfit_mesh_targets_sample: null argument");
  if (num_points <= 0) return fail("smalfit_mesh_targets_sample: num_points must be positive");
  mesh3d_sample_kernel<<<dim3((num_points + 255) / 256, t->d.N), 256, 0, (hipStream_t)stream>>>(
      t->d, num_points, (uint32_t)(seed & 0xFFFFFFFFull), (uint32_t)(seed >> 32), iteration, points);
  LAUNCH_OK("mesh3d_sample_kernel");
  return 0;
}

// ---- Stage.step in one call ------------------------------------------------------------------------------------------
int smalfit_fit3d_step(smalfit_engine* e, smalfit_mesh_objective* m, smalfit_mesh_targets* t, void* stream,
                       const smalfit_fit3d_args* a) {
  if (!e || !m || !a) return fail("smalfit_fit3d_step: null argument");
  const int N = a->num_meshes, nb = a->num_betas, S = a->num_points;
  const ModelDev& md = e->model->dev;
  if (N <= 0 || N > e->maxM || N > m->max_meshes) return fail("smalfit_fit3d_step: num_meshes exceeds the engine's max_frames or the objective's max_meshes");
  if (md.V != m->t.V) return fail("smalfit_fit3d_step: engine and objective were built for different meshes");
  if (nb <= 0 || nb > md.NBall || nb > 64) return fail("smalfit_fit3d_step: num_betas out of range");
  if (!a->betas || !a->global_rot || !a->joint_rot || !a->trans || !a->losses) return fail("smalfit_fit3d_step: missing parameter / losses pointer");
  const bool chamfer = a->weights[0] > 0.f;
  if (chamfer) {
    if (S <= 0 || S > m->max_points) return fail("smalfit_fit3d_step: the chamfer term needs 1 <= num_points <= max_points");
    if (!a->points && !t) return fail("smalfit_fit3d_step: neither target points nor target meshes given");
    if (!a->points && t->d.N != N) return fail("smalfit_fit3d_step: number of target meshes differs from num_meshes");
  }
  struct Trained { float* p; float* mm; float* vv; float lr; const char* name; };
  const Trained tr[kFit3dParams] = {{a->betas, a->m_betas, a->v_betas, a->lr_betas, "betas"},
                                    {a->global_rot, a->m_global_rot, a->v_global_rot, a->lr_global_rot, "global_rot"},
                                    {a->joint_rot, a->m_joint_rot, a->v_joint_rot, a->lr_joint_rot, "joint_rot"},
                                    {a->trans, a->m_trans, a->v_trans, a->lr_trans, "trans"},
                                    {a->deform_verts, a->m_deform_verts, a->v_deform_verts, a->lr_deform_verts, "deform_verts"}};
  bool any = false;
  for (const Trained& x : tr)
    if (x.lr > 0.f) {
      if (!x.p || !x.mm || !x.vv) return fail(std::string("smalfit_fit3d_step: ") + x.name + " is trained (lr > 0) but its parameter or Adam state is missing");
      any = true;
    }
  if (any && a->adam_t <= 0) return fail("smalfit_fit3d_step: adam_t must be the 1-based step count");
  hipStream_t st = (hipStream_t)stream;

  // SMAL3DFitter.forward: LBS on [global_rot | joint_rot] (theta is built inside the head kernel), untranslated
  HeadExtras ex;
  ex.grot = a->global_rot; ex.jrot = a->joint_rot; ex.gmask = e->ones; ex.rmask = e->ones;
  if (run_lbs_forward(e, st, N, a->betas, nb, nb, a->log_beta_scales, 6, e->zeros, nullptr, &ex)) return 1;

  // target points of this iteration
  const float* pts = a->points;
  if (chamfer && !pts) {
    float* dst = a->points_out ? a->points_out : m->points;
    mesh3d_sample_kernel<<<dim3((S + 255) / 256, N), 256, 0, st>>>(t->d, S, (uint32_t)(a->seed & 0xFFFFFFFFull),
                                                                  (uint32_t)(a->seed >> 32), a->iteration, dst);
    LAUNCH_OK("mesh3d_sample_kernel");
    pts = dst;
  } else if (chamfer && a->points_out && a->points_out != a->points) {
    HIP_OK(hipMemcpyAsync(a->points_out, a->points, (size_t)N * S * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
  }

  // Stage.forward and its gradient wrt the vertices
  // (the compose kernel reads the engine's planar vertices in place; the gather kernel leaves a planar copy of the
  // vertex gradient where the LBS adjoint expects it: no layout-conversion launches in between)
  const bool need_pose = a->lr_global_rot > 0.f || a->lr_joint_rot > 0.f, need_beta = a->lr_betas > 0.f;
  if (run_mesh_objective(m, st, N, nullptr, a->trans, a->deform_verts, pts, S, a->weights, a->verts_out, a->losses,
                         m->dverts, m->dtrans, e->verts, md.Vp, (need_pose || need_beta) ? e->dext : nullptr)) return 1;
  if (!any) return 0;

  // back through the LBS (forward state is still in the engine)
  if (need_pose || need_beta) {
    if (run_lbs_backward(e, st, N, nb, 0, nullptr, nullptr, e->dext, true, need_beta, false, nullptr, 105)) return 1;
    if (need_beta) {
      AssembleArgs g;
      std::memset(&g, 0, sizeof(g));
      g.M = N; g.nb = nb; g.NBall = md.NBall; g.nblk_beta = e->nblk_beta; g.betas_shared = 0;
      g.dbeta_part = e->dbeta_part; g.dJrest = e->dJrest; g.JS = md.JS; g.dbetaJ = e->dbetaJ; g.ngrp_beta = 1; g.g_betas = m->gbetas;
      g.win = WinMap{1, 0, N};
      assemble_kernel<false><<<N, 256, 0, st>>>(g, AssembleExt{});
      LAUNCH_OK("assemble_kernel");
    }
  }

  // torch.optim.Adam over the parameters of the scheme, one launch
  Fit3dAdamArgs ad{};
  ad.b1 = a->beta1; ad.b2 = a->beta2; ad.eps = a->eps;
  const float* grads[kFit3dParams] = {m->gbetas, e->dtheta, e->dtheta, m->dtrans, m->dverts};
  const int counts[kFit3dParams] = {N * nb, N * 3, N * 102, N * 3, N * md.V * 3};
  const int row_len[kFit3dParams] = {nb, 3, 102, 3, md.V * 3};
  const int g_stride[kFit3dParams] = {nb, 105, 105, 3, md.V * 3};
  const int g_offset[kFit3dParams] = {0, 0, 3, 0, 0};
  int blocks = 0;
  for (int k = 0; k < kFit3dParams; ++k) {
    if (!(tr[k].lr > 0.f)) continue;
    Fit3dAdamSeg& sg = ad.seg[ad.nseg++];
    sg.p = tr[k].p; sg.g = grads[k]; sg.m = tr[k].mm; sg.v = tr[k].vv;
    sg.count = counts[k]; sg.row_len = row_len[k]; sg.g_stride = g_stride[k]; sg.g_offset = g_offset[k];
    adam_bias_terms(tr[k].lr, a->beta1, a->beta2, a->adam_t, sg.step_size, ad.bc2_sqrt);   // (bc2_sqrt: the same for every lr)
    sg.block0 = blocks;
    blocks += (counts[k] + 255) / 256;
  }
  fit3d_adam_kernel<<<blocks, 256, 0, st>>>(ad);
  LAUNCH_OK("fit3d_adam_kernel");
  return 0;
}

}  // extern "C"
