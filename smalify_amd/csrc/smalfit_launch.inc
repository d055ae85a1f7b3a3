// Host side of libsmalfit.so: model upload, workspace carving, kernel sequencing, C-ABI.
// Included at the end of smalfit_kernels.hip (same translation unit as the kernels).  Every choice between launches (plan_eval
// for an evaluation), every grid that depends on the problem's size and every refusal of an argument is a function of
// smalfit_plan.h, and the tables of a model are built by smal_model_pack.h; here are the pointers, the allocations, the copies and
// the launches.  (Errors of the runtime -- allocations, copies, launches -- are worded here.)
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/smalfit.h"
#include "smalfit_plan.h"
#include "smal_model_pack.h"

namespace smalfit {

static thread_local std::string g_err;
static_assert(kHeadPriorFrames == kPriorFrames, "smalfit_plan.h counts the prior blocks of lbs_head_images_kernel");
#ifdef SMALFIT_DEV_PROBES
static int g_dbg = 0;             // developer builds only (tools/build_variant.sh ... -DSMALFIT_DEV_PROBES): smalfit_debug_set
#else
static constexpr int g_dbg = 0;   // the product has no run-time switches: probes and statistics are compiled out
#endif

static int fail(const std::string& msg) {
  g_err = msg;
  return 1;
}
// a refusal of smalfit_plan.h (nullptr: none) under the name of the entry point that met it
static int refused(const char* who, const char* why) { return why ? fail(std::string(who) + ": " + why) : 0; }

#define HIP_OK(expr)                                                                         \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess)                                                                    \
      return fail(std::string(#expr) + ": " + hipGetErrorString(_e));                        \
  } while (0)

#define LAUNCH_OK(what)                                                                      \
  do {                                                                                       \
    hipError_t _e = hipGetLastError();                                                       \
    if (_e != hipSuccess) return fail(std::string("launch ") + what + ": " + hipGetErrorString(_e)); \
  } while (0)

// one device allocation holding `b` -> its base, or nullptr with the runtime's error worded under the entry point's name
static unsigned char* upload_blob(const Blob& b, const char* who) {
  void* dev = nullptr;
  if (hipMalloc(&dev, b.bytes.size()) != hipSuccess) { fail(std::string(who) + ": hipMalloc failed (no HIP device?)"); return nullptr; }
  if (hipMemcpy(dev, b.bytes.data(), b.bytes.size(), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(dev);
    fail(std::string(who) + ": hipMemcpy failed");
    return nullptr;
  }
  return (unsigned char*)dev;
}

// a workspace of many buffers in one device allocation: list the fields (each starts at a multiple of 256 bytes), allocate
// `bytes` (the end of the last field) or more, point() the fields into the slab
struct Carver {
  struct Item { void** ptr; size_t off; };
  std::vector<Item> items;
  size_t bytes = 0;
  template <class T>
  void field(T*& ptr, size_t count) {
    const size_t off = align_up(bytes, 256);
    items.push_back({(void**)&ptr, off});
    bytes = off + count * sizeof(T);
  }
  void point(void* slab) const {
    for (const Item& it : items) *it.ptr = (unsigned char*)slab + it.off;
  }
};

static const int kCanonical[25] = {10, 9, 8, 20, 19, 18, 14, 13, 12, 24, 23, 22, 25,   // config.py:77-88
                                   31, 33, 34, 35, 36, 38, 37, 39, 40, 15, 15, 28};

}  // namespace smalfit

using namespace smalfit;

struct smalfit_model {
  ModelDev dev;
  void* blob = nullptr;
  int V = 0, Vp = 0, F = 0, NBall = 0;
};

struct smalfit_engine {
  smalfit_model* model = nullptr;
  int maxM = 0, Mp = 0, S = 0, Tx = 0, T = 0, cap = 0, CS = PBM_SPLITS, nvt = 0, nblk_beta = 0;
  void* slab = nullptr;
  // forward state
  float *theta, *v_shaped, *Jrest, *Rm, *Gm, *scm, *Am, *pfT, *vposed, *verts, *proj, *joints;
  // raster
  int2* fbox;
  int* status;
  float4* frec;
  int4* brect;
  unsigned long long* gacc;
  unsigned* bcnt;
  float2* zband;      // persistent per-pixel depth bounds (lo, hi) of the last exact selection
  float2* blist;      // separate allocation: [M][S*S][kBandCap]
  unsigned char* plist;   // per-face candidate lists of the forward sweep, read by the backward gather: [M][F][kListCap]
  unsigned char* pcount;  // their lengths (kNoList: evaluate the whole box): [M][F]
  unsigned long long* zbuf = nullptr;   // colour render only, allocated on first use: [M][S*S]
  float* vnorm = nullptr;               // colour render only: vertex normals [M][3][Vp]
  unsigned char* cover = nullptr;       // smalfit_fit_metrics only, allocated on first use: hard coverage, a byte per pixel [M][S*S]
  int *qcount, *frect, *queue, *bqueue;
  long long* qloss;
  int nrb = 0;
  float2* gz;
  float* zc;          // per-frame reference depth of the rasteriser
  float* lpart;
  long long* qpart;
  int* asm_counter;
  float* shstate;     // shared parameters between the iterations of smalfit_fit_run: [2 slots][value, exp_avg, exp_avg_sq][32: betas 20 | limb scales 6]
  float *silbuf, *tile_loss, *dface;
  // adjoints
  float *dJ41, *dvert, *dvp, *dext, *dA, *dpf_part, *dbeta_part, *dtheta, *dls, *dJrest;
  float* dbetaJ;
  float *dth_direct, *dtr_direct, *dtr_part, *loss_part, *loss_betas, *gb_prior, *gls_prior;
  float *win_gb, *win_gls;                             // smalfit_fit_eval_windows: the rows before they are added up, [maxM][kWindowRowBetas], [maxM][kWindowRowScales]
  float *loss_betas_pf, *gb_prior_pf, *gls_prior_pf;   // independent images: the prior per frame, [maxM], [maxM][kPriorSlotB], [maxM][kPriorSlotLs]
  unsigned long long* frame_qloss;                     // the queue kernels' loss per frame: [maxM][kFrameLossStride], zero between evaluations
  float *ones, *zeros;
  int* canon;
  // priors
  float *pose_prec = nullptr, *pose_mean = nullptr, *pose_mask = nullptr;
  float *lim_min = nullptr, *lim_max = nullptr;      // joint limits (34,3) each
  bool has_joint_limits = false;
  float *shape_prec = nullptr, *shape_mean = nullptr;
  int shape_dim = 0;
  bool has_pose_prior = false;
  bool unclamped_edge_t = false;          // SMALFIT_OPT_UNCLAMPED_EDGE_T
  // optional replay of one captured iteration (smalfit_engine_set_graph)
  bool use_graph = false;
  hipGraphExec_t graph_exec = nullptr;
  std::vector<unsigned char> graph_key;   // bytes of the (fit args, adam args sans step, stream, config epoch) the graph was captured for
  unsigned config_epoch = 0;              // bumped by every setter whose state is baked into captured launches (priors, limits)
  int* step_counter = nullptr;            // device: Adam step count read by the captured Adam node
  // optional per-section HIP-event timing (smalfit_engine_profile_*)
  bool prof_on = false;
  int prof_iter = 0, prof_cap = 0, prof_stride = 1, prof_tick = 0;
  std::vector<hipEvent_t> prof_ev;     // [prof_cap][SMALFIT_NUM_SECTIONS][2]
};

namespace smalfit {
struct Section {
  smalfit_engine* e; hipStream_t st; int id; bool on;
  Section(smalfit_engine* e_, hipStream_t st_, int id_) : e(e_), st(st_), id(id_) {
    on = e->prof_on && e->prof_iter < e->prof_cap && (e->prof_tick % e->prof_stride) == 0;
    if (on) (void)hipEventRecord(e->prof_ev[((size_t)e->prof_iter * SMALFIT_NUM_SECTIONS + id) * 2], st);
  }
  ~Section() {
    if (on) (void)hipEventRecord(e->prof_ev[((size_t)e->prof_iter * SMALFIT_NUM_SECTIONS + id) * 2 + 1], st);
  }
};
}  // namespace smalfit

namespace smalfit {
// the backward gather in the variant the engine's options select
static void launch_raster_bwd(smalfit_engine* e, hipStream_t st, int M) {
  const ModelDev& m = e->model->dev;
  const unsigned grid = (unsigned)raster_bwd_grid(m.F, M), block = kBwdLanes * kBwdFaces;
  const float inv_s = raster_bwd_inv_s(e->S);
  if (e->unclamped_edge_t)
    raster_bwd_kernel<true><<<grid, block, 0, st>>>(m.F, M, e->S, inv_s, e->frec, e->fbox, e->zc, e->gz, e->plist, e->pcount, e->dface);
  else
    raster_bwd_kernel<false><<<grid, block, 0, st>>>(m.F, M, e->S, inv_s, e->frec, e->fbox, e->zc, e->gz, e->plist, e->pcount, e->dface);
}
}  // namespace smalfit

extern "C" {

int smalfit_version(void) { return SMALFIT_ABI_VERSION; }
#ifdef SMALFIT_DEV_PROBES
void smalfit_debug_set(int flags) { g_dbg = flags; }
int smalfit_debug_stats(smalfit_engine* e, int* out8) {
  (void)hipDeviceSynchronize();
  (void)hipMemcpy(out8, e->status, 8 * sizeof(int), hipMemcpyDeviceToHost);
  (void)hipMemset(e->status, 0, 8 * sizeof(int));
  return 0;
}
#endif
#ifdef SMALFIT_WORK_STATS
int smalfit_debug_work_stats(unsigned long long* out32) {   // read and clear the face-sweep work counters
  (void)hipDeviceSynchronize();
  (void)hipMemcpyFromSymbol(out32, HIP_SYMBOL(smalfit::g_work), 32 * sizeof(unsigned long long));
  static const unsigned long long z[32] = {0};
  (void)hipMemcpyToSymbol(HIP_SYMBOL(smalfit::g_work), z, sizeof(z));
  return 0;
}
#endif
#ifdef SMALFIT_PHASES
int smalfit_debug_phase_stats(unsigned long long* out192) {   // read and clear the phase timers of the latency-chain kernels (tools/lbs_phases.py)
  (void)hipDeviceSynchronize();
  (void)hipMemcpyFromSymbol(out192, HIP_SYMBOL(smalfit::g_phase), 12 * 16 * sizeof(unsigned long long));
  static const unsigned long long z[12 * 16] = {0};
  (void)hipMemcpyToSymbol(HIP_SYMBOL(smalfit::g_phase), z, sizeof(z));
  return 0;
}
#endif
const char* smalfit_last_error(void) { return g_err.c_str(); }

// ------------------------------------------------------------------------------------------------
// model
// ------------------------------------------------------------------------------------------------
int smalfit_model_create(const smalfit_model_desc* d, smalfit_model** out) {
  if (refused("smalfit_model_create", null_argument_refusal(d && out))) return 1;
  if (refused("smalfit_model_create", model_dims_refusal(d->num_verts, d->num_faces, d->num_betas))) return 1;
  if (refused("smalfit_model_create", model_desc_refusal(d, kDefaultLandmarks, 6))) return 1;
  const ModelPackHost p = pack_smal_model(d);
  Blob b;
  size_t off[kModelTables];
  const auto tables = model_tables(p, d->parents);
  for (int i = 0; i < kModelTables; ++i) off[i] = b.add(tables[i].data, tables[i].bytes);
  unsigned char* base = upload_blob(b, "smalfit_model_create");
  if (!base) return 1;
  smalfit_model* m = new smalfit_model();
  m->blob = base;
  ModelDev& g = m->dev;
  auto floats = [&](ModelTable t) { return (const float*)(base + off[t]); };
  auto ints = [&](ModelTable t) { return (const int*)(base + off[t]); };
  g.V = p.V; g.Vp = p.Vp; g.F = p.F; g.NBall = p.NB;
  g.vt = floats(kT_vt); g.sd = floats(kT_sd); g.pd = floats(kT_pd);
  g.Kw = p.Kw; g.w_j = ints(kT_w_j); g.w_val = floats(kT_w_val);
  g.wc_off = ints(kT_wc_off); g.wc_v = ints(kT_wc_v); g.wc_val = floats(kT_wc_val);
  g.jr_off = ints(kT_jr_off); g.jr_v = ints(kT_jr_v); g.jr_val = floats(kT_jr_val);
  g.Kj = p.Kj; g.jrv_j = ints(kT_jrv_j); g.jrv_val = floats(kT_jrv_val);
  g.Jt = floats(kT_Jt); g.JS = floats(kT_JS);
  g.parents = ints(kT_parents); g.faces = ints(kT_faces);
  g.vf_off = ints(kT_vf_off); g.vf_idx = ints(kT_vf_idx);
  g.scale_idx = ints(kT_sidx);
  for (int i = 0; i < 6; ++i) g.landmarks[i] = kDefaultLandmarks[i];
  g.tree = tree_levels(d->parents);
  m->V = p.V; m->Vp = p.Vp; m->F = p.F; m->NBall = p.NB;
  *out = m;
  return 0;
}

void smalfit_model_destroy(smalfit_model* m) {
  if (!m) return;
  if (m->blob) (void)hipFree(m->blob);
  delete m;
}

// ------------------------------------------------------------------------------------------------
// engine
// ------------------------------------------------------------------------------------------------
int smalfit_engine_create(smalfit_model* model, int max_frames, int image_size, smalfit_engine** out) {
  if (refused("smalfit_engine_create", engine_create_refusal(model && out, max_frames, image_size))) return 1;
  smalfit_engine* e = new smalfit_engine();
  e->model = model;
  e->maxM = max_frames;
  e->Mp = (int)align_up((size_t)max_frames, 16);
  e->S = image_size;
  e->Tx = (image_size + 15) / 16;
  e->T = e->Tx * e->Tx;
  e->nrb = resolve_tiles(image_size);   // per frame
  e->nvt = vertex_blocks(model->Vp);
  e->nblk_beta = nblk_beta(model->Vp);
  const size_t M = max_frames, Vp = model->Vp, F = model->F, S = image_size, T = e->T;
  Carver w;
  w.field(e->theta, M * 105);
  w.field(e->v_shaped, M * 3 * Vp);
  w.field(e->Jrest, M * 105);
  w.field(e->Rm, M * 315);
  w.field(e->Gm, M * 420);
  w.field(e->scm, M * 105);
  w.field(e->Am, M * 420);
  w.field(e->pfT, (size_t)308 * e->Mp);
  w.field(e->vposed, M * 3 * Vp);
  w.field(e->verts, M * 3 * Vp);
  w.field(e->proj, M * 3 * Vp);
  w.field(e->joints, M * 123);
  w.field(e->fbox, M * F);
  w.field(e->frec, M * F * kRecVecs);
  w.field(e->brect, M * rect_count(model->F));
  w.field(e->plist, M * F * kListCap);
  w.field(e->pcount, M * F);
  w.field(e->gacc, M * S * S);
  w.field(e->bcnt, M * S * S);
  w.field(e->zband, M * S * S);
  w.field(e->qcount, kQCountInts);
  w.field(e->frect, M * 4);
  w.field(e->queue, M * S * S);
  w.field(e->bqueue, M * S * S);
  w.field(e->qloss, kQueueLossBlocks);
  w.field(e->status, 8);
  w.field(e->gz, M * S * S);
  w.field(e->silbuf, M * S * S);
  w.field(e->tile_loss, M * (size_t)e->nrb);
  w.field(e->dface, M * F * 6);
  w.field(e->dJ41, M * 123);
  w.field(e->dvert, M * 3 * Vp);
  w.field(e->dvp, M * 3 * Vp);
  w.field(e->dext, M * 3 * Vp);
  w.field(e->dA, M * 420);
  w.field(e->dpf_part, (size_t)e->CS * M * 308);
  w.field(e->dbeta_part, dbeta_rows(max_frames) * e->nblk_beta * model->NBall);
  w.field(e->dtheta, M * 105);
  w.field(e->dls, M * 6);
  w.field(e->dJrest, M * 105);
  w.field(e->dbetaJ, M * (size_t)model->NBall);
  w.field(e->dth_direct, M * 105);
  w.field(e->dtr_direct, M * 3);
  w.field(e->dtr_part, (size_t)e->nvt * M * 3);
  w.field(e->loss_part, M * 8);
  w.field(e->loss_betas, 4);
  w.field(e->lpart, 64);
  w.field(e->qpart, 64);
  w.field(e->zc, M);
  w.field(e->asm_counter, 4);
  w.field(e->shstate, 2 * kSharedSlotFloats);
  w.field(e->step_counter, 4);
  w.field(e->gb_prior, 64);
  w.field(e->gls_prior, 16);
  w.field(e->loss_betas_pf, M);
  w.field(e->gb_prior_pf, M * 32);
  w.field(e->gls_prior_pf, M * 8);
  w.field(e->frame_qloss, M * kFrameLossStride);
  w.field(e->win_gb, M * kWindowRowBetas);      // (a window holds at least one frame: at most M rows)
  w.field(e->win_gls, M * kWindowRowScales);
  w.field(e->ones, 128);
  w.field(e->zeros, M * 128);
  w.field(e->canon, 32);
  w.field(e->pose_prec, 105 * 105);
  w.field(e->pose_mean, 105);
  w.field(e->pose_mask, 105);
  w.field(e->lim_min, 102);
  w.field(e->lim_max, 102);
  w.field(e->shape_prec, 41 * 41);
  w.field(e->shape_mean, 41);
  const size_t slab_bytes = align_up(w.bytes, 256);
  if (hipMalloc(&e->slab, slab_bytes) != hipSuccess) { delete e; return fail("smalfit_engine_create: hipMalloc of workspace failed"); }
  w.point(e->slab);
  if (hipMemset(e->slab, 0, slab_bytes) != hipSuccess) { (void)hipFree(e->slab); delete e; return fail("smalfit_engine_create: hipMemset failed"); }
  if (hipMemsetD32((hipDeviceptr_t)e->zband, 0x7f800000, (size_t)M * S * S * 2) != hipSuccess ||
      hipMalloc(&e->blist, (size_t)M * S * S * kBandCap * sizeof(float2)) != hipSuccess) {
    (void)hipFree(e->slab); delete e; return fail("smalfit_engine_create: allocation of the band lists failed");
  }
  std::vector<float> ones(128, 1.0f);
  (void)hipMemcpy(e->ones, ones.data(), 128 * 4, hipMemcpyHostToDevice);
  (void)hipMemcpy(e->canon, kCanonical, 25 * 4, hipMemcpyHostToDevice);
  *out = e;
  return 0;
}

void smalfit_engine_destroy(smalfit_engine* e) {
  if (!e) return;
  for (auto ev : e->prof_ev) (void)hipEventDestroy(ev);
  if (e->graph_exec) (void)hipGraphExecDestroy(e->graph_exec);
  if (e->slab) (void)hipFree(e->slab);
  if (e->blist) (void)hipFree(e->blist);
  if (e->zbuf) (void)hipFree(e->zbuf);
  if (e->cover) (void)hipFree(e->cover);
  if (e->vnorm) (void)hipFree(e->vnorm);
  delete e;
}

int smalfit_engine_status(smalfit_engine* e, void* stream, int* bits) {
  if (refused("smalfit_engine_status", null_argument_refusal(e && bits))) return 1;
  hipStream_t st = (hipStream_t)stream;
  HIP_OK(hipStreamSynchronize(st));
  HIP_OK(hipMemcpy(bits, e->status, sizeof(int), hipMemcpyDeviceToHost));
  HIP_OK(hipMemset(e->status, 0, sizeof(int)));
  return 0;
}

int smalfit_engine_reset_raster_cache(smalfit_engine* e, void* stream) {
  if (refused("smalfit_engine_reset_raster_cache", null_argument_refusal(e != nullptr))) return 1;
  HIP_OK(hipMemsetD32Async((hipDeviceptr_t)e->zband, 0x7f800000, (size_t)e->maxM * e->S * e->S * 2, (hipStream_t)stream));
  return 0;
}

int smalfit_engine_set_pose_prior(smalfit_engine* e, const float* prec, const float* mean, const float* mask) {
  if (refused("smalfit_engine_set_pose_prior", null_argument_refusal(e && prec && mean && mask))) return 1;
  HIP_OK(hipMemcpy(e->pose_prec, prec, 105 * 105 * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(e->pose_mean, mean, 105 * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(e->pose_mask, mask, 105 * 4, hipMemcpyHostToDevice));
  e->has_pose_prior = true;
  e->config_epoch++;
  return 0;
}

int smalfit_engine_set_joint_limits(smalfit_engine* e, const float* min_values, const float* max_values) {
  if (refused("smalfit_engine_set_joint_limits", null_argument_refusal(e && min_values && max_values))) return 1;
  if (refused("smalfit_engine_set_joint_limits", joint_limits_refusal(min_values, max_values))) return 1;
  HIP_OK(hipMemcpy(e->lim_min, min_values, 102 * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(e->lim_max, max_values, 102 * 4, hipMemcpyHostToDevice));
  e->has_joint_limits = true;
  e->config_epoch++;
  return 0;
}

int smalfit_engine_clear_joint_limits(smalfit_engine* e) {
  if (refused("smalfit_engine_clear_joint_limits", null_argument_refusal(e != nullptr))) return 1;
  e->has_joint_limits = false;
  e->config_epoch++;
  return 0;
}

int smalfit_engine_set_option(smalfit_engine* e, int option, int value) {
  if (refused("smalfit_engine_set_option", null_argument_refusal(e != nullptr))) return 1;
  if (refused("smalfit_engine_set_option", option_refusal(option, value))) return 1;
  if (option == SMALFIT_OPT_UNCLAMPED_EDGE_T) e->unclamped_edge_t = value != 0;
  e->config_epoch++;
  return 0;
}

int smalfit_engine_set_shape_prior(smalfit_engine* e, const float* prec, const float* mean, int dim) {
  if (refused("smalfit_engine_set_shape_prior", shape_prior_refusal(e && prec && mean, dim))) return 1;
  HIP_OK(hipMemcpy(e->shape_prec, prec, (size_t)dim * dim * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(e->shape_mean, mean, (size_t)dim * 4, hipMemcpyHostToDevice));
  e->shape_dim = dim;
  e->config_epoch++;
  return 0;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// internal pipelines
// ------------------------------------------------------------------------------------------------
namespace smalfit {

// shape -> pose -> skin (+ joints).  theta must already be in e->theta.
// optional extras of the head launch: build theta from the fitter's parameters, evaluate the shape prior (as EvalPlan says)
struct HeadExtras {
  const float *grot = nullptr, *jrot = nullptr, *gmask = nullptr, *rmask = nullptr;
  HeadKernel head = HeadKernel::Plain;    // EvalPlan::head
  HeadPrior prior = HeadPrior::None;      // EvalPlan::head_prior, with prior_dim, prior_uses_ls, prior_weight
  int prior_D = 0, prior_use_ls = 0;
  float prior_w = 0.f;
  const float *Rs_in = nullptr, *joff = nullptr, *voff = nullptr;   // SMAL.__call__ options (component API)
  int joff_stride = 0;
  const PendingStep* pending = nullptr;   // HeadKernel::Step: the optimiser step the previous evaluation left to this launch
  int prior_slot = 0;                     // which half of gb_prior / gls_prior the prior block writes (a pending step reads the other)
};
static constexpr int kPriorSlotB = 32, kPriorSlotLs = 8;   // floats per slot of smalfit_engine::gb_prior / gls_prior, per row of gb_prior_pf / gls_prior_pf

static int run_lbs_forward(smalfit_engine* e, hipStream_t st, int M, const float* betas, int betas_stride,
                           int nb, const float* logscale, int ls_stride, const float* trans,
                           float* joints_out, const HeadExtras* ex = nullptr) {
  const ModelDev& m = e->model->dev;
  const HeadExtras none{};
  const HeadExtras& x = ex ? *ex : none;
  HeadArgs h;
  std::memset(&h, 0, sizeof(h));
  h.M = M; h.Mp = e->Mp; h.nb = nb; h.betas_stride = betas_stride; h.ls_stride = ls_stride;
  h.nshape_x = vertex_blocks(m.Vp); h.nshape = head_shape_blocks(M, m.Vp, betas_stride != 0);
  h.betas = betas; h.logscale = logscale;
  h.theta_in = x.grot ? nullptr : e->theta;       // component API: theta was copied in by the caller
  h.grot = x.grot; h.jrot = x.jrot; h.gmask = x.gmask; h.rmask = x.rmask;
  h.Rs_in = x.Rs_in; h.joff = x.joff; h.joff_stride = x.joff_stride; h.voff = x.voff;
  h.theta = e->theta; h.Jrest = e->Jrest; h.v_shaped = e->v_shaped;
  h.Rm = e->Rm; h.Gm = e->Gm; h.scm = e->scm; h.Am = e->Am; h.pfT = e->pfT;
  if (x.prior != HeadPrior::None) {
    h.prior_prec = e->shape_prec; h.prior_mean = e->shape_mean; h.prior_D = x.prior_D; h.prior_use_ls = x.prior_use_ls;
    h.prior_w = x.prior_w; h.prior_loss = e->loss_betas;
    h.prior_gb = e->gb_prior + x.prior_slot * kPriorSlotB; h.prior_gls = e->gls_prior + x.prior_slot * kPriorSlotLs;
  }
  PriorFrames pf;
  std::memset(&pf, 0, sizeof(pf));
  if (x.prior == HeadPrior::PerFrame) {
    pf.on = 1; pf.loss = e->loss_betas_pf; pf.gb = e->gb_prior_pf; pf.gb_stride = kPriorSlotB; pf.gls = e->gls_prior_pf; pf.gls_stride = kPriorSlotLs;
  }
  const int nhead = head_blocks(M, m.Vp, betas_stride != 0, x.prior);
  switch (x.head) {
    case HeadKernel::Step: lbs_head_step_kernel<<<nhead, 256, 0, st>>>(m, h, *x.pending); break;
    case HeadKernel::Images: lbs_head_images_kernel<<<nhead, 256, 0, st>>>(m, h, pf); break;
    case HeadKernel::Plain: lbs_head_kernel<<<nhead, 256, 0, st>>>(m, h); break;
  }
  LAUNCH_OK("lbs_head_kernel");
  const int vs_stride = betas_stride ? 3 * m.Vp : 0;
  const SkinForm form = skin_form(M, m.Vp);
  const Grid2 sg = skin_grid(form, M, m.Vp);
  switch (form) {
    case SkinForm::Wide:
      skin_mfma_kernel<<<dim3(sg.x, sg.y), 256, 0, st>>>(m, M, e->Mp, e->v_shaped, vs_stride, e->pfT, e->Am, trans, e->vposed, e->verts, e->proj);
      break;
    case SkinForm::Split:
      skin_mfma_split_kernel<<<dim3(sg.x, sg.y), kSkinThreads, 0, st>>>(m, M, e->Mp, e->v_shaped, vs_stride, e->pfT, e->Am, trans, e->vposed,
                                                                     e->verts, e->proj);
      break;
    case SkinForm::Plain:
      skin_kernel<8><<<dim3(sg.x, sg.y), 256, 0, st>>>(m, M, e->Mp, e->v_shaped, vs_stride, e->pfT, e->Am, trans, e->vposed, e->verts, e->proj);
      break;
  }
  LAUNCH_OK("skin_kernel");
  if (joints_out) {   // callers that only need the vertices (smalfit_fit3d_step) skip the joint regression
    joints_kernel<<<dim3(kJointBlocks, M), 128, 0, st>>>(m, e->verts, joints_out);
    LAUNCH_OK("joints_kernel");
  }
  return 0;
}

// the queue kernels in the instantiation EvalPlan::frame_loss selects (floss: the per-frame counters it then feeds)
template <typename... Args>
static void launch_raster_band(hipStream_t st, bool frame_loss, Args... args) {
  if (frame_loss) raster_band_kernel<true><<<kBandBlocks, 256, 0, st>>>(args...);
  else raster_band_kernel<false><<<kBandBlocks, 256, 0, st>>>(args...);
}
template <typename... Args>
static void launch_raster_select(hipStream_t st, bool frame_loss, Args... args) {
  if (frame_loss) raster_select_kernel<true><<<kSelectBlocks, 64 * kSelWaves, 0, st>>>(args...);
  else raster_select_kernel<false><<<kSelectBlocks, 64 * kSelWaves, 0, st>>>(args...);
}

// sweep (face boxes / records, per-pixel count + log-alpha), resolve (K-nearest).  e->proj holds camera-space vertices.
// `joints_out` / `la`: the joint regression and the per-frame loss terms ride along as extra workgroups of the sweep and
// resolve launches (they depend on the skinned vertices only and are needed by the backward pass only).
// `queue_loss` / `floss`: the queue kernels write their loss partials / count them per frame too (EvalPlan)
static int run_raster_forward(smalfit_engine* e, hipStream_t st, int M, WinMap win, float w_sil,
                              SilTarget tsil, float* sil_out, float* blk_loss,
                              float* joints_out = nullptr, const LossArgs* la = nullptr, bool queue_loss = false,
                              unsigned long long* floss = nullptr) {
  // e->gz is persistent state: .y carries each pixel's depth threshold into the next evaluation (verified there)
  float2* gz = e->gz;
  const ModelDev& m = e->model->dev;
  {
    // (SMALFIT_SEC_RASTER_BBOX records nothing any more: the sweep forms its faces' boxes and records itself)
    Section sec(e, st, SMALFIT_SEC_RASTER_SWEEP);
    // the per-pixel accumulators are zero here: whoever reads them last (resolve / band kernel) clears them; the two
    // queue counters are reset by the sweep launch's first frame rider
    raster_sweep_kernel<<<sweep_launch_grid(m.F, M, joints_out != nullptr), 256, 0, st>>>(m, M, e->S, e->proj, e->frec, e->fbox, e->brect, e->zc, e->frect,
                                                                                      e->qcount, e->verts, joints_out, e->zband, e->gacc, e->bcnt,
                                                                                      e->blist, e->plist, e->pcount);
    LAUNCH_OK("raster_sweep_kernel");
  }
  {
    Section sec(e, st, SMALFIT_SEC_RASTER_RESOLVE);
    LossArgs no_loss;
    std::memset(&no_loss, 0, sizeof(no_loss));
    const int loss_frames = la ? M : 0;
    raster_resolve_kernel<<<resolve_grid(e->nrb, M, loss_frames), 256, 0, st>>>(e->S, M, win, w_sil, e->gacc, e->bcnt, e->frect, e->zband, tsil, sil_out, gz,
                                                                             blk_loss, e->qcount, e->queue, e->bqueue, g_dbg ? e->status : nullptr,
                                                                             la ? *la : no_loss, loss_frames);
    LAUNCH_OK("raster_resolve_kernel");
    // the band kernel's loss partials follow the select kernel's in qloss
    launch_raster_band(st, floss != nullptr, e->S, M, win, w_sil, e->gacc, e->bcnt, e->blist, tsil, sil_out, gz, e->zband,
                       e->qcount, e->queue, e->bqueue, queue_loss ? e->qloss + kSelectBlocks : nullptr, floss);
    LAUNCH_OK("raster_band_kernel");
  }
  Section sec(e, st, SMALFIT_SEC_RASTER_SELECT);
  launch_raster_select(st, floss != nullptr, m.F, e->S, M, win, w_sil, e->frec, e->zc, e->brect, e->fbox, e->qcount, e->queue,
                       tsil, sil_out, gz, e->zband, e->pcount, queue_loss ? e->qloss : nullptr, g_dbg, floss);
  LAUNCH_OK("raster_select_kernel");
  return 0;
}

// everything downstream of d(verts): dA, pose-blend / shape-blend adjoints, chain adjoint
static int run_lbs_backward(smalfit_engine* e, hipStream_t st, int M, int nb, int betas_shared,
                            const float* dface, const float* dJ41, const float* dext, bool need_pose,
                            bool need_beta, bool need_ls, const float* dth_direct, int j_stride, float* dRs_out = nullptr) {
  const ModelDev& m = e->model->dev;
  vertex_bwd_kernel<<<vertex_bwd_grid(m.Vp, M), 256, 0, st>>>(m, M, e->proj, dface, dJ41, dext, e->Am, e->dvert, e->dvp, e->dtr_part);
  LAUNCH_OK("vertex_bwd_kernel");
  const int nPB = need_pose ? mid_pb_ids(M) : 0;   // (up to PBM_TILES x 16 frames) x 32 pose features x column split
  const DbetaGrid db = dbeta_grid(need_beta, m.Vp, betas_shared != 0, M);
  lbs_bwd_mid_kernel<<<mid_grid(M, nPB), 256, 0, st>>>(m, M, nPB, e->dvert, e->vposed, e->dvp, e->dA, e->dpf_part);
  LAUNCH_OK("lbs_bwd_mid_kernel");
  // the shape-blend adjoint partials ride on the chain launch: db.blocks() workgroups after its M frame blocks
  chain_bwd_kernel<<<chain_grid(M, db), 256, 0, st>>>(m, M, e->theta, e->Rm, e->Gm, e->scm, e->Jrest, j_stride, e->dA,
                                                    need_pose ? e->dpf_part : nullptr, e->CS, dth_direct, e->dtheta,
                                                    need_ls ? e->dls : nullptr, e->dJrest, need_beta ? e->dbetaJ : nullptr, dRs_out,
                                                    nb, betas_shared, db.bx, db.by, db.bz, e->dvp, e->dbeta_part);
  LAUNCH_OK("chain_bwd_kernel");
  return 0;
}

// d/d betas of M frames with their own shapes, nb floats each, from the partials run_lbs_backward (betas_shared 0) left:
// assemble_kernel with only its per-frame betas roles
static int launch_frame_betas_assembly(smalfit_engine* e, hipStream_t st, int M, int nb, float* g_betas) {
  const ModelDev& m = e->model->dev;
  AssembleArgs g;
  std::memset(&g, 0, sizeof(g));
  g.M = M; g.nb = nb; g.NBall = m.NBall; g.nblk_beta = e->nblk_beta; g.betas_shared = 0;
  g.dbeta_part = e->dbeta_part; g.dJrest = e->dJrest; g.JS = m.JS; g.dbetaJ = e->dbetaJ; g.ngrp_beta = 1; g.g_betas = g_betas;
  g.win = WinMap{1, 0, M};
  assemble_kernel<false><<<frame_betas_grid(M), 256, 0, st>>>(g, AssembleExt{});
  LAUNCH_OK("assemble_kernel");
  return 0;
}

}  // namespace smalfit

// ------------------------------------------------------------------------------------------------
// SMALFitter fused evaluation
// ------------------------------------------------------------------------------------------------
namespace smalfit {
// How smalfit_fit_run strings evaluations together: an evaluation may take over the optimiser step its predecessor left pending
// (lbs_head_step_kernel), and may itself stop after the backward pass, leaving gradient assembly + Adam to its successor.
struct EvalFold {
  const PendingStep* pending = nullptr;   // taken by this evaluation's head launch
  int prior_slot = 0;                     // half of the shape prior's gradient buffers this evaluation writes
  bool assemble = true;                   // run assemble_kernel (gradients to the caller's buffers, the nine loss terms)
  AssembleArgs* args_out = nullptr;       // the assembly's arguments, for the successor's pending step
  const smalfit_window_rows* window_rows = nullptr;   // smalfit_fit_eval_windows: one row per window (checked by the caller)
};
static EngineFacts engine_facts(const smalfit_engine* e) { return EngineFacts{e->maxM, e->has_pose_prior, e->shape_dim, e->has_joint_limits}; }

// plan_eval decides; here the plan's fields and the pointers of the block, the rows and the engine meet in the kernels' arguments
static int fit_eval_impl(smalfit_engine* e, void* stream, const smalfit_fit_args* a, const EvalFold& fold) {
  if (refused("smalfit_fit_eval", null_argument_refusal(e && a))) return 1;
  if (refused("smalfit_fit_eval", fit_args_refusal(a, engine_facts(e)))) return 1;
  if (refused("smalfit_fit_eval", fit_model_refusal(e->model->NBall))) return 1;
  const smalfit_window_rows* wr = fold.window_rows;
  EvalMode mode;
  mode.pending = fold.pending != nullptr; mode.assemble = fold.assemble;
  mode.window_rows = wr != nullptr; mode.want_betas = wr && wr->g_betas; mode.want_scales = wr && wr->g_log_beta_scales;
  const EvalPlan p = plan_eval(a, engine_facts(e), mode);
  const int M = p.M;
  hipStream_t st = (hipStream_t)stream;
  const ModelDev& m = e->model->dev;
  const float* gmask = a->global_mask ? a->global_mask : e->ones;
  const float* rmask = a->rotation_mask ? a->rotation_mask : e->ones;
  {
    Section sec(e, st, SMALFIT_SEC_LBS_FWD);
    HeadExtras ex;
    ex.grot = a->global_rotation; ex.jrot = a->joint_rotations; ex.gmask = gmask; ex.rmask = rmask;
    ex.head = p.head; ex.pending = fold.pending; ex.prior_slot = fold.prior_slot;
    ex.prior = p.head_prior; ex.prior_D = p.prior_dim; ex.prior_use_ls = p.prior_uses_ls ? 1 : 0; ex.prior_w = p.prior_weight;
    if (run_lbs_forward(e, st, M, a->betas, p.betas_stride, p.nb, p.limb_scales ? a->log_beta_scales : nullptr, p.ls_stride, a->trans,
                        p.joints_in_head ? e->joints : nullptr, &ex)) return 1;
  }

  LossArgs la;
  la.M = M; la.S = e->S; la.win = p.win;
  la.theta = e->theta; la.trans = a->trans; la.joints = e->joints; la.canon = e->canon;
  la.tj = a->target_joints; la.vis = a->target_visibility;
  la.w_j2d = a->w_j2d; la.w_pose = a->w_pose; la.w_splay = a->w_splay; la.w_temp = p.w_temp;
  la.w_limit = p.w_limit; la.lim_min = e->lim_min; la.lim_max = e->lim_max;
  la.pose_prec = e->pose_prec; la.pose_mean = e->pose_mean; la.pose_mask = e->pose_mask;
  la.halo_prev = p.halos ? a->halo_prev : nullptr;
  la.halo_next = p.halos ? a->halo_next : nullptr;
  la.proj_out = a->proj_out;
  la.dth_direct = e->dth_direct; la.dJ41 = e->dJ41; la.dtr_direct = e->dtr_direct; la.loss_part = e->loss_part;
  if (p.loss_launch == LossLaunch::OwnKernel) {
    loss_kernel<<<M, 128, 0, st>>>(la);
    LAUNCH_OK("loss_kernel");
  } else {
    const SilTarget tsil{p.sil_target == SilTargetKind::F32 ? a->target_sil : nullptr, p.sil_target == SilTargetKind::U8 ? a->target_sil_u8 : nullptr};
    if (run_raster_forward(e, st, M, p.win, a->w_sil, tsil, a->sil_out, p.sil_on ? e->tile_loss : nullptr, e->joints, &la,
                           p.queue_loss, p.frame_loss ? e->frame_qloss : nullptr)) return 1;
  }
  if (p.raster_backward) {
    Section sec(e, st, SMALFIT_SEC_RASTER_BWD);
    launch_raster_bwd(e, st, M);
    LAUNCH_OK("raster_bwd_kernel");
  }
  if (p.verts_out) {
    planar_to_interleaved_kernel<<<dim3(elem_blocks(m.V * 3), M), 256, 0, st>>>(M, m.V, m.Vp, e->verts, 3 * m.Vp, a->trans, a->verts_out);
    LAUNCH_OK("planar_to_interleaved_kernel");
  }
  {
    Section sec(e, st, SMALFIT_SEC_LBS_BWD);
    if (run_lbs_backward(e, st, M, p.nb, p.bwd_betas_shared, p.raster_backward ? e->dface : nullptr, e->dJ41, nullptr, p.need_pose, p.need_beta,
                         p.need_ls, e->dth_direct, p.j_stride)) return 1;
  }

  const bool prior_shared = p.head_prior == HeadPrior::Shared, prior_rows = p.head_prior == HeadPrior::PerFrame;
  AssembleArgs g;
  g.M = M; g.S = e->S; g.T = e->nrb; g.win = p.win; g.nb = p.nb; g.NBall = m.NBall;
  g.nblk_beta = e->nblk_beta; g.nvt = e->nvt; g.betas_shared = p.asm_betas_shared; g.ls_shared = p.asm_ls_shared;
  g.w_sil = a->w_sil;
  g.dbeta_part = e->dbeta_part; g.dJrest = e->dJrest; g.JS = m.JS; g.dbetaJ = e->dbetaJ; g.ngrp_beta = p.ngrp_beta;
  // (independent images leave the shared-shape slots unused: one row per image instead, AssembleExt)
  g.gb_prior = prior_shared ? e->gb_prior + fold.prior_slot * kPriorSlotB : nullptr;
  g.gls_prior = prior_shared && p.prior_uses_ls ? e->gls_prior + fold.prior_slot * kPriorSlotLs : nullptr;
  g.dls = e->dls; g.dtheta = e->dtheta; g.gmask = gmask; g.rmask = rmask;
  g.dtr_direct = e->dtr_direct; g.dtr_part = e->dtr_part; g.loss_part = e->loss_part;
  g.loss_betas = prior_shared ? e->loss_betas : nullptr;
  g.tile_loss = p.sil_on ? e->tile_loss : nullptr;
  g.qloss = p.queue_loss ? e->qloss : nullptr;
  g.nqblk = kQueueLossBlocks;
  g.g_betas = p.assembly_leaves_betas ? nullptr : a->g_betas;
  g.g_ls = p.need_ls && !p.assembly_leaves_scales ? a->g_log_beta_scales : nullptr;
  g.g_grot = a->g_global_rotation; g.g_jrot = a->g_joint_rotations; g.g_trans = a->g_trans;
  g.losses = a->losses;
  g.lpart = e->lpart; g.qpart = e->qpart; g.counter = e->asm_counter;
  AssembleExt gx;
  std::memset(&gx, 0, sizeof(gx));
  gx.losses_pf = p.rows ? a->losses_per_frame : nullptr; gx.frame_qloss = e->frame_qloss; gx.prior_windows = p.prior_windows;
  if (prior_rows) {
    gx.gb_prior_pf = e->gb_prior_pf; gx.gb_stride = kPriorSlotB; gx.prior_loss_pf = e->loss_betas_pf;
    if (p.prior_uses_ls) { gx.gls_prior_pf = e->gls_prior_pf; gx.gls_stride = kPriorSlotLs; }
  }
  WindowRowsDev wd;
  std::memset(&wd, 0, sizeof(wd));
  if (wr) {
    static_assert(kWindowRowBetas >= 20 && kWindowRowScales >= 6, "a row of the workspace holds a row of the gradient");
    wd.W = p.W; wd.clear_qloss = p.clear_qloss;
    wd.losses = wr->losses; wd.g_betas = wr->g_betas; wd.g_ls = wr->g_log_beta_scales;
    wd.row_betas = p.need_beta ? e->win_gb : nullptr; wd.row_ls = p.ls_rows ? e->win_gls : nullptr;
    wd.tot_betas = a->g_betas; wd.tot_ls = p.ls_rows ? a->g_log_beta_scales : nullptr;
    wd.counter = e->asm_counter + 1;          // (assemble_kernel's is slot 0)
  }
  if (fold.args_out) *fold.args_out = g;
  if (fold.assemble) {
    if (p.independent) assemble_kernel<true><<<assemble_grid(p.asm_shape_sets), 256, 0, st>>>(g, gx);
    else assemble_kernel<false><<<assemble_grid(p.asm_shape_sets), 256, 0, st>>>(g, gx);
    LAUNCH_OK("assemble_kernel");
    if (wr) {     // (before frame_loss_rows_kernel, which clears the per-frame counters both read)
      window_rows_kernel<<<window_rows_grid(wd.W), 256, 0, st>>>(g, gx, wd);
      LAUNCH_OK("window_rows_kernel");
    }
    if (p.rows) {
      frame_loss_rows_kernel<<<frame_loss_rows_grid(), 256, 0, st>>>(g, gx);
      LAUNCH_OK("frame_loss_rows_kernel");
    }
  }
  if (e->prof_on) {
    if (e->prof_iter < e->prof_cap && (e->prof_tick % e->prof_stride) == 0) e->prof_iter++;
    e->prof_tick++;
  }
  return 0;
}
}  // namespace smalfit

extern "C" {

int smalfit_fit_eval(smalfit_engine* e, void* stream, const smalfit_fit_args* a) { return fit_eval_impl(e, stream, a, EvalFold{}); }

int smalfit_fit_eval_windows(smalfit_engine* e, void* stream, const smalfit_fit_args* a, const smalfit_window_rows* rows) {
  if (refused("smalfit_fit_eval_windows", null_argument_refusal(e && a && rows))) return 1;
  // the sizes of both blocks before any other field of either
  if (refused("smalfit_fit_eval_windows", window_rows_size_refusal(rows))) return 1;
  if (refused("smalfit_fit_eval_windows", fit_args_refusal(a, engine_facts(e)))) return 1;
  if (refused("smalfit_fit_eval_windows", window_rows_refusal(a, rows))) return 1;
  EvalFold fold;
  fold.window_rows = rows;
  return fit_eval_impl(e, stream, a, fold);
}

// ------------------------------------------------------------------------------------------------
// per-section timing with HIP events on the caller's stream
// ------------------------------------------------------------------------------------------------
int smalfit_engine_profile_begin(smalfit_engine* e, int max_evals, int stride) {
  if (refused("smalfit_engine_profile_begin", profile_begin_refusal(e != nullptr, max_evals, stride))) return 1;
  for (auto ev : e->prof_ev) (void)hipEventDestroy(ev);
  e->prof_ev.assign((size_t)max_evals * SMALFIT_NUM_SECTIONS * 2, nullptr);
  for (auto& ev : e->prof_ev) HIP_OK(hipEventCreate(&ev));
  e->prof_cap = max_evals;
  e->prof_iter = 0;
  e->prof_stride = stride;
  e->prof_tick = 0;
  e->prof_on = true;
  return 0;
}

int smalfit_engine_profile_end(smalfit_engine* e, void* stream, float* ms_total, int* counts) {
  if (refused("smalfit_engine_profile_end", null_argument_refusal(e && ms_total && counts))) return 1;
  HIP_OK(hipStreamSynchronize((hipStream_t)stream));
  e->prof_on = false;
  for (int sct = 0; sct < SMALFIT_NUM_SECTIONS; ++sct) { ms_total[sct] = 0.f; counts[sct] = 0; }
  for (int it = 0; it < e->prof_iter; ++it)
    for (int sct = 0; sct < SMALFIT_NUM_SECTIONS; ++sct) {
      float ms = 0.f;
      hipEvent_t a = e->prof_ev[((size_t)it * SMALFIT_NUM_SECTIONS + sct) * 2];
      hipEvent_t b = e->prof_ev[((size_t)it * SMALFIT_NUM_SECTIONS + sct) * 2 + 1];
      if (hipEventElapsedTime(&ms, a, b) == hipSuccess) { ms_total[sct] += ms; counts[sct]++; }
    }
  (void)hipGetLastError();   // sections that did not run in an evaluation leave unrecorded events: not an error
  for (auto ev : e->prof_ev) (void)hipEventDestroy(ev);
  e->prof_ev.clear();
  e->prof_cap = e->prof_iter = 0;
  return 0;
}

// ------------------------------------------------------------------------------------------------
// SMAL.__call__ and its adjoint
// ------------------------------------------------------------------------------------------------
namespace smalfit {
// stages a per-frame template offset: planar copy in e->dext, its joint regression (rows of 123 floats) in e->dJ41
static int stage_vertex_offset(smalfit_engine* e, hipStream_t st, int M, const float* v_offset, HeadExtras& ex) {
  const ModelDev& m = e->model->dev;
  interleaved_to_planar_kernel<<<dim3(vertex_blocks(m.Vp), M), 256, 0, st>>>(M, m.V, m.Vp, v_offset, e->dext);
  LAUNCH_OK("interleaved_to_planar_kernel");
  joints_kernel<<<dim3(kJointBlocks, M), 128, 0, st>>>(m, e->dext, e->dJ41);
  LAUNCH_OK("joints_kernel");
  ex.voff = e->dext; ex.joff = e->dJ41; ex.joff_stride = 123;
  return 0;
}
static int check_lbs_args(smalfit_engine* e, const smalfit_lbs_args* a, const char* who) {
  if (refused(who, null_argument_refusal(e && a))) return 1;
  return refused(who, lbs_args_refusal(a, e->maxM, e->model->dev.NBall));
}
static int lbs_forward_common(smalfit_engine* e, hipStream_t st, const smalfit_lbs_args* a, float* joints_out) {
  const int M = a->num_frames, nb = a->num_betas;
  HeadExtras ex;
  if (a->theta) HIP_OK(hipMemcpyAsync(e->theta, a->theta, (size_t)M * 105 * 4, hipMemcpyDeviceToDevice, st));
  else HIP_OK(hipMemsetAsync(e->theta, 0, (size_t)M * 105 * 4, st));
  ex.Rs_in = a->Rs;
  if (a->v_offset && stage_vertex_offset(e, st, M, a->v_offset, ex)) return 1;
  return run_lbs_forward(e, st, M, a->beta, nb, nb, a->logscale, 6, e->zeros, joints_out, &ex);
}
}  // namespace smalfit

int smalfit_lbs_forward_ex(smalfit_engine* e, void* stream, const smalfit_lbs_args* a) {
  if (check_lbs_args(e, a, "smalfit_lbs_forward_ex")) return 1;
  if (refused("smalfit_lbs_forward_ex", lbs_outputs_refusal(a))) return 1;
  const ModelDev& m = e->model->dev;
  const int M = a->num_frames;
  hipStream_t st = (hipStream_t)stream;
  if (lbs_forward_common(e, st, a, a->joints)) return 1;
  const dim3 grid(elem_blocks(m.V * 3), M);
  planar_to_interleaved_kernel<<<grid, 256, 0, st>>>(M, m.V, m.Vp, e->verts, 3 * m.Vp, nullptr, a->verts);
  if (a->v_shaped) planar_to_interleaved_kernel<<<grid, 256, 0, st>>>(M, m.V, m.Vp, e->v_shaped, 3 * m.Vp, nullptr, a->v_shaped);
  LAUNCH_OK("planar_to_interleaved_kernel");
  if (a->Rs_out) HIP_OK(hipMemcpyAsync(a->Rs_out, e->Rm, (size_t)M * 315 * 4, hipMemcpyDeviceToDevice, st));
  return 0;
}

int smalfit_lbs_backward_ex(smalfit_engine* e, void* stream, const smalfit_lbs_args* a) {
  if (check_lbs_args(e, a, "smalfit_lbs_backward_ex")) return 1;
  const ModelDev& m = e->model->dev;
  const int M = a->num_frames, nb = a->num_betas;
  hipStream_t st = (hipStream_t)stream;
  // the forward's joint output doubles as scratch for the offset's joint regression: regress into e->joints afterwards
  if (lbs_forward_common(e, st, a, e->joints)) return 1;
  const float* dext = nullptr;
  if (a->dverts) {
    // (e->dext held the planar offset during the forward; the head kernel has consumed it)
    interleaved_to_planar_kernel<<<dim3(vertex_blocks(m.Vp), M), 256, 0, st>>>(M, m.V, m.Vp, a->dverts, e->dext);
    LAUNCH_OK("interleaved_to_planar_kernel");
    dext = e->dext;
  }
  // djoints may alias nothing inside the engine: the offset staging used e->dJ41, which run_lbs_backward reads as the joint
  // adjoint -- copy the caller's (or zeros) in now that the forward is done
  const float* dj = a->djoints;
  if (a->v_offset) {
    if (dj) HIP_OK(hipMemcpyAsync(e->dJ41, dj, (size_t)M * 123 * 4, hipMemcpyDeviceToDevice, st));
    else HIP_OK(hipMemsetAsync(e->dJ41, 0, (size_t)M * 123 * 4, st));
    dj = e->dJ41;
  }
  if (run_lbs_backward(e, st, M, nb, 0, nullptr, dj, dext, true, a->dbeta != nullptr || a->dv_offset != nullptr,
                       a->logscale != nullptr && a->dlogscale != nullptr, nullptr, 105, a->Rs ? a->dRs : nullptr)) return 1;
  if (a->dtheta && a->theta) HIP_OK(hipMemcpyAsync(a->dtheta, e->dtheta, (size_t)M * 105 * 4, hipMemcpyDeviceToDevice, st));
  if (a->dlogscale) {
    if (a->logscale) HIP_OK(hipMemcpyAsync(a->dlogscale, e->dls, (size_t)M * 6 * 4, hipMemcpyDeviceToDevice, st));
    else HIP_OK(hipMemsetAsync(a->dlogscale, 0, (size_t)M * 6 * 4, st));
  }
  if (a->dbeta && launch_frame_betas_assembly(e, st, M, nb, a->dbeta)) return 1;
  if (a->dv_offset) {
    offset_grad_kernel<<<dim3(elem_blocks(m.V), M), 256, 0, st>>>(m, M, e->dvp, e->dJrest, a->dv_offset);
    LAUNCH_OK("offset_grad_kernel");
  }
  return 0;
}

int smalfit_lbs_forward(smalfit_engine* e, void* stream, int M, int nb, const float* beta, const float* theta,
                        const float* logscale, float* verts, float* joints, float* Rs, float* v_shaped) {
  if (refused("smalfit_lbs_forward", null_argument_refusal(theta != nullptr))) return 1;
  smalfit_lbs_args a;
  std::memset(&a, 0, sizeof(a));
  a.num_frames = M; a.num_betas = nb; a.beta = beta; a.theta = theta; a.logscale = logscale;
  a.verts = verts; a.joints = joints; a.Rs_out = Rs; a.v_shaped = v_shaped;
  return smalfit_lbs_forward_ex(e, stream, &a);
}

int smalfit_lbs_backward(smalfit_engine* e, void* stream, int M, int nb, const float* beta, const float* theta,
                         const float* logscale, const float* dverts, const float* djoints, float* dbeta,
                         float* dtheta, float* dlogscale) {
  if (refused("smalfit_lbs_backward", null_argument_refusal(theta != nullptr))) return 1;
  smalfit_lbs_args a;
  std::memset(&a, 0, sizeof(a));
  a.num_frames = M; a.num_betas = nb; a.beta = beta; a.theta = theta; a.logscale = logscale;
  a.dverts = dverts; a.djoints = djoints; a.dbeta = dbeta; a.dtheta = dtheta; a.dlogscale = dlogscale;
  return smalfit_lbs_backward_ex(e, stream, &a);
}

int smalfit_rodrigues(void* stream, int count, const float* theta, float* R) {
  if (refused("smalfit_rodrigues", operator_args_refusal(count, theta && R))) return 1;
  rodrigues_kernel<<<elem_blocks(count), 256, 0, (hipStream_t)stream>>>(count, theta, R);
  LAUNCH_OK("rodrigues_kernel");
  return 0;
}

namespace smalfit {
// the caller's parent table as a kernel argument, checked
static int pack_parents(const int* parents, Parents35& par, const char* who) {
  if (!parents_ordered(parents, 35)) return refused(who, kParentsRefusal);
  par.p[0] = -1;
  for (int i = 1; i < 35; ++i) par.p[i] = parents[i];
  return 0;
}
}  // namespace smalfit

int smalfit_global_rigid_transformation(void* stream, int count, const float* Rs, const float* Js, const int* parents,
                                        const float* logscale, float* new_J, float* A) {
  if (refused("smalfit_global_rigid_transformation", operator_args_refusal(count, Rs && Js && parents && new_J && A))) return 1;
  Parents35 par;
  if (pack_parents(parents, par, "smalfit_global_rigid_transformation")) return 1;
  global_rigid_kernel<<<rigid_blocks(count), 64, 0, (hipStream_t)stream>>>(count, Rs, Js, par, logscale, new_J, A);
  LAUNCH_OK("global_rigid_kernel");
  return 0;
}

int smalfit_global_rigid_transformation_backward(void* stream, int count, const float* Rs, const float* Js, const int* parents,
                                                 const float* logscale, const float* d_new_J, const float* d_A,
                                                 float* scratch, float* dRs, float* dJs, float* dlogscale) {
  if (refused("smalfit_global_rigid_transformation_backward", operator_args_refusal(count, Rs && Js && parents && d_new_J && d_A && scratch && dRs && dJs))) return 1;
  Parents35 par;
  if (pack_parents(parents, par, "smalfit_global_rigid_transformation_backward")) return 1;
  global_rigid_bwd_kernel<<<rigid_blocks(count), 64, 0, (hipStream_t)stream>>>(count, Rs, Js, par, logscale, d_new_J, d_A, scratch, dRs, dJs,
                                                                            logscale ? dlogscale : nullptr);
  LAUNCH_OK("global_rigid_bwd_kernel");
  return 0;
}

int smalfit_rodrigues_backward(void* stream, int count, const float* theta, const float* dR, float* dtheta) {
  if (refused("smalfit_rodrigues_backward", operator_args_refusal(count, theta && dR && dtheta))) return 1;
  rodrigues_bwd_kernel<<<elem_blocks(count), 256, 0, (hipStream_t)stream>>>(count, theta, dR, dtheta);
  LAUNCH_OK("rodrigues_bwd_kernel");
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Renderer
// ------------------------------------------------------------------------------------------------
int smalfit_render_forward(smalfit_engine* e, void* stream, int M, const float* verts, const float* points, int P,
                           float* sil, float* proj_points) {
  if (refused("smalfit_render_forward", null_argument_refusal(e && verts))) return 1;
  if (refused("smalfit_render_forward", render_frames_refusal(M, e->maxM))) return 1;
  hipStream_t st = (hipStream_t)stream;
  const ModelDev& m = e->model->dev;
  if (sil) {
    project_verts_kernel<<<dim3(vertex_blocks(m.Vp), M), 256, 0, st>>>(M, m.V, m.Vp, verts, e->proj);
    LAUNCH_OK("project_verts_kernel");
    if (run_raster_forward(e, st, M, WinMap{1, 0, M}, 0.f, SilTarget{nullptr, nullptr}, sil, nullptr)) return 1;
  }
  if (points && proj_points && P > 0) {
    project_points_kernel<<<elem_blocks((long long)M * P), 256, 0, st>>>(M * P, e->S, points, proj_points);
    LAUNCH_OK("project_points_kernel");
  }
  return 0;
}

int smalfit_render_color(smalfit_engine* e, void* stream, int M, const float* verts, const float* rgb, float* image) {
  if (refused("smalfit_render_color", null_argument_refusal(e && verts && rgb && image))) return 1;
  if (refused("smalfit_render_color", render_frames_refusal(M, e->maxM))) return 1;
  hipStream_t st = (hipStream_t)stream;
  const ModelDev& m = e->model->dev;
  const size_t npx = (size_t)e->S * e->S;
  if (!e->zbuf && hipMalloc(&e->zbuf, (size_t)e->maxM * npx * sizeof(unsigned long long)) != hipSuccess)
    return fail("smalfit_render_color: hipMalloc of the z-buffer failed");
  if (!e->vnorm && hipMalloc(&e->vnorm, (size_t)e->maxM * 3 * m.Vp * sizeof(float)) != hipSuccess)
    return fail("smalfit_render_color: hipMalloc of the vertex normals failed");
  const dim3 vgrid(vertex_blocks(m.Vp), M);
  interleaved_to_planar_kernel<<<vgrid, 256, 0, st>>>(M, m.V, m.Vp, verts, e->verts);
  project_verts_kernel<<<vgrid, 256, 0, st>>>(M, m.V, m.Vp, verts, e->proj);
  vnormal_kernel<<<vgrid, 256, 0, st>>>(m, M, e->verts, e->vnorm);
  HIP_OK(hipMemsetAsync(e->zbuf, 0xff, (size_t)M * npx * sizeof(unsigned long long), st));
  color_zbuf_kernel<<<dim3(color_face_blocks(m.F), M), 256, 0, st>>>(m, e->S, e->proj, e->zbuf);
  color_shade_kernel<<<dim3((unsigned)elem_blocks((long long)npx), M), 256, 0, st>>>(m, e->S, e->proj, e->verts, e->vnorm, e->zbuf, rgb[0], rgb[1],
                                                                            rgb[2], image);
  LAUNCH_OK("colour render kernels");
  return 0;
}

// silhouette intersection / union counts and PCK per frame (definitions: include/smalfit.h; rules and grids: smalfit_plan.h)
// Like smalfit_render_color it projects into the engine's own workspace (e->proj) and keeps its mask there (e->cover): the call
// must not overlap another call on the same engine (calls on one stream never do); an evaluation after it projects afresh
int smalfit_fit_metrics(smalfit_engine* e, void* stream, const smalfit_metrics_args* a) {
  if (refused("smalfit_fit_metrics", null_argument_refusal(e && a))) return 1;
  if (refused("smalfit_fit_metrics", metrics_args_refusal(a, e->maxM))) return 1;
  hipStream_t st = (hipStream_t)stream;
  const ModelDev& m = e->model->dev;
  const int M = a->num_frames, S = e->S;
  const size_t npx = (size_t)S * S;
  if (!e->cover && hipMalloc(&e->cover, (size_t)e->maxM * npx) != hipSuccess)
    return fail("smalfit_fit_metrics: hipMalloc of the coverage mask failed");
  project_verts_kernel<<<dim3(vertex_blocks(m.Vp), M), 256, 0, st>>>(M, m.V, m.Vp, a->verts, e->proj);
  HIP_OK(hipMemsetAsync(e->cover, 0, (size_t)M * npx, st));
  HIP_OK(hipMemsetAsync(a->sil_counts, 0, (size_t)M * 4 * sizeof(unsigned), st));
  const Grid2 cg = cover_grid(m.F, M), sg = sil_counts_grid(S, M);
  cover_kernel<<<dim3(cg.x, cg.y), 256, 0, st>>>(m, S, e->proj, e->cover);
  if (a->target_sil_u8) sil_counts_kernel<unsigned char><<<dim3(sg.x, sg.y), 256, 0, st>>>(S, e->cover, a->target_sil_u8, a->sil_counts);
  else sil_counts_kernel<float><<<dim3(sg.x, sg.y), 256, 0, st>>>(S, e->cover, a->target_sil, a->sil_counts);
  if (metrics_keypoints(a) && (a->keypoint_dist || a->pck_counts)) {
    PckThresholds thr{};
    for (int t = 0; t < a->num_thresholds; ++t) thr.t[t] = a->thresholds[t];
    pck_kernel<<<pck_grid(M), 64, 0, st>>>(a->proj_joints, a->target_joints, a->target_visibility, a->sil_counts, a->num_thresholds, thr,
                                          a->keypoint_dist, a->pck_counts);
  }
  LAUNCH_OK("metrics kernels");
  if (a->mask_out) HIP_OK(hipMemcpyAsync(a->mask_out, e->cover, (size_t)M * npx, hipMemcpyDeviceToDevice, st));
  return 0;
}

int smalfit_render_backward(smalfit_engine* e, void* stream, int M, const float* verts, const float* sil,
                            const float* dsil, float* dverts) {
  if (refused("smalfit_render_backward", null_argument_refusal(e && verts && sil && dsil && dverts))) return 1;
  if (refused("smalfit_render_backward", render_frames_refusal(M, e->maxM))) return 1;
  hipStream_t st = (hipStream_t)stream;
  const ModelDev& m = e->model->dev;
  project_verts_kernel<<<dim3(vertex_blocks(m.Vp), M), 256, 0, st>>>(M, m.V, m.Vp, verts, e->proj);
  // recompute the forward (stateless adjoint): depth thresholds land in gz.y, then seed gz.x from dsil
  if (run_raster_forward(e, st, M, WinMap{1, 0, M}, 0.f, SilTarget{nullptr, nullptr}, e->silbuf, nullptr)) return 1;
  const size_t total = (size_t)M * e->S * e->S;
  gpix_from_dsil_kernel<<<(unsigned)elem_blocks((long long)total), 256, 0, st>>>(total, sil, dsil, e->gz);
  launch_raster_bwd(e, st, M);
  raster_vertex_grad_kernel<<<dim3(elem_blocks(m.V), M), 256, 0, st>>>(m, e->proj, e->dface, dverts);
  LAUNCH_OK("render_backward kernels");
  return 0;
}

int smalfit_engine_face_list_lengths(smalfit_engine* e, void* stream, int M, unsigned char* lengths) {
  if (refused("smalfit_engine_face_list_lengths", null_argument_refusal(e && lengths))) return 1;
  if (refused("smalfit_engine_face_list_lengths", render_frames_refusal(M, e->maxM))) return 1;
  HIP_OK(hipMemcpyAsync(lengths, e->pcount, (size_t)M * e->model->dev.F, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}

int smalfit_project_points_backward(void* stream, int count, int image_size, const float* points, const float* dproj,
                                    float* dpoints) {
  if (refused("smalfit_project_points_backward", operator_args_refusal(count, points && dproj && dpoints))) return 1;
  project_points_bwd_kernel<<<elem_blocks(count), 256, 0, (hipStream_t)stream>>>(count, image_size, points, dproj, dpoints);
  LAUNCH_OK("project_points_bwd_kernel");
  return 0;
}

int smalfit_pose_prior(smalfit_engine* e, void* stream, int N, const float* x, float* out) {
  if (refused("smalfit_pose_prior", pose_prior_refusal(e && x && out, N, e && e->has_pose_prior))) return 1;
  pose_prior_kernel<<<N, 128, 0, (hipStream_t)stream>>>(x, e->pose_prec, e->pose_mean, e->pose_mask, out);
  LAUNCH_OK("pose_prior_kernel");
  return 0;
}

int smalfit_pose_prior_backward(smalfit_engine* e, void* stream, int N, const float* x, const float* dout, float* dx) {
  if (refused("smalfit_pose_prior_backward", pose_prior_refusal(e && x && dout && dx, N, e && e->has_pose_prior))) return 1;
  pose_prior_bwd_kernel<<<N, 128, 0, (hipStream_t)stream>>>(x, e->pose_prec, e->pose_mean, e->pose_mask, dout, dx);
  LAUNCH_OK("pose_prior_bwd_kernel");
  return 0;
}

int smalfit_temporal(smalfit_engine* e, void* stream, int N, float w_temp, const float* global_rotation,
                     const float* joint_rotations, const float* trans, const float* global_mask,
                     const float* rotation_mask, float* losses, float* g_global_rotation, float* g_joint_rotations,
                     float* g_trans) {
  if (refused("smalfit_temporal", null_argument_refusal(e && global_rotation && joint_rotations && trans && losses))) return 1;
  if (refused("smalfit_temporal", temporal_frames_refusal(N, e->maxM))) return 1;
  hipStream_t st = (hipStream_t)stream;
  const float* gmask = global_mask ? global_mask : e->ones;
  const float* rmask = rotation_mask ? rotation_mask : e->ones;
  build_theta_kernel<<<elem_blocks(N * 105), 256, 0, st>>>(N, global_rotation, joint_rotations, gmask, rmask, e->theta);
  temporal_kernel<<<1, 128, 0, st>>>(N, w_temp, e->theta, trans, losses, e->dtheta, g_trans ? g_trans : e->dtr_direct);
  split_theta_grad_kernel<<<elem_blocks(N * 105), 256, 0, st>>>(N, e->dtheta, gmask, rmask, g_global_rotation, g_joint_rotations);
  LAUNCH_OK("temporal kernels");
  return 0;
}

namespace smalfit {
// the ranges of `o` packed for the segment kernels, checked: every launch of them (eager, graph node) goes through here
static int packed_adam_segments(const smalfit_adam_args* o, AdamSegments& sg) {
  const char* why = pack_adam_segments(o, sg);
  return why ? fail(why) : 0;
}

// optimizer.step() with the hyperparameters of `o` on the packed ranges at the 1-based step t; fresh: the moments are
// taken as zero instead of being read
static int launch_adam_segments(hipStream_t st, const AdamSegments& sg, const smalfit_adam_args* o, int t, bool fresh) {
  const int total = sg.off[sg.nseg];
  if (total == 0) return 0;
  float step_size, bc2_sqrt;
  adam_bias_terms(o->lr, o->beta1, o->beta2, t, step_size, bc2_sqrt);
  adam_segments_kernel<<<elem_blocks(total), 256, 0, st>>>(sg, o->param, o->grad, o->exp_avg, o->exp_avg_sq, step_size,
                                                           o->beta1, o->beta2, o->eps, bc2_sqrt, fresh ? 1 : 0);
  LAUNCH_OK("adam_segments_kernel");
  return 0;
}

// the next step of the optimiser `o` describes: t = o->step + 1, and the first step of a stage does not read the moments
static int launch_adam_next_step(hipStream_t st, const smalfit_adam_args* o) {
  AdamSegments sg;
  if (packed_adam_segments(o, sg)) return 1;
  return launch_adam_segments(st, sg, o, o->step + 1, o->step == 0);
}
}  // namespace smalfit

int smalfit_adam_segments(void* stream, const smalfit_adam_args* o) {
  if (refused("smalfit_adam_segments", null_argument_refusal(o != nullptr))) return 1;
  if (refused("smalfit_adam_segments", step_refusal(o->step))) return 1;
  return launch_adam_next_step((hipStream_t)stream, o);
}

int smalfit_engine_set_graph(smalfit_engine* e, int enable) {
  if (refused("smalfit_engine_set_graph", null_argument_refusal(e != nullptr))) return 1;
  e->use_graph = enable != 0;
  if (!e->use_graph && e->graph_exec) { (void)hipGraphExecDestroy(e->graph_exec); e->graph_exec = nullptr; e->graph_key.clear(); }
  return 0;
}

namespace smalfit {
static int launch_adam_graph_node(smalfit_engine* e, hipStream_t st, const AdamSegments& sg, const smalfit_adam_args* o) {
  const int total = sg.off[sg.nseg];
  if (total == 0) return 0;
  adam_segments_graph_kernel<<<elem_blocks(total), 256, 0, st>>>(sg, o->param, o->grad, o->exp_avg, o->exp_avg_sq, e->step_counter,
                                                                 o->lr, o->beta1, o->beta2, o->eps);
  LAUNCH_OK("adam_segments_graph_kernel");
  return 0;
}

// RunLoop::Graph: one iteration (tick, the evaluation's kernels, Adam) captured once per (arguments, stream) and replayed
static int run_graph_replay(smalfit_engine* e, hipStream_t st, const smalfit_fit_args* a, const smalfit_adam_args* o,
                            const AdamSegments& sg, int iterations) {
  smalfit_adam_args okey = *o;
  okey.step = 0;
  // (the engine's configuration is baked into the captured launches too: prior dimensions, limit switch, probes)
  const unsigned cfg[2] = {e->config_epoch, (unsigned)g_dbg};
  std::vector<unsigned char> key(sizeof(*a) + sizeof(okey) + sizeof(st) + sizeof(cfg));
  std::memcpy(key.data(), a, sizeof(*a));
  std::memcpy(key.data() + sizeof(*a), &okey, sizeof(okey));
  std::memcpy(key.data() + sizeof(*a) + sizeof(okey), &st, sizeof(st));
  std::memcpy(key.data() + sizeof(*a) + sizeof(okey) + sizeof(st), cfg, sizeof(cfg));
  if (!e->graph_exec || key != e->graph_key) {
    if (e->graph_exec) { (void)hipGraphExecDestroy(e->graph_exec); e->graph_exec = nullptr; }
    hipGraph_t graph = nullptr;
    HIP_OK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    tick_kernel<<<1, 1, 0, st>>>(e->step_counter);
    int rc = smalfit_fit_eval(e, st, a);
    if (!rc) rc = launch_adam_graph_node(e, st, sg, o);
    const hipError_t ce = hipStreamEndCapture(st, &graph);
    if (rc) { if (graph) (void)hipGraphDestroy(graph); return 1; }
    if (ce != hipSuccess) return fail(std::string("hipStreamEndCapture: ") + hipGetErrorString(ce));
    const hipError_t ie = hipGraphInstantiate(&e->graph_exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ie != hipSuccess) { e->graph_exec = nullptr; return fail(std::string("hipGraphInstantiate: ") + hipGetErrorString(ie)); }
    e->graph_key = key;
  }
  set_counter_kernel<<<1, 1, 0, st>>>(e->step_counter, o->step);
  LAUNCH_OK("set_counter_kernel");
  for (int it = 0; it < iterations; ++it) HIP_OK(hipGraphLaunch(e->graph_exec, st));
  return 0;
}

// the optimiser step iteration `it` leaves to the head launch of iteration it + 1: the assembly `g` of its gradients, Adam at
// step o->step + it + 1.  Per-frame tensors are stepped in place; the shared ones follow shared_route(it, iterations)
static void pend_step(smalfit_engine* e, const smalfit_fit_args* a, const smalfit_adam_args* o, const FoldPlan& plan,
                      const AssembleArgs& g, int it, int iterations, PendingStep& ps) {
  std::memset(&ps, 0, sizeof(ps));
  ps.g = g;
  const int t = o->step + it + 1;
  adam_bias_terms(o->lr, o->beta1, o->beta2, t, ps.step_size, ps.bc2_sqrt);
  ps.b1 = o->beta1; ps.b2 = o->beta2; ps.eps = o->eps; ps.fresh = t == 1 ? 1 : 0;
  PendingTensor* pt[5] = {&ps.betas, &ps.ls, &ps.grot, &ps.jrot, &ps.trans};
  const float* tensor[5] = {a->betas, a->logscale_mode ? a->log_beta_scales : nullptr, a->global_rotation, a->joint_rotations, a->trans};
  const SharedRoute route = shared_route(it, iterations);
  for (int k = 0; k < 5; ++k) {
    PendingTensor& T = *pt[k];
    if (!plan.train[k]) { T.p_in = T.m_in = T.v_in = tensor[k]; continue; }   // read as it is (unconditional loads: any readable words as moments)
    const int off = plan.off[k];
    T.train = 1;
    T.p_in = T.p = o->param + off; T.m_in = T.m = o->exp_avg + off; T.v_in = T.v = o->exp_avg_sq + off; T.g = o->grad + off;
    if (!tensor_is_shared(k, a->logscale_mode)) continue;
    const int at = k == 0 ? kSharedSlotBetas : kSharedSlotScales;
    if (route.read != kCaller) {
      const float* src = e->shstate + route.read * kSharedSlotFloats + at;
      T.p_in = src; T.m_in = src + 32; T.v_in = src + 64;
    }
    if (route.write != kCaller) {
      float* dst = e->shstate + route.write * kSharedSlotFloats + at;
      T.p = dst; T.m = dst + 32; T.v = dst + 64;
    }
  }
}

// RunLoop::Folded.  Gradient assembly and Adam of every iteration but the last ride in the NEXT iteration's head launch -- its
// frame blocks are the first and only readers of the stepped per-frame parameters, so no fence, counter or tail is needed --
// and the loss terms of those iterations, which no caller can see, are not summed at all.  The last iteration closes with the
// two kernels as ever, so the caller finds parameters, moments, gradients and losses exactly as from the plain chain.
static int run_folded_loop(smalfit_engine* e, hipStream_t st, const smalfit_fit_args* a, const smalfit_adam_args* o,
                           const AdamSegments& sg, const FoldPlan& plan, int iterations) {
  PendingStep ps;
  for (int it = 0; it < iterations; ++it) {
    const bool last = it == iterations - 1;
    EvalFold fold;
    AssembleArgs g;
    fold.pending = it ? &ps : nullptr; fold.prior_slot = prior_slot(it); fold.assemble = last; fold.args_out = &g;
    if (fit_eval_impl(e, st, a, fold)) return 1;
    if (!last) pend_step(e, a, o, plan, g, it, iterations, ps);
  }
  const bool betas_home = plan.train[0], scales_home = plan.train[1] && tensor_is_shared(1, a->logscale_mode);
  const int slot = restore_slot(iterations, betas_home || scales_home);
  if (slot != kCaller) {
    shared_state_restore_kernel<<<1, 64, 0, st>>>(e->shstate + slot * kSharedSlotFloats, o->param, o->exp_avg, o->exp_avg_sq,
                                                 betas_home ? 20 : 0, plan.off[0], scales_home ? 6 : 0, plan.off[1]);
    LAUNCH_OK("shared_state_restore_kernel");
  }
  const int t = o->step + iterations;
  return launch_adam_segments(st, sg, o, t, t == 1);
}

// RunLoop::Plain
static int run_plain_chain(smalfit_engine* e, hipStream_t st, const smalfit_fit_args* a, const smalfit_adam_args* o,
                           const AdamSegments& sg, int iterations) {
  for (int it = 0; it < iterations; ++it) {
    const int t = o->step + it + 1;
    if (smalfit_fit_eval(e, st, a)) return 1;
    if (launch_adam_segments(st, sg, o, t, t == 1)) return 1;
  }
  return 0;
}
}  // namespace smalfit

int smalfit_fit_run(smalfit_engine* e, void* stream, const smalfit_fit_args* a, const smalfit_adam_args* o, int iterations) {
  if (refused("smalfit_fit_run", null_argument_refusal(e && a && o))) return 1;
  if (refused("smalfit_fit_run", iterations_refusal(iterations))) return 1;
  if (refused("smalfit_fit_run", step_refusal(o->step))) return 1;
  if (refused("smalfit_fit_run", fit_args_size_refusal(a))) return 1;
  if (refused("smalfit_fit_run", fit_model_refusal(e->model->NBall))) return 1;   // (before a capture could begin)
  AdamSegments sg;
  if (packed_adam_segments(o, sg)) return 1;
  hipStream_t st = (hipStream_t)stream;
  if (refused("smalfit_fit_run", graph_subject_refusal(e->use_graph, a))) return 1;
  const FoldPlan plan = plan_fold(a, o, sg);
  switch (run_loop(e->use_graph, e->prof_on, iterations, st != nullptr, plan.accepted())) {
    case RunLoop::Graph: return run_graph_replay(e, st, a, o, sg, iterations);
    case RunLoop::Folded: return run_folded_loop(e, st, a, o, sg, plan, iterations);
    case RunLoop::Plain: break;
  }
  return run_plain_chain(e, st, a, o, sg, iterations);
}

int smalfit_shard_record(void* stream, int num_shared, const float* shared_grad, int num_frames, const float* global_rotation,
                         const float* joint_rotations, const float* trans, const float* global_mask,
                         const float* rotation_mask, float* record) {
  if (refused("smalfit_shard_record", shard_record_refusal(num_shared, num_frames, shared_grad && global_rotation && joint_rotations && trans &&
                                                                                         global_mask && rotation_mask && record))) return 1;
  shard_record_kernel<<<elem_blocks(num_shared + 216), 256, 0, (hipStream_t)stream>>>(num_shared, shared_grad, num_frames, global_rotation,
                                                                                    joint_rotations, trans, global_mask, rotation_mask, record);
  LAUNCH_OK("shard_record_kernel");
  return 0;
}

int smalfit_shard_local_step(smalfit_engine* e, void* stream, const smalfit_fit_args* a, const smalfit_adam_args* o, int num_shared,
                             const float* shared_grad, float* record) {
  if (refused("smalfit_shard_local_step", null_argument_refusal(e && a && o && record && shared_grad))) return 1;
  if (refused("smalfit_shard_local_step", step_refusal(o->step))) return 1;
  if (refused("smalfit_shard_local_step", shard_subject_refusal(a))) return 1;
  if (smalfit_fit_eval(e, stream, a)) return 1;
  if (launch_adam_next_step((hipStream_t)stream, o)) return 1;
  return smalfit_shard_record(stream, num_shared, shared_grad, a->num_frames, a->global_rotation, a->joint_rotations, a->trans,
                              a->global_mask ? a->global_mask : e->ones, a->rotation_mask ? a->rotation_mask : e->ones, record);
}

int smalfit_shard_reduce_step(void* stream, int world_size, int record_stride, const float* gathered, int num_shared,
                              int num_trainable, const smalfit_adam_args* o) {
  if (refused("smalfit_shard_reduce_step", shard_reduce_refusal(world_size, record_stride, gathered != nullptr, num_shared, num_trainable, o))) return 1;
  float step_size, bc2_sqrt;
  adam_bias_terms(o->lr, o->beta1, o->beta2, o->step + 1, step_size, bc2_sqrt);
  shard_reduce_adam_kernel<<<elem_blocks(num_shared), 256, 0, (hipStream_t)stream>>>(world_size, record_stride, gathered, num_shared, num_trainable,
                                                                                   o->param, o->grad, o->exp_avg, o->exp_avg_sq, step_size,
                                                                                   o->beta1, o->beta2, o->eps, bc2_sqrt, o->step == 0 ? 1 : 0);
  LAUNCH_OK("shard_reduce_adam_kernel");
  return 0;
}

int smalfit_rccl_allgather(void* ctx, const float* send, float* recv, int count, void* stream) {
  const smalfit_rccl_ctx* c = (const smalfit_rccl_ctx*)ctx;
  if (!c || !c->comm || !c->nccl_all_gather) return refused("smalfit_rccl_allgather", "no communicator / ncclAllGather address");
  typedef int (*all_gather_t)(const void*, void*, size_t, int, void*, hipStream_t);
  const int kNcclFloat32 = 7;                                   // ncclDataType_t: ncclFloat32
  const int rc = ((all_gather_t)c->nccl_all_gather)(send, recv, (size_t)count, kNcclFloat32, c->comm, (hipStream_t)stream);
  if (rc != 0) return fail("smalfit_rccl_allgather: ncclAllGather returned " + std::to_string(rc));
  return 0;
}

int smalfit_shard_run(smalfit_engine* e, void* stream, const smalfit_fit_args* a, const smalfit_adam_args* ol,
                      const smalfit_adam_args* os, const smalfit_shard_args* sh, int iterations) {
  if (refused("smalfit_shard_run", null_argument_refusal(e && a && ol && os && sh))) return 1;
  if (refused("smalfit_shard_run", shard_run_refusal(a, ol, os, sh, iterations))) return 1;
  const int stride = sh->num_shared + 216;
  for (int it = 0; it < iterations; ++it) {
    smalfit_adam_args l = *ol, s = *os;
    l.step = s.step = ol->step + it;
    if (smalfit_shard_local_step(e, stream, a, &l, sh->num_shared, sh->shared_grad, sh->record)) return 1;
    if (sh->allgather(sh->allgather_ctx, sh->record, sh->gathered, stride, stream)) {
      if (g_err.empty() || g_err.find("allgather") == std::string::npos) return fail("smalfit_shard_run: the caller's all-gather reported an error");
      return 1;
    }
    if (smalfit_shard_reduce_step(stream, sh->world_size, stride, sh->gathered, sh->num_shared, sh->num_trainable_shared, &s)) return 1;
  }
  return 0;
}

int smalfit_adam_step(void* stream, int count, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                      float lr, float beta1, float beta2, float eps, int t) {
  if (refused("smalfit_adam_step", adam_step_refusal(count, param && grad && exp_avg && exp_avg_sq, t))) return 1;
  // one range [0, count); the moments are always read, also at t = 1
  smalfit_adam_args o{};
  o.param = param; o.grad = const_cast<float*>(grad); o.exp_avg = exp_avg; o.exp_avg_sq = exp_avg_sq;
  o.num_segments = 1; o.seg_begin[0] = 0; o.seg_end[0] = count;
  o.lr = lr; o.beta1 = beta1; o.beta2 = beta2; o.eps = eps;
  AdamSegments sg;
  if (packed_adam_segments(&o, sg)) return 1;
  return launch_adam_segments((hipStream_t)stream, sg, &o, t, false);
}

}  // extern "C"
