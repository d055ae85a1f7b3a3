// soft-silhouette rasteriser, forward and backward (K5) -- part of smalfit_kernels.hip (included inside namespace smalfit; not a translation unit of its own)

// ------------------------------------------------------------------------------------------------
// K5: soft-silhouette rasteriser  (DESIGN.md section 4 has the measurements behind each choice)
//
// pytorch3d keeps, per pixel, only the faces_per_pixel = 100 candidates nearest in depth; with the
// reference's head-on initial pose a pixel sees hundreds of candidates, so the truncation is first-class.
// Measured on MI355X while designing this (64 frames, 256^2): evaluating every face of a tile for all the tile's
// pixels does 4.6x more lane evaluations than letting each face walk its own blur-expanded pixel box; one global
// atomic per candidate is capped at ~50 G/s (memory-side on this multi-XCD part); per-pixel candidate lists in HBM
// mean 35-50 M scattered 8-byte stores.  Hence:
//   sweep      block = 32 consecutive faces.  Prologue: per-face pixel box + the face's 64-byte record (edge vectors, reciprocals,
//              depth plane) from the projected vertices, the union box of every 8 consecutive faces, the frame's reference
//              depth; riders: the frame's active pixel region.  Faces are Morton-ordered once at model creation, so
//              consecutive faces are screen-space neighbours in any pose.  (Until it was folded in: a launch of its own, face_bbox.)
//              Then 16 lanes per face walking the box row-major.  Per pixel two cached
//              depth bounds lo <= hi: candidates <= lo go into ONE packed 64-bit integer per pixel
//              (count << 50 | sum of -log2(1 - p) in 2^-24 fixed point; 32x32-pixel LDS window, one global atomic per
//              touched pixel), candidates in (lo, hi] into the pixel's band list (<= 64 entries, staged per wave),
//              candidates beyond hi are dropped unevaluated.  Integer adds commute: order-independent results.
//   resolve    thread per pixel of the active region: with c = #{<= lo}, b = #band the K nearest are proved from
//              counts (c <= K <= c + b) or the pixel is queued.
//   band       half-wave per pixel: ranks the band entries, adds the K - c nearest, re-centres / narrows the bounds.
//   select     wave per queued pixel: exact K nearest from scratch (union boxes -> face boxes -> evaluation ->
//              candidates in LDS in face order -> K-th depth by linear-histogram refinement + exact ranks), new
//              bounds sized to the current miss rate.  The cache is only ever a verified shortcut.
//   bwd        face-parallel gather with the same box walk; the depth of the farthest included candidate is stored
//              with the adjoint seed so that it applies exactly the forward's truncation.
// ------------------------------------------------------------------------------------------------
// ablation probes of the selection kernel (stop a queued pixel after a given phase; tools/raster_probe.py): compiled
// out of the product, present only in developer builds made with tools/build_variant.sh NAME -DSMALFIT_DEV_PROBES
#ifdef SMALFIT_DEV_PROBES
#define SMALFIT_PROBE(flags, bit) (((flags) & (bit)) != 0)
#else
#define SMALFIT_PROBE(flags, bit) false
#endif

// work statistics of the two face sweeps (developer builds only: tools/build_variant.sh NAME -DSMALFIT_DEV_PROBES -DSMALFIT_WORK_STATS;
// read and cleared with smalfit_debug_work_stats, tools/sweep_counters.py)
#ifdef SMALFIT_WORK_STATS
__device__ unsigned long long g_work[32];
__device__ float g_probe_seed_scale;   // |adjoint seed| of a pixel with alpha = 1 (written by raster_resolve_kernel)
#define SMALFIT_WORK(...) __VA_ARGS__
__device__ __forceinline__ void work_add(int slot, unsigned long long v) {
  // wave-wide sum, one atomic per wave (called with the wave converged)
  unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = ((unsigned long long)__shfl_xor(hi, o, 64) << 32) | __shfl_xor(lo, o, 64);
    const unsigned long long s = (((unsigned long long)hi << 32) | lo) + w;
    lo = (unsigned)s; hi = (unsigned)(s >> 32);
  }
  if ((threadIdx.x & 63) == 0) atomicAdd(&g_work[slot], ((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
#else
#define SMALFIT_WORK(...)
#endif

// per-face candidate lists handed from the forward sweep to the backward gather: the pixels of the face's box at which the face
// passed the forward's tests (depth not beyond the pixel's cached far bound, then inside / within the blur radius).  The backward
// gather evaluates those pairs only (a third of the box on the benchmark).  Two formats share a face's 128 bytes:
//   * a LIST of box-relative pixel indices (u8), appended in LDS through the face's own counter while the sweep walks the box and
//     copied out once: boxes of <= 256 pixels with <= kListLds candidates.  The backward walks it 16 entries per round, every lane busy.
//   * 16 MASKS (round 6, kMaskList).  Both kernels walk a box row-major with 16 lanes, lane s taking the pixels q = s, s + 16, ...:
//     bit r of the lane's 64-bit word says "candidate at pixel 16 r + s".  The sweep collects the word in registers (the round's bit is
//     wave-uniform: one scalar shift per round, two vector ORs per candidate), so it costs nothing to have, never overflows, and covers
//     boxes of up to 64 rounds = 1024 pixels.  The backward visits each lane's set bits: its lanes are unevenly loaded on small
//     faces (masks for every face: 86 instead of 76 us on the headline scene), which matters little on the long walks of large ones.
//     Until round 5 such faces walked their whole box: on a crop-filling animal the 10 % of the faces with more than 256 pixels (24 %
//     of the box pixels) plus the 9 % whose lists overflowed.
//   The four faces of a sweep wave are the four faces of a backward wave; the sweep picks ONE format for all four (lists when all
//   four qualify), so that a backward wave runs one kind of loop instead of one after the other.
//   * kNoList: "evaluate the whole box" -- more than 1024 pixels, or the exact selection found one of the K nearest beyond the old
//     far bound at a pixel of the box.
constexpr int kListCap = 128;             // bytes per face in HBM: <= 128 indices, or 16 lanes x one 64-bit mask
// list entries per face staged in the sweep's LDS (longer lists go out as masks).  With the 36 x 36 window the kernel's LDS is
// 19 984 bytes: eight workgroups per CU, like its 63 registers (checked in raster_sweep_kernel)
constexpr int kListLds = 128;
static_assert(kListLds <= kListCap && kListLds % 8 == 0, "lists are copied out in 8-byte pieces");
constexpr int kMaskRounds = 64;           // rounds (of 16 pixels) a mask covers
constexpr unsigned char kMaskList = 254;  // pcount: the face's 128 bytes hold the 16 masks
constexpr unsigned char kNoList = 255;    // pcount: walk the whole box
constexpr float kBoxSlack = 1.0f / 64.0f; // pixels added to each side of a face's pixel box (rounding guard)
// (kRectFaces, kSelGroups, kSweepFaces and the other constants the launches are sized by: smalfit_plan.h)
constexpr int kTicketBase = 64, kTicketStride = 16;   // in the queue-counter array: one counter per 64-byte line
constexpr int kQCountInts = kTicketBase + 8 * kSelGroups * kTicketStride;
// LDS accumulator window edge (pixels); outside: global atomics.  Round 6 (was 32): see the zeroing loop of the sweep; 40 with 64-entry
// lists measured +4.1 % on the crop-filling scene but -0.7 % on the headline one, 36 with full lists +3.1 % / -0.3 %
// (profiles/r6_ab_lists_window.txt)
constexpr int kAccWin = 36;
constexpr int kCountShift = 50;
constexpr float kLogFix = 16777216.0f;    // 2^24
constexpr int kBandCap = 64;              // per-pixel list of candidates between the two cached depth bounds
// (round 5: 24 / 40 / 12 instead of round 3's 30 / 50 / 16 -- with the sweep at its issue ceiling a band entry appended costs more than a
// miss re-selected: +0.2 % / +0.6 % / +1.3 % on the 195-step run / the crop-filling fit / the 20-step window; 20 / 32 / 10 and 16 / 28 / 8
// measured the same within noise, 36 / 60 / 20 worse: profiles/r5_ab_band_fill.txt.  Round 3: 60 left 4 entries of headroom below
// kBandCap; 50 / half-width 4 measured best then, profiles/r3_ab_band_policy_*.txt)
constexpr int kBandFill = 24;             // the select kernel sizes the band to hold at most this many entries ...
constexpr int kBandFillWide = 40, kBandFillNarrow = 12;   // ... or these, by miss rate
constexpr int kBandStage = 64;            // band entries staged per wave in the sweep before a batched append
constexpr float kBandHalf = 4.0f;         // initial half-width of the band, in mean depth gaps of the K nearest

// target silhouettes: float32 (M,S,S), or bytes b = 255 t (the masks the reference's loaders read are 8-bit images,
// data_loader.py:43: a quarter of the target traffic).  b / 255 is a correctly rounded division: the value a float32
// tensor holding b / 255 carries, bit for bit (tests/test_gpu_fullsize.py).
struct SilTarget {
  const float* f;
  const unsigned char* b;
  __host__ __device__ explicit operator bool() const { return f != nullptr || b != nullptr; }
  __device__ __forceinline__ float operator[](size_t i) const { return b ? (float)b[i] / 255.0f : f[i]; }
};

// Frame-to-XCD affinity of the per-frame rasteriser kernels.  Workgroups are dealt to the 8 XCDs round-robin by their
// linear id, and each XCD has its own L2: with a (blocks, frames) grid the blocks of one frame land on all eight, so the
// face records one kernel writes are read back through HBM by the next (a 2-3 us dependent load at the head of every
// block).  These kernels use a 1-D grid instead and give frame n to XCD n % 8 in all of them: producer and consumer
// share an L2.  Only speed depends on the placement (HIP promises none); results never do.
//   grid.x = xcd_grid(blocks_per_frame, M) of smalfit_plan.h;   xcd_block(blocks_per_frame, n, bx) -> frame n (may be >= M: exit), block bx
__device__ __forceinline__ void xcd_block_of(int b /*linear workgroup id; b % 8 must be the workgroup's blockIdx.x % 8*/, int blocks_per_frame, int& n, int& bx) {
  const XcdBlock x = xcd_block_at(b, blocks_per_frame);
  n = x.n;
  bx = x.bx;
}
__device__ __forceinline__ void xcd_block(int blocks_per_frame, int& n, int& bx) { xcd_block_of((int)blockIdx.x, blocks_per_frame, n, bx); }

__device__ __forceinline__ unsigned orderable(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float from_orderable(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ float wave_prod(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v *= __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ bool box_contains(int2 b, int x, int y) {
  return (b.x & 0xffff) <= x && x <= (b.x >> 16) && (b.y & 0xffff) <= y && y <= (b.y >> 16);
}
__device__ __forceinline__ unsigned long long pack_candidate(float d) {
  // count in the top bits, -log2(1 - p) = -log2 sigmoid(d / sigma) in [0, 256) as 2^-24 fixed point.
  // v_exp_f32 / v_log_f32 directly (1 ulp; the argument ranges need no denormal handling: 2^-|x| only matters while
  // it is > 2^-24 next to 1).  One rounded term is off by <= 6e-8 relative in alpha, like a rounded multiplication.
  const float x2 = d * (1.4426950408889634f / kSigma);
  const float t = __builtin_amdgcn_exp2f(-fabsf(x2));
  const float f = fminf(__builtin_amdgcn_logf(1.0f + t) - fminf(x2, 0.0f), 255.99998f);
  // rounded to the NEAREST 2^-24 (round 6; the conversion truncates, so half a unit is added by the multiply-add that scales -- same
  // instruction count): truncation made every term half a unit too small on average, i.e. alpha too large by the same factor at every
  // pixel -- 2^(2^-25 c) - 1 ~ 2e-8 per candidate, 1-2e-6 with the 50-100 candidates of a pixel: a bias of one sign in every adjoint
  // seed and in the silhouette loss (the loss term was 7e-7 ... 3.6e-6 off the float64 oracle where a float32 torch evaluation is
  // 1e-7 ... 3e-7 off; the shared-shape gradient, which adds the frames' seeds up, 3-5 x a float32 evaluation's deviation)
  return (1ull << kCountShift) | (unsigned long long)(unsigned)fmaf(f, kLogFix, 0.5f);
}

// A finished pixel: its silhouette value, |sil - target| and the adjoint seed of the squared distances,
// gx = -wn sgn(sil - target) alpha / sigma with wn = w_sil / (Bn S S) formed by the caller.  Resolve, the band ranking and the
// exact selection all finish their pixels here; the loss bookkeeping, the stores and the depth bounds are each caller's own.
struct PixelSeed { float sil, adiff, gx; };
__device__ __forceinline__ PixelSeed pixel_no_target(float alpha) { return {1.0f - alpha, 0.f, 0.f}; }
__device__ __forceinline__ PixelSeed pixel_seed(float alpha, float ts, float wn) {
  PixelSeed p = pixel_no_target(alpha);
  const float diff = p.sil - ts;
  p.adiff = fabsf(diff);
  const float sgn = (diff > 0.f) ? 1.0f : ((diff < 0.f) ? -1.0f : 0.0f);
  p.gx = -wn * sgn * alpha * (1.0f / kSigma);
  return p;
}

// p = sigmoid(-d / sigma) with the hardware exp2 / rcp (backward sweep)
__device__ __forceinline__ float prob_fast(float d) {
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(d * (1.4426950408889634f / kSigma)));
}

// The face record kernels share: raster_sweep_kernel's prologue evaluates make_face_rec ONCE per face and evaluation, keeps the
// 16 floats the per-pixel maths reads (64 bytes, one cache line) in LDS for its own pixel loop and stores them; selection and
// backward load them instead of rebuilding them from the projected vertices (four reciprocals and ~40 instructions -- per
// covering face and PIXEL in the selection, per lane at the head of every short-lived wave of the backward gather).  One
// definition also means the kernels cannot disagree on a face's edge constants.  The degenerate-edge offsets t0 are implied:
// il == 0 exactly when the edge is degenerate.
constexpr int kRecVecs = 4;               // float4 per face record
__device__ __forceinline__ void store_face_rec(float4* __restrict__ o, const FaceRec& r) {
  o[0] = make_float4(r.ax, r.ay, r.e1x, r.e1y);
  o[1] = make_float4(r.e2x, r.e2y, r.e3x, r.e3y);
  o[2] = make_float4(r.il1, r.il2, r.il3, r.area);
  o[3] = make_float4(r.inv_den, r.pz0, r.gzx, r.gzy);
}
__device__ __forceinline__ void unpack_face_rec(const float4 a, const float4 b, const float4 c, const float4 d, FaceRec& r) {
  r.ax = a.x; r.ay = a.y; r.e1x = a.z; r.e1y = a.w;
  r.e2x = b.x; r.e2y = b.y; r.e3x = b.z; r.e3y = b.w;
  r.il1 = c.x; r.il2 = c.y; r.il3 = c.z; r.area = c.w;
  r.t01 = (c.x == 0.0f) ? 1.0f : 0.0f; r.t02 = (c.y == 0.0f) ? 1.0f : 0.0f; r.t03 = (c.z == 0.0f) ? 1.0f : 0.0f;
  r.inv_den = d.x; r.pz0 = d.y; r.gzx = d.z; r.gzy = d.w; r.pad = 0.0f;
}
__device__ __forceinline__ void load_face_rec(const float4* __restrict__ fr, FaceRec& r) {
  const float4 a = fr[0], b = fr[1], c = fr[2], d = fr[3];
  unpack_face_rec(a, b, c, d, r);
}

// 5a: what the sweep's workgroups form before they walk pixels (until the box launch was folded into the sweep, a kernel of its
// own that handed the sweep 64 bytes of record and 8 of box per face through HBM): the frame's reference depth, a face's
// conservative pixel box, and -- one rider workgroup per frame -- the frame's active pixel region.

// reference depth of frame n (mean over 64 spread vertices; pz: the frame's plane of view-space depths), called by a whole wave.
// The rasteriser orders candidates by pz - zc, which is the same order (the subtraction is exact for depths within a factor
// two) but keeps the cached per-pixel bounds valid when the whole animal moves along the view axis.
__device__ __forceinline__ float frame_ref_depth(const float* __restrict__ pz, int V, int lane) {
  return wave_sum(pz[(int)(((long long)lane * V) >> 6)]) * (1.0f / 64.0f);
}

// conservative pixel box of a face with projected corners a, b, c that make_face_rec accepted (`ok`): c0 | c1 << 16, r0 | r1 << 16;
// c0 = 1 > c1 = 0 when nothing of it is on screen
__device__ __forceinline__ int2 face_pixel_box(bool ok, float ax, float ay, float bx, float by, float cx, float cy, int S) {
  int2 box = make_int2(1, 1);
  if (ok) {
    const float xlo = fminf(ax, fminf(bx, cx)) - kBlurSqrt, xhi = fmaxf(ax, fmaxf(bx, cx)) + kBlurSqrt;
    const float ylo = fminf(ay, fminf(by, cy)) - kBlurSqrt, yhi = fmaxf(ay, fmaxf(by, cy)) + kBlurSqrt;
    // pixel centre x_p = 1 - (2c+1)/S  =>  c = ((1 - x_p) S - 1) / 2
    const float fs = (float)S;
    // Exactly the pixels whose centres lie inside the expanded bounding box (every candidate's does: inside the
    // triangle, or closer than sqrt(blur) to it), widened by 1/64 pixel -- two orders of magnitude more than the
    // rounding of these bounds at any image size the engine accepts.  (A floor / ceil pair would add a ring of up to
    // one pixel either side: +35 % pixels on the ~9-pixel boxes of the benchmark.)
    float c0 = ceilf(((1.0f - xhi) * fs - 1.0f) * 0.5f - kBoxSlack);
    float c1 = floorf(((1.0f - xlo) * fs - 1.0f) * 0.5f + kBoxSlack);
    float r0 = ceilf(((1.0f - yhi) * fs - 1.0f) * 0.5f - kBoxSlack);
    float r1 = floorf(((1.0f - ylo) * fs - 1.0f) * 0.5f + kBoxSlack);
    c0 = fminf(fmaxf(c0, 0.f), fs - 1.f); c1 = fminf(fmaxf(c1, -1.f), fs - 1.f);
    r0 = fminf(fmaxf(r0, 0.f), fs - 1.f); r1 = fminf(fmaxf(r1, -1.f), fs - 1.f);
    const bool finite = (xlo == xlo) && (xhi == xhi) && (ylo == ylo) && (yhi == yhi);
    const bool onscreen = finite && (xhi >= -1.0f) && (xlo <= 1.0f) && (yhi >= -1.0f) && (ylo <= 1.0f) &&
                          (c1 >= c0) && (r1 >= r0);
    if (onscreen) box = make_int2((int)c0 | ((int)c1 << 16), (int)r0 | ((int)r1 << 16));
  }
  return box;
}

// One rider workgroup per frame, first in the sweep's grid: the frame's active pixel region, and (frame 0's) the reset of the
// queue counters.  Both are first read by the resolve launch.  (Until round 3 this was extra work of the frame's first face
// workgroup, which made that workgroup the kernel's last to finish.)  Called by every thread of a 256-thread workgroup.
__device__ __forceinline__ void frame_region_block(const ModelDev& m, int S, const float* __restrict__ proj, int* __restrict__ frect,
                                                   int* __restrict__ qcount, int n, float (*rr)[4] /*4 x 4 floats of LDS*/) {
  const int Vp = m.Vp;
  if (n == 0) {
    if (threadIdx.x < 3) qcount[threadIdx.x] = 0;
    for (int i = threadIdx.x; i < 8 * kSelGroups; i += 256) qcount[kTicketBase + i * kTicketStride] = 0;   // the selection's ticket counters
  }
  const float* px = proj + (size_t)n * 3 * Vp;
  // the frame's active region: pixel box of ALL projected vertices, blur-expanded -- a superset of every face box, so
  // pixels outside it have no candidate at all (no atomics).
  float xlo = 3.0e38f, xhi = -3.0e38f, ylo = 3.0e38f, yhi = -3.0e38f;
#pragma unroll 8
  for (int v = threadIdx.x; v < m.V; v += 256) {
    const float x = px[v], y = px[Vp + v];
    xlo = fminf(xlo, x); xhi = fmaxf(xhi, x); ylo = fminf(ylo, y); yhi = fmaxf(yhi, y);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    xlo = fminf(xlo, __shfl_xor(xlo, o, 64)); xhi = fmaxf(xhi, __shfl_xor(xhi, o, 64));
    ylo = fminf(ylo, __shfl_xor(ylo, o, 64)); yhi = fmaxf(yhi, __shfl_xor(yhi, o, 64));
  }
  if ((threadIdx.x & 63) == 0) { float* q = rr[threadIdx.x >> 6]; q[0] = xlo; q[1] = xhi; q[2] = ylo; q[3] = yhi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) { xlo = fminf(xlo, rr[w][0]); xhi = fmaxf(xhi, rr[w][1]); ylo = fminf(ylo, rr[w][2]); yhi = fmaxf(yhi, rr[w][3]); }
    xlo -= kBlurSqrt; xhi += kBlurSqrt; ylo -= kBlurSqrt; yhi += kBlurSqrt;
    const float fs = (float)S;
    const float c0 = fmaxf(floorf(((1.0f - xhi) * fs - 1.0f) * 0.5f), 0.f), c1 = fminf(ceilf(((1.0f - xlo) * fs - 1.0f) * 0.5f), fs - 1.f);
    const float r0 = fmaxf(floorf(((1.0f - yhi) * fs - 1.0f) * 0.5f), 0.f), r1 = fminf(ceilf(((1.0f - ylo) * fs - 1.0f) * 0.5f), fs - 1.f);
    int4 o = make_int4(0, 0, 0, 0);              // (S - c0, c1 + 1, S - r0, r1 + 1); zeros = empty
    if (c0 <= c1 && r0 <= r1) o = make_int4(S - (int)c0, (int)c1 + 1, S - (int)r0, (int)r1 + 1);
    *reinterpret_cast<int4*>(frect + n * 4) = o;
  }
}

// 5b: sweep.  Each pixel carries two cached depth bounds lo <= hi from the last exact selection (zband; +inf
// while the pixel never had more than K candidates).  Candidates not farther than lo are accumulated into ONE packed
// integer (count << 50 | log sum); candidates in (lo, hi] are appended to the pixel's short band list; farther ones
// are dropped.  raster_resolve_kernel proves from the counts that the K nearest are {<= lo} + the nearest few of the
// band, or sends the pixel to the exact selection.
// The launch also forms what it sweeps (until then face_bbox_kernel's launch, 14 us for 36 MB that this kernel read straight back):
// grid = sweep_launch_grid: [frame riders: frame_region_block] [sweep blocks] [joint riders, only with joints_out: joints_block --
// independent of the rasteriser, latency-bound, and otherwise a launch of its own; short, and behind the sweep blocks because in
// front of the face workgroups of the box launch they measured 0.4 % slower]; sweep_block_at of smalfit_plan.h deals the roles.
__global__ void __launch_bounds__(256, 1)
raster_sweep_kernel(ModelDev m, int M, int S, const float* __restrict__ proj, float4* __restrict__ frec /*[M][F][kRecVecs]: see store_face_rec*/,
                    int2* __restrict__ fbox /*[M][F]*/, int4* __restrict__ brect /*[M][ceil(F/8)]*/, float* __restrict__ zc /*[M]*/,
                    int* __restrict__ frect /*[M][4]: S - x0, x1 + 1, S - y0, y1 + 1 of the active region; 0 = empty*/,
                    int* __restrict__ qcount /*[0..2]: select / band queue lengths, pixels resolve sent to select; [8..15]: the selection's tickets; reset here*/,
                    const float* __restrict__ jverts, float* __restrict__ joints_out /*[M][41][3] or null*/,
                    const float2* __restrict__ zband,
                    unsigned long long* __restrict__ gacc /*[M][S*S]*/, unsigned* __restrict__ bcnt /*[M][S*S]*/,
                    float2* __restrict__ blist /*[M][S*S][kBandCap]*/, unsigned char* __restrict__ plist /*[M][F][kListCap]*/,
                    unsigned char* __restrict__ pcount /*[M][F]*/) {
  // Prologue: TWO dependent trips to memory, by one wave, and ONE barrier.  Threads 0..31 form the block's 32 face records and
  // boxes from the frame's projected vertices (46 KB, resident in the L2 of the frame's XCD): the face's three indices, then
  // its nine coordinates, make_face_rec, face_pixel_box, all into LDS where the pixel loop reads them; the union boxes by
  // sub-wave shuffles.  The second wave forms the frame's reference depth from static addresses (the same trip as the indices);
  // waves 1..3 zero the accumulator window meanwhile.  Behind the barrier the records leave for the selection and the backward
  // gather as ONE contiguous 2 KB run (128 threads x 16 bytes), the boxes as 256 bytes: stores that drain under the pixel loop.
  // (Round 4 set the shape: one barrier, every load issued before the window is zeroed; each further barrier costs the launch
  // ~10 us over its 15.5 k workgroups -- profiles/r4_ab_experiments.txt.)
  static_assert(kSweepFaces % kRectFaces == 0, "a sweep block is a whole number of union boxes");
  __shared__ __attribute__((aligned(16))) float4 raw[kSweepFaces][kRecVecs];
  __shared__ int2 boxes[kSweepFaces];
  __shared__ unsigned long long acc[kAccWin * kAccWin];   // near candidates: count << 50 | log sum
  __shared__ float2 st_e[4][kBandStage];
  __shared__ int st_p[4][kBandStage];
  __shared__ int st_n[4];
  __shared__ __attribute__((aligned(8))) unsigned char lsts[kSweepFaces][kListLds];
  __shared__ int lcn[kSweepFaces];
  __shared__ int4 brect_s;                                // the block's rectangle: x0, x1, y0, y1
  __shared__ float zc_s;                                  // the frame's reference depth
  static_assert(sizeof(raw) + sizeof(boxes) + sizeof(acc) + sizeof(st_e) + sizeof(st_p) + sizeof(st_n) + sizeof(lsts) + sizeof(lcn) +
                sizeof(brect_s) + 16 /*zc_s, padded*/ <= 160 * 1024 / 8, "eight sweep workgroups per CU (160 KB of LDS)");
  const int t = threadIdx.x;
  const int F = m.F;
  const SweepBlock role = sweep_block_at((int)blockIdx.x, F, M);
  if (role.role != SweepRole::Faces) {
    // the riders' few floats of LDS alias the accumulator window
    if (role.role == SweepRole::Joint) joints_block(m, jverts, joints_out, role.bx, role.n, reinterpret_cast<float*>(acc));
    else if (role.n < M) frame_region_block(m, S, proj, frect, qcount, role.n, reinterpret_cast<float (*)[4]>(acc));
    return;
  }
  const int n = role.n, bxi = role.bx;
  if (n >= M) return;                                     // a frame of the padding: stores nothing
  const int f0 = bxi * kSweepFaces;
  SMALFIT_WORK(const unsigned long long ws_t0 = __builtin_amdgcn_s_memtime();)
  static_assert(kSweepFaces * kRecVecs <= 128 && kRecVecs == 4 && kSweepFaces <= 32, "faces by threads 0..31; record quarters leave by threads 0..127, boxes by 128..159");
  const float* px = proj + (size_t)n * 3 * m.Vp;
  // (the wave's id through readfirstlane: s_setprio is a scalar instruction and must sit behind a provably uniform branch)
  if ((__builtin_amdgcn_readfirstlane(t) >> 6) == 0) {
    // the block waits at the barrier for this wave's two trips and ~150 instructions, and the SIMD it shares with seven other
    // waves is issue-bound in their pixel loops: it issues first until it is through (+0.4 % of the whole iteration)
    __builtin_amdgcn_s_setprio(3);
    if (t < kSweepFaces) {
      const int Vp = m.Vp;
      const int f = f0 + t;
      int2 box = make_int2(1, 1);                           // c0 = 1 > c1 = 0: empty
      if (f < F) {
        const int i0 = m.faces[f * 3], i1 = m.faces[f * 3 + 1], i2 = m.faces[f * 3 + 2];
        const float ax = px[i0], ay = px[Vp + i0], az = px[2 * Vp + i0];
        const float bx = px[i1], by = px[Vp + i1], bz = px[2 * Vp + i1];
        const float cx = px[i2], cy = px[Vp + i2], cz = px[2 * Vp + i2];
        FaceRec r;
        const bool ok = make_face_rec(ax, ay, az, bx, by, bz, cx, cy, cz, r);
        box = face_pixel_box(ok, ax, ay, bx, by, cx, cy, S);
        store_face_rec(&raw[t][0], r);
      }
      boxes[t] = box;
      lcn[t] = 0;
      // union box of each group of kRectFaces consecutive faces (sub-wave shuffle reduction): the selection's index; then of all
      // the block's faces: its rectangle
      const bool live = (box.x & 0xffff) <= (box.x >> 16);
      int x0 = live ? (box.x & 0xffff) : 0x7fff, x1 = live ? (box.x >> 16) : -1;
      int y0 = live ? (box.y & 0xffff) : 0x7fff, y1 = live ? (box.y >> 16) : -1;
#pragma unroll
      for (int o = kRectFaces / 2; o > 0; o >>= 1) {
        x0 = min(x0, __shfl_xor(x0, o, kRectFaces)); x1 = max(x1, __shfl_xor(x1, o, kRectFaces));
        y0 = min(y0, __shfl_xor(y0, o, kRectFaces)); y1 = max(y1, __shfl_xor(y1, o, kRectFaces));
      }
      if ((t & (kRectFaces - 1)) == 0 && f < F)
        brect[(size_t)n * rect_count(F) + f / kRectFaces] = make_int4(x0, x1, y0, y1);
#pragma unroll
      for (int o = kSweepFaces / 2; o >= kRectFaces; o >>= 1) {
        x0 = min(x0, __shfl_xor(x0, o, kSweepFaces)); x1 = max(x1, __shfl_xor(x1, o, kSweepFaces));
        y0 = min(y0, __shfl_xor(y0, o, kSweepFaces)); y1 = max(y1, __shfl_xor(y1, o, kSweepFaces));
      }
      if (t == 0) brect_s = make_int4(x0, x1, y0, y1);
    }
    __builtin_amdgcn_s_setprio(0);
  } else {
    // every row of the window is zeroed: the rectangle is not known before the barrier (zeroing only the rows it reaches measured
    // as no gain in round 6)
    float zcv = 0.f;
    if (t < 128) zcv = frame_ref_depth(px + 2 * m.Vp, m.V, t - 64);
    for (int i = t - 64; i < kAccWin * kAccWin; i += 192) acc[i] = 0ull;
    if (t == 64) {
      zc_s = zcv;
      if (bxi == 0) zc[n] = zcv;                          // for the selection and the backward gather
    }
    if (t >= 128 && t < 132) st_n[t - 128] = 0;
  }
  SMALFIT_WORK(const unsigned long long ws_t1 = __builtin_amdgcn_s_memtime();)
  __syncthreads();
  SMALFIT_WORK(const unsigned long long ws_t2 = __builtin_amdgcn_s_memtime();)
  int rect[4];                                            // x0, x1, y0, y1 (uniform: scalar registers)
  {
    const int4 b = brect_s;
    rect[0] = __builtin_amdgcn_readfirstlane(b.x); rect[1] = __builtin_amdgcn_readfirstlane(b.y);
    rect[2] = __builtin_amdgcn_readfirstlane(b.z); rect[3] = __builtin_amdgcn_readfirstlane(b.w);
  }
  if (t < kSweepFaces * kRecVecs) {
    if (f0 + (t >> 2) < F) frec[((size_t)n * F + f0) * kRecVecs + t] = raw[t >> 2][t & 3];
  } else if (t < 128 + kSweepFaces && f0 + (t - 128) < F) {
    const int2 bq = boxes[t - 128];
    fbox[(size_t)n * F + f0 + (t - 128)] = bq;
    if ((bq.x & 0xffff) > (bq.x >> 16)) pcount[(size_t)n * F + f0 + (t - 128)] = 0;   // nothing on screen: an empty list (faces with a box: below)
  }
  if (rect[1] < rect[0]) return;                        // no face of this block is on screen
  // The LDS window: kAccWin x kAccWin accumulator cells CENTRED on the block's rectangle (round 4; until then anchored at its corner).
  // It matters when the rectangle does not fit -- 32 faces of a crop-filling animal span ~45 x 40 pixels: anchored at the corner,
  // 28 % of that scene's near pairs fell outside the window, one global atomic each (10.7 M per launch, twice the window flushes');
  // the faces' boxes overlap most in the middle of the rectangle.  Uniform over the block (scalar registers).
  const int rw = rect[1] - rect[0] + 1, rh = rect[3] - rect[2] + 1;
  const int wx0 = rect[0] + max(0, (rw - kAccWin) >> 1), wy0 = rect[2] + max(0, (rh - kAccWin) >> 1);
  const float wx0f = (float)wx0, wy0f = (float)wy0;
  const bool clip = rw > kAccWin || rh > kAccWin;       // some pixel of the block lies outside the LDS window
  constexpr float hwin = 0.5f * (float)(kAccWin - 1);
  const size_t fbase = (size_t)n * S * S;
  unsigned long long* ga = gacc + fbase;
  const float2* zbp = zband + fbase;
  const int sub = t & 15, grp = t >> 4;
  const float inv_s = 1.0f / (float)S;
  const int wv = t >> 6, lane = t & 63;
  float zcn = zc_s;
  asm volatile("" : "+v"(zcn));        // in a vector register: a float add with a scalar operand issues at half rate
  auto flush_band = [&]() {                              // called with the wave converged
    const int cnt = min(__builtin_amdgcn_readfirstlane(st_n[wv]), kBandStage);
    for (int i = lane; i < cnt; i += 64) {
      const size_t pi = fbase + (size_t)st_p[wv][i];
      const unsigned slot = atomicAdd(&bcnt[pi], 1u);
      if (slot < (unsigned)kBandCap) blist[pi * kBandCap + slot] = st_e[wv][i];
    }
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) st_n[wv] = 0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };
  SMALFIT_WORK(int ws_vis = 0; int ws_depth = 0; int ws_eval = 0; int ws_near = 0; int ws_trips = 0; int ws_rounds = 0; int ws_clipped = 0;)
#pragma unroll 1
  for (int step = 0; step < kSweepFaces / 16; ++step) {
    SMALFIT_WORK(ws_rounds += wave_max_i(ws_trips); ws_trips = 0;)
    if (__builtin_amdgcn_readfirstlane(st_n[wv]) >= kBandStage / 2) flush_band();
    const int k = step * 16 + grp;
    const int2 box = boxes[k];
    const int c0 = box.x & 0xffff, c1 = box.x >> 16, r0 = box.y & 0xffff, r1 = box.y >> 16;
    if (c0 > c1) continue;
    FaceRec rk;                                      // in registers: the LDS atomics below would force a reload per pixel
    unpack_face_rec(raw[k][0], raw[k][1], raw[k][2], raw[k][3], rk);
    // The box's pixels in row-major order, 16 at a time (no lane idles except in the last round).  The walk runs in FLOAT
    // (round 4): on this chip only plain float32 multiply-adds / adds and 32-bit integer adds issue at the full rate (~2.6 cycles per
    // wave-instruction per SIMD at 8 waves); conversions, compares, selects, min / max, integer multiply-adds and shift-adds take
    // ~4.5, transcendentals ~8.4 (profiles/r4_ubench_valu_issue_costs.txt), and the loop is bound by exactly that issue time.
    // Every quantity below is a small integer held exactly in a float: row / column from the linear index by one multiply-add,
    // one floor and one more multiply-add ((q + 1/2) / bw stays >= 1/1024 away from an integer, the reciprocal is good to 1 ulp),
    // the pixel centres by the same fused multiply-add as pix_to_ndc (same bits), the pixel's byte offset by one more.
    const int bw = c1 - c0 + 1, npx = bw * (r1 - r0 + 1);
    const bool listed = npx <= 256;                  // box-relative pixel indices are bytes
    // the lane's candidate mask (see kListCap): bit r = "candidate at pixel 16 r + sub".  The round's bit is the same in every lane
    // of the wave (the lanes walk in lockstep): a scalar register pair, shifted once per round; rounds past the 64th shift it out.
    unsigned long long lmask = 0ull, lbit = 1ull;
    const float bwf = (float)bw, ibw = __builtin_amdgcn_rcpf(bwf), hbw = 0.5f * ibw, npxf = (float)npx;
    const float r0f = (float)r0, c0f = (float)c0;
    const float ndc_a = -2.0f * inv_s, ndc_b = 1.0f - inv_s;          // pix_to_ndc(i) = fma(i, ndc_a, ndc_b)
    const float s8 = 8.0f * (float)S;
    // The pixel's cached bounds are requested a ROUND AHEAD (round 5): the load is the head of the round's dependent chain, and on a
    // crop-filling animal the bounds of eight resident windows no longer sit in the L1.  The index maths of the next round is formed
    // twice (here and at the top of that round: carrying it would take the kernel past 64 registers) -- eight more instructions per
    // round and still 3 % less time on both scenes (119.6 -> 115.6 us, 312.8 -> 305.0 us), bit-identical.
    auto bounds_of = [&](float q) {
      const float ry = floorf(fmaf(q, ibw, hbw));
      const float rw = r0f + ry, cl = c0f + fmaf(-ry, bwf, q);
      return *reinterpret_cast<const float2*>(reinterpret_cast<const char*>(zbp) + (unsigned)fmaf(rw, s8, 8.0f * cl));
    };
    float2 zb_next = make_float2(0.f, 0.f);
    if ((float)sub < npxf) zb_next = bounds_of((float)sub);
    for (float qf = (float)sub; qf < npxf; qf += 16.0f, lbit <<= 1) {
      const float ryf = floorf(fmaf(qf, ibw, hbw));
      const float rowf = r0f + ryf, colf = c0f + fmaf(-ryf, bwf, qf);
      const unsigned boff = (unsigned)fmaf(rowf, s8, 8.0f * colf);      // byte offset of the pixel in an 8-byte-per-pixel plane (< 2^24)
      const float2 zb = zb_next;
      if (qf + 16.0f < npxf) zb_next = bounds_of(qf + 16.0f);
      const float ppx = fmaf(colf, ndc_a, ndc_b), ppy = fmaf(rowf, ndc_a, ndc_b);
      const float rz = face_pixel_depth(rk, ppx, ppy) - zcn;   // depth relative to the frame reference
      SMALFIT_WORK(++ws_vis; ++ws_trips;)
      if (!(rz <= zb.y)) continue;                   // beyond the pixel's far bound: dropped whatever its distance
      SMALFIT_WORK(++ws_depth;)
      PixEval e;
      if (!face_pixel_candidate(rk, ppx, ppy, e.d)) continue;
      SMALFIT_WORK(++ws_eval;)
      lmask |= lbit;                                 // the face's candidates: as a mask ...
      if (listed) {                                  // ... and as a list (the backward gather visits these pixels instead of the box)
        const int pos = atomicAdd(&lcn[k], 1);
        if (pos < kListLds) lsts[k][pos] = (unsigned char)(int)qf;
      }
      if (rz <= zb.x) {
        SMALFIT_WORK(++ws_near;)
        const float lxf = colf - wx0f, lyf = rowf - wy0f;
        // (a block whose rectangle fits the window -- nearly all -- skips the per-pixel window test: `clip` is uniform)
        if (!clip || (fabsf(lxf - hwin) <= hwin && fabsf(lyf - hwin) <= hwin))
          atomicAdd(reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(acc) + (unsigned)fmaf(lyf, 8.0f * (float)kAccWin, 8.0f * lxf)), pack_candidate(e.d));
        else { atomicAdd(reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(ga) + boff), pack_candidate(e.d)); SMALFIT_WORK(++ws_clipped;) }
      } else {
        const int sl = atomicAdd(&st_n[wv], 1);
        if (sl < kBandStage) {
          st_p[wv][sl] = (int)(boff >> 3);
          st_e[wv][sl] = make_float2(rz, e.d);
        } else {                                       // staging buffer full: append directly
          const size_t pi = fbase + (size_t)(boff >> 3);
          const unsigned slot = atomicAdd(&bcnt[pi], 1u);
          if (slot < (unsigned)kBandCap) blist[pi * kBandCap + slot] = make_float2(rz, e.d);
        }
      }
    }
    {
      // (lane indices re-derived behind an opaque copy of the thread id: values that are only needed out here must not
      // occupy registers across the pixel loop -- the kernel sits at the 64-register occupancy step)
      int tt = threadIdx.x;
      asm volatile("" : "+v"(tt));
      const int sub2 = tt & 15, k2 = step * 16 + (tt >> 4);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");     // the group's own LDS appends, in program order
      const int cnt = lcn[k2];
      const int2 bx = boxes[k2];
      const int npx2 = ((bx.x >> 16) - (bx.x & 0xffff) + 1) * ((bx.y >> 16) - (bx.y & 0xffff) + 1);
      int n2, bx2;
      xcd_block_of((int)blockIdx.x - box_frame_blocks(M), sweep_blocks_per_frame(F), n2, bx2);
      const size_t fi = (size_t)n2 * F + bx2 * kSweepFaces + k2;
      // one format for the wave's four faces (= the four faces of one backward wave): lists when every one of them has one
      const bool has_list = npx2 <= 256 && cnt <= kListLds;
      unsigned char flag;
      if (__ballot(!has_list) == 0ull) {
        flag = (unsigned char)cnt;
        if (sub2 * 8 < cnt) reinterpret_cast<uint2*>(plist + fi * kListCap)[sub2] = reinterpret_cast<const uint2*>(&lsts[k2][0])[sub2];
      } else if (npx2 <= 16 * kMaskRounds) {
        flag = kMaskList;
        reinterpret_cast<unsigned long long*>(plist + fi * kListCap)[sub2] = lmask;
      } else {
        flag = kNoList;
      }
      if (sub2 == 0) pcount[fi] = flag;
    }
  }
  SMALFIT_WORK(const unsigned long long ws_t3 = __builtin_amdgcn_s_memtime();)
  // the last band flush is split around the window flush: the list slots (returning global atomics, a full trip to the
  // memory side) are requested here and the entries stored after the window has been flushed -- the workgroup is about to
  // retire, and nothing else would hide that trip
  static_assert(kBandStage <= 64, "one staged band entry per lane in the final flush");
  const int fcnt = min(__builtin_amdgcn_readfirstlane(st_n[wv]), kBandStage);
  size_t fpi = 0;
  unsigned fslot = (unsigned)kBandCap;
  float2 fe = make_float2(0.f, 0.f);
  if (lane < fcnt) {
    fpi = fbase + (size_t)st_p[wv][lane];
    fe = st_e[wv][lane];
    fslot = atomicAdd(&bcnt[fpi], 1u);
  }
  __syncthreads();
  SMALFIT_WORK(const unsigned long long ws_t4 = __builtin_amdgcn_s_memtime();)
  SMALFIT_WORK(ws_rounds += wave_max_i(ws_trips); int ws_flush = 0;)
  const int ww = min(kAccWin, rect[1] - wx0 + 1), wh = min(kAccWin, rect[3] - wy0 + 1);
  for (int i = t; i < wh * kAccWin; i += 256) {
    const int lyw = i / kAccWin, lxw = i % kAccWin;
    if (lxw >= ww) continue;
    const unsigned long long v = acc[lyw * kAccWin + lxw];
    if (v) { atomicAdd(&ga[(wy0 + lyw) * S + wx0 + lxw], v); SMALFIT_WORK(++ws_flush;) }
  }
  if (fslot < (unsigned)kBandCap) blist[fpi * kBandCap + fslot] = fe;
  SMALFIT_WORK(work_add(0, ws_vis); work_add(1, ws_depth); work_add(2, ws_eval); work_add(3, ws_near); work_add(7, ws_clipped); work_add(31, (lane == 0 && clip) ? 1 : 0);
               work_add(4, lane == 0 ? ws_rounds : 0); work_add(5, ws_flush); work_add(6, lane == 0 ? 1 : 0);)
}

// The queues of the band / select kernels are filled in a non-deterministic order, so which block sums which pixel
// varies from run to run: their loss partials are kept as 2^-40 fixed-point integers (integer adds commute), which
// makes the reported loss bit-reproducible like everything else.
constexpr float kLossFix = 1099511627776.0f;    // 2^40: a weighted per-pixel loss of 1 over 8M pixels still fits int64
__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int lo = __shfl_xor((int)(v & 0xffffffffll), o, 64), hi = __shfl_xor((int)(v >> 32), o, 64);
    v += ((long long)hi << 32) | (unsigned int)lo;
  }
  return v;
}

// One row of loss terms per frame (smalfit_fit_args.losses_per_frame) needs the queue kernels' loss per FRAME, and their persistent
// workgroups draw pixels of any frame: the <true> instantiations of the band / select kernels also add every settled pixel's
// fixed-point loss to its frame's 64-bit counter -- integer adds again, so order-free and bit-reproducible.  A lane keeps a running
// sum while its pixels stay in one frame (the queues are roughly frame-ordered) and sends one atomic per change of frame.
// Counters sit 256 bytes apart (different memory channels); frame_loss_rows_kernel reads and clears them.  The <false>
// instantiations are the kernels as they were: without per-frame rows nothing here costs a register or an instruction.
// (kFrameLossStride, unsigned long longs between two frames' counters: smalfit_plan.h)
struct FrameLoss { long long acc; int n; };
__device__ __forceinline__ void frame_loss_flush(unsigned long long* floss, FrameLoss& f) {
  if (f.acc) atomicAdd(floss + (size_t)f.n * kFrameLossStride, (unsigned long long)f.acc);
  f.acc = 0;
}
__device__ __forceinline__ void frame_loss_add(unsigned long long* floss, FrameLoss& f, int n, long long v) {
  if (n != f.n) { frame_loss_flush(floss, f); f.n = n; }
  f.acc += v;
}

// alpha = 2^-(sum / 2^24) for the fixed-point log sum of a pixel: integer part by exponent arithmetic, the 24-bit
// fraction through the hardware exp2 (1 ulp) -- no double precision needed; resolve and band kernels share it
__device__ __forceinline__ float alpha_from_log_sum(unsigned long long sum) {
  const unsigned ip = (unsigned)(sum >> 24);
  if (ip >= 160u) return 0.0f;                               // below the smallest float32 denormal
  const float frac = (float)(unsigned)(sum & 0xffffffull) * (1.0f / kLogFix);
  return ldexpf(__builtin_amdgcn_exp2f(-frac), -(int)ip);
}

// 5c: resolve.  With c = #candidates <= lo and b = #band entries of a pixel, the K nearest are known exactly when
// (no bounds yet: c <= K)  or  (c <= K <= c + b: {<= lo} plus the K - c nearest band entries)  or  (hi = +inf and
// c + b < K: everything).  Otherwise -- more than K below lo, a band overflow, an unknown number beyond hi, or a
// depth tie at the cut -- raster_select_kernel redoes the pixel from scratch and refreshes its bounds.
// raster_resolve_kernel is thread-per-pixel: it finishes the pixels that need no sorting and appends the others to
// the band queue or the select queue (one global atomic per block and queue).
// (kResSub, kResEdge -- a resolve workgroup takes (16 kResSub)^2 pixels, kResSub^2 per thread -- and the grid's layout: smalfit_plan.h)
__global__ void __launch_bounds__(256)
raster_resolve_kernel(int S, int M, WinMap win, float w_sil, unsigned long long* __restrict__ gacc,
                      unsigned* __restrict__ bcnt, const int* __restrict__ frect, const float2* __restrict__ zband,
                      SilTarget tsil, float* __restrict__ sil_out,
                      float2* __restrict__ gz, float* __restrict__ blk_loss, int* __restrict__ qcount /*[0] select, [1] band*/,
                      int* __restrict__ queue, int* __restrict__ bqueue, int* __restrict__ stats /*developer counters or null*/,
                      LossArgs la, int loss_frames /*> 0: that many extra workgroups evaluate the per-frame loss terms (loss_block) --
                      independent of the pixels, a chain of dependent latencies, and otherwise a launch of its own*/) {
  // the riders come FIRST in the grid (round 4: at its end they were dispatched after the last pixel workgroup, and their chain of
  // dependent latencies -- ~10 us -- was the tail of the launch); their count is padded to a multiple of 8 so that the pixel
  // workgroups keep their frame -> XCD placement
  const int nlf = resolve_loss_blocks(loss_frames);
  if ((int)blockIdx.x < nlf) {
    if ((int)blockIdx.x < loss_frames) loss_block(la, (int)blockIdx.x);
    return;
  }
  __shared__ int qn[2], qbase[2];
  __shared__ float red[16];
  constexpr int K = kFacesPerPixel;
  constexpr int R2 = kResSub * kResSub;
  constexpr unsigned long long kSumMask = (1ull << kCountShift) - 1ull;
  const float kInf = __int_as_float(0x7f800000);
  const int TX = resolve_tiles_x(S);
  int n, bxi;
  xcd_block_of((int)blockIdx.x - nlf, TX * TX, n, bxi);
  if (n >= M) return;
  const int tx = bxi % TX, ty = bxi / TX;
  const int t = threadIdx.x;
  SMALFIT_WORK(if (t == 0 && bxi == 0 && n == 0) g_probe_seed_scale = w_sil / ((float)win.window * (float)S * (float)S) * (1.0f / kSigma);)
  if (t < 2) qn[t] = 0;
  __syncthreads();
  // tiles outside the frame's active region hold no candidate: silhouette 0, nothing else to read or write
  const int4 fr = *reinterpret_cast<const int4*>(frect + n * 4);
  // A workgroup wholly outside the active region (three quarters of them on the benchmark) only owes the loss the sum of its
  // target pixels.  One wave takes the 32 x 32 pixels, 16 per lane (one 16-byte load of byte targets, four of float targets; the
  // same pixels in the same order either way, so the two storages stay bit-identical), and nobody waits at a workgroup barrier:
  // these workgroups used to hold a CU slot through two barriers each while the active ones queued behind them (-3 us).
  // (The path is taken only without a silhouette image / debug counters and with 16-byte aligned targets, and it adds the same
  // target pixels in another order than the per-thread path below: the REPORTED sil_reproj loss can differ in its last bits between
  // an evaluation that asks for sil_out and one that does not -- never the gradients;
  // tests/test_gpu_parity.py::test_silhouette_loss_with_and_without_the_image_output.)
  {
    const int x0 = tx * kResEdge, y0 = ty * kResEdge;
    const bool wg_active = fr.y > 0 && x0 <= fr.y - 1 && x0 + kResEdge - 1 >= S - fr.x && y0 <= fr.w - 1 && y0 + kResEdge - 1 >= S - fr.z;
    const bool aligned = tsil.b ? ((reinterpret_cast<size_t>(tsil.b) & 15) == 0) : ((reinterpret_cast<size_t>(tsil.f) & 15) == 0);
    if (!wg_active && !sil_out && !stats && kResEdge == 32 && (S & 31) == 0 && aligned) {
      if (!blk_loss || t >= 64) return;
      float l = 0.f;
      if (tsil) {
        const size_t pi = ((size_t)n * S + (y0 + (t >> 1))) * S + x0 + (t & 1) * 16;
        if (tsil.b) {
          const uint4 v = *reinterpret_cast<const uint4*>(tsil.b + pi);
          const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int k = 0; k < 16; ++k) l += (float)((w[k >> 2] >> (8 * (k & 3))) & 0xffu) / 255.0f;
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float4 v = *reinterpret_cast<const float4*>(tsil.f + pi + 4 * k);
            l += fabsf(v.x); l += fabsf(v.y); l += fabsf(v.z); l += fabsf(v.w);
          }
        }
      }
      l = wave_sum(l);
      if (t == 0) blk_loss[(size_t)n * (TX * TX) + bxi] = l;
      return;
    }
  }
  // ---- all loads of the thread's pixels first (independent, in flight together), then the decisions
  size_t pis[R2];
  bool inimg[R2], active[R2];
  unsigned long long vbs[R2];
  int bs[R2];
  float2 zbs[R2];
  float tss[R2];
#pragma unroll
  for (int s = 0; s < R2; ++s) {
    const int stx = tx * kResSub + (s % kResSub), sty = ty * kResSub + (s / kResSub);     // 16-pixel tile of this sub-block
    const int col = stx * 16 + (t & 15), row = sty * 16 + (t >> 4);
    inimg[s] = (col < S) && (row < S);
    pis[s] = ((size_t)n * S + row) * S + col;
    active[s] = inimg[s] && fr.y > 0 && stx * 16 <= fr.y - 1 && stx * 16 + 15 >= S - fr.x && sty * 16 <= fr.w - 1 && sty * 16 + 15 >= S - fr.z;
    vbs[s] = 0ull; bs[s] = 0; zbs[s] = make_float2(kInf, kInf); tss[s] = 0.f;
    if (active[s]) { vbs[s] = gacc[pis[s]]; bs[s] = (int)bcnt[pis[s]]; zbs[s] = zband[pis[s]]; }
    if (inimg[s] && tsil) tss[s] = tsil[pis[s]];
  }
  int action[R2], slot[R2];                        // 0: finished from the sum alone, 1: select queue, 2: band queue
  float l = 0.f;
#pragma unroll
  for (int s = 0; s < R2; ++s) {
    action[s] = 0; slot[s] = 0;
    const size_t pi = pis[s];
    if (inimg[s] && !active[s]) {
      if (sil_out) sil_out[pi] = 0.f;
      if (tsil) l += fabsf(tss[s]);
    }
    if (active[s]) {
      const unsigned long long vb = vbs[s];
      const int c = (int)(vb >> kCountShift);
      const int b = bs[s];
      const float2 zb = zbs[s];
      const int need = K - c;
      float zthr = kInf;
      int act = 0;
      // Saturated pixels (round 5): the c candidates at or below `lo` are ALL accumulated, so with c <= K they are the c nearest, a
      // subset of the K nearest, and the product over the K nearest is at most theirs.  Once that is <= 2^-26 the silhouette is
      // 1.0f exactly whatever the remaining K - c factors are (1 - alpha rounds to 1), and where the target is 1 too the pixel's loss
      // and adjoint seed are exactly zero: nothing for the band ranking or the exact selection to decide.  These are the interior
      // pixels of the animal -- most of the pixels that hold depth bounds at all.  (Their bounds simply stay as they are.)
      const bool saturated = c > 0 && c <= K && (vb & kSumMask) >= (26ull << 24) && (!tsil || tss[s] == 1.0f);
      if (saturated) act = 0;
      else if (!(zb.x < kInf)) act = (c <= K) ? 0 : 1;
      else if (need < 0 || b > kBandCap) act = 1;
      else if (need == 0) zthr = zb.x;                              // exactly K at or below lo
      else if (need > b) act = (zb.y < kInf) ? 1 : (b == 0 ? 0 : 2);   // hi = +inf: fewer than K candidates in all
      else act = 2;
      if (stats && zb.x < kInf) {
        atomicAdd(&stats[1], 1);
        if (act != 1) { atomicAdd(&stats[2], 1); atomicAdd(&stats[3], b); }
        else atomicAdd(&stats[need < 0 ? 4 : (b > kBandCap ? 5 : 6)], 1);
      }
      if (act == 0) {
        const float alpha = (c > 0) ? alpha_from_log_sum(vb & kSumMask) : 1.0f;
        PixelSeed p = pixel_no_target(alpha);
        if (sil_out) sil_out[pi] = p.sil;
        if (tsil) {
          p = pixel_seed(alpha, tss[s], w_sil / ((float)frame_window_size(n, win) * (float)S * (float)S));
          l += p.adiff;
        }
        gz[pi] = make_float2(p.gx, zthr);
      } else {
        slot[s] = atomicAdd(&qn[act - 1], 1);
      }
      // the accumulators are left zero for the next sweep by whoever reads them last (band pixels: raster_band_kernel)
      if (act != 2) {
        if (vb) gacc[pi] = 0ull;
        if (b) bcnt[pi] = 0u;
      }
      action[s] = act;
    }
  }
  // (the workgroup's loss partial shares the two barriers of the queue reservation: same sum, same order as block_sum)
  {
    const float lw = wave_sum(l);
    if ((t & 63) == 0) red[t >> 6] = lw;
  }
  __syncthreads();
  if (t < 2) qbase[t] = qn[t] > 0 ? atomicAdd(&qcount[t], qn[t]) : 0;
  if (t == 64 && blk_loss) {
    float tot = 0.f;
    for (int i = 0; i < 4; ++i) tot += red[i];
    blk_loss[(size_t)n * (TX * TX) + bxi] = tot;
  }
  if (t == 2 && qn[0] > 0) atomicAdd(&qcount[2], qn[0]);   // [2] stays fixed while the band kernel appends its failures to [0]
  __syncthreads();
#pragma unroll
  for (int s = 0; s < R2; ++s) {
    if (action[s] == 1) queue[qbase[0] + slot[s]] = (int)pis[s];
    else if (action[s] == 2) bqueue[qbase[1] + slot[s]] = (int)pis[s] | (bs[s] > 32 ? (int)0x80000000 : 0);   // bit 31: more than 32 band entries
  }
}

// Register budget of the band kernel: the narrow ranking loop is unrolled by four, the rare wide loop stays rolled
constexpr int kBandNarrowUnroll = 4, kBandWideUnroll = 1;
// 5c': band.  Persistent grid, one QUARTER-wave (16 lanes) per queued pixel: a lane holds band entries l and l + 16 (and
// l + 32, l + 48 of the rare lists with more than 32 entries): rank by counting against an LDS broadcast of the depths,
// include the K - c nearest, check for a tie at the cut, then re-centre (and, when the pose moves little, narrow) the
// pixel's bounds.  (Round 3: a band holds 16-30 entries in the steady state, so a half-wave per pixel left half its lanes
// idle; with 16 lanes per pixel twice as many pixels are in flight per wave -- the kernel is bound by the chain of
// dependent loads per pixel, not by arithmetic.)
// the band work of 256-thread workgroup `bi` of `nblocks`.  zs: 16 x 64 floats of LDS.  A pixel whose band cannot decide (a
// depth tie at the cut) is appended to the selection queue.  Returns the lane's loss partial.
template <bool kFrameLoss>
__device__ __forceinline__ long long
band_role(int bi, int nblocks, float (*zs)[64], int S, int M, WinMap win, float w_sil, unsigned long long* __restrict__ gacc,
          unsigned* __restrict__ bcnt, const float2* __restrict__ blist,
          SilTarget tsil, float* __restrict__ sil_out, float2* __restrict__ gz,
          float2* __restrict__ zband, int* __restrict__ qcount, int* __restrict__ queue, const int* __restrict__ bqueue,
          unsigned long long* __restrict__ floss /*kFrameLoss: the per-frame counters*/) {
  static_assert(kBandCap == 64, "four band entries per lane of a quarter-wave");
  (void)M;
  constexpr int K = kFacesPerPixel;
  constexpr unsigned long long kSumMask = (1ull << kCountShift) - 1ull;
  const float kInf = __int_as_float(0x7f800000);
  const int t = threadIdx.x, qw = t >> 4, ql = t & 15;
  const int qshift = 16 * (qw & 3);                         // this quarter's bits in a wave ballot
  const int nb = qcount[1];
  const int npix = S * S;
  long long lacc = 0;
  FrameLoss fl{0, 0};
  // band population this evaluation's miss rate calls for (same rule as the selection kernel; qcount[2] does not
  // change while this kernel runs, so the decision is the same in every run)
  const float miss = (float)qcount[2] / (float)max(qcount[2] + nb, 1);
  const int fill_target = (miss > 0.12f) ? kBandFillWide : ((miss > 0.02f) ? kBandFill : kBandFillNarrow);
  // Software pipeline over this quarter-wave's pixels: the operands of pixel j + 1 (loads that depend on its queue
  // entry) are in flight while pixel j is ranked; the queue entry itself is fetched two pixels ahead.
  const int jstep = nblocks * 16;
  const int j0 = bi * 16 + qw;
  struct Operands { int gp; unsigned long long vb; int b; float ts; float2 zb, e0, e1, e2, e3; };
  auto fetch = [&](int entry) {
    Operands o;
    const int gp = entry & 0x7fffffff;                     // bit 31 of a queue entry: the list has a second half
    o.gp = gp;
    const size_t pi = (size_t)gp;
    o.vb = gacc[pi];
    o.b = (int)bcnt[pi];
    o.ts = tsil ? tsil[pi] : 0.f;
    o.zb = zband[pi];
    o.e0 = blist[pi * kBandCap + ql];                      // list slots are read whether or not they are occupied
    o.e1 = blist[pi * kBandCap + 16 + ql];
    o.e2 = o.e3 = make_float2(0.f, 0.f);
    if (entry < 0) { o.e2 = blist[pi * kBandCap + 32 + ql]; o.e3 = blist[pi * kBandCap + 48 + ql]; }
    return o;
  };
  Operands nxt = fetch((j0 < nb) ? bqueue[j0] : 0);
  int gp_after = (j0 + jstep < nb) ? bqueue[j0 + jstep] : 0;
  for (int j = j0; j < nb; j += jstep) {
    const Operands cur = nxt;
    if (j + jstep < nb) nxt = fetch(gp_after);
    if (j + 2 * jstep < nb) gp_after = bqueue[j + 2 * jstep];
    const int gp = cur.gp;
    const size_t pi = (size_t)gp;
    const unsigned long long vb = cur.vb;
    const int b = cur.b;
    const float ts = cur.ts;
    const float2 zb_old = cur.zb;
    float2 e[4] = {cur.e0, cur.e1, cur.e2, cur.e3};
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (ql + 16 * i >= b) e[i] = make_float2(kInf, 0.f);
    const bool wide = b > 32;                              // uniform over the quarter-wave
    const int need = min(K - (int)(vb >> kCountShift), b);
    if (ql == 0) { gacc[pi] = 0ull; bcnt[pi] = 0u; }        // zero for the next sweep
#pragma unroll
    for (int i = 0; i < 4; ++i) zs[qw][ql + 16 * i] = e[i].x;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    int rank[4] = {0, 0, 0, 0};
#pragma unroll kBandNarrowUnroll
    for (int k4 = 0; k4 < 8; ++k4) {
      const float4 q = *reinterpret_cast<const float4*>(&zs[qw][k4 * 4]);
      rank[0] += (q.x < e[0].x) + (q.y < e[0].x) + (q.z < e[0].x) + (q.w < e[0].x);
      rank[1] += (q.x < e[1].x) + (q.y < e[1].x) + (q.z < e[1].x) + (q.w < e[1].x);
    }
    if (wide) {
#pragma unroll kBandWideUnroll
      for (int k4 = 0; k4 < 8; ++k4) {
        const float4 q = *reinterpret_cast<const float4*>(&zs[qw][k4 * 4]);
        const float4 p = *reinterpret_cast<const float4*>(&zs[qw][32 + k4 * 4]);
        rank[0] += (p.x < e[0].x) + (p.y < e[0].x) + (p.z < e[0].x) + (p.w < e[0].x);
        rank[1] += (p.x < e[1].x) + (p.y < e[1].x) + (p.z < e[1].x) + (p.w < e[1].x);
        rank[2] += (q.x < e[2].x) + (q.y < e[2].x) + (q.z < e[2].x) + (q.w < e[2].x) + (p.x < e[2].x) + (p.y < e[2].x) + (p.z < e[2].x) + (p.w < e[2].x);
        rank[3] += (q.x < e[3].x) + (q.y < e[3].x) + (q.z < e[3].x) + (q.w < e[3].x) + (p.x < e[3].x) + (p.y < e[3].x) + (p.z < e[3].x) + (p.w < e[3].x);
      }
    }
    unsigned long long pv = 0ull;
    float zin = -kInf, zout = kInf;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool live = ql + 16 * i < b, in = live && rank[i] < need;
      if (in) { pv += pack_candidate(e[i].y) & kSumMask; zin = fmaxf(zin, e[i].x); }
      if (live && !in) zout = fminf(zout, e[i].x);
    }
    int s_lo = (int)(pv & 0xffffffull), s_hi = (int)(pv >> 24);        // <= 4 terms of < 2^32 per lane, 16 lanes: both halves fit an int
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
      s_lo += __shfl_xor(s_lo, o, 16); s_hi += __shfl_xor(s_hi, o, 16);
      zin = fmaxf(zin, __shfl_xor(zin, o, 16)); zout = fminf(zout, __shfl_xor(zout, o, 16));
    }
    // ranks ignore ties: with a tie at the cut the number of entries <= zin is not `need`; let the selection decide
    int taken = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned long long bal = __ballot((ql + 16 * i < b) && (e[i].x <= zin));
      taken += __popc((unsigned)(bal >> qshift) & 0xffffu);
    }
    if (ql == 0) {
      if (taken == need && zin < zout) {
        const unsigned long long sum = (vb & kSumMask) + ((unsigned long long)(unsigned)s_hi << 24) + (unsigned long long)(unsigned)s_lo;
        const float alpha = alpha_from_log_sum(sum);
        PixelSeed p = pixel_no_target(alpha);
        if (sil_out) sil_out[pi] = p.sil;
        if (tsil) {
          const int n = gp / npix;
          const float wn = w_sil / ((float)frame_window_size(n, win) * (float)S * (float)S);
          p = pixel_seed(alpha, ts, wn);
          const long long lp = (long long)(p.adiff * wn * kLossFix);
          lacc += lp;
          if constexpr (kFrameLoss) frame_loss_add(floss, fl, n, lp);
        }
        gz[pi] = make_float2(p.gx, zin);
        // re-centre the pixel's bounds on the depth of its K-th nearest as just determined (zin), keeping the
        // half-width (or narrowing it when it holds more candidates than the current pose motion calls for): the band
        // follows the surface from iteration to iteration.  Bounds are hints -- any value is valid.
        if (zb_old.y < kInf) {
          float half = 0.5f * (zb_old.y - zb_old.x);
          if (4 * b > 5 * fill_target) half *= (float)fill_target / (float)b;   // wider than the pose motion needs now
          zband[pi] = make_float2(zin - half, zin + half);
        }
      } else {
        queue[atomicAdd(&qcount[0], 1)] = gp;
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
  if constexpr (kFrameLoss) frame_loss_flush(floss, fl);
  return lacc;
}

// 6 waves per SIMD: <= 80 registers, six instead of five workgroups per CU (resolve + band 43.5 -> 41.9 us; 8 spills)
template <bool kFrameLoss>
__global__ void __launch_bounds__(256, 6)
raster_band_kernel(int S, int M, WinMap win, float w_sil, unsigned long long* __restrict__ gacc,
                   unsigned* __restrict__ bcnt, const float2* __restrict__ blist,
                   SilTarget tsil, float* __restrict__ sil_out, float2* __restrict__ gz,
                   float2* __restrict__ zband, int* __restrict__ qcount, int* __restrict__ queue,
                   const int* __restrict__ bqueue, long long* __restrict__ bloss /*[gridDim.x]: weighted |sil - target| per block in 2^-40 fixed point, or null*/,
                   unsigned long long* __restrict__ floss /*kFrameLoss: [M][kFrameLossStride], the same loss per frame*/) {
  __shared__ __attribute__((aligned(16))) float zs[16][64];
  const int t = threadIdx.x;
  const long long lacc = band_role<kFrameLoss>(blockIdx.x, gridDim.x, zs, S, M, win, w_sil, gacc, bcnt, blist, tsil, sil_out, gz, zband,
                                               qcount, queue, bqueue, floss);
  if (bloss) {
    __shared__ long long lred[4];
    const long long ws = wave_sum_i64(lacc);
    if ((t & 63) == 0) lred[t >> 6] = ws;
    __syncthreads();
    if (t == 0) bloss[blockIdx.x] = (lred[0] + lred[1]) + (lred[2] + lred[3]);
  }
}

// 5d: select.  Persistent grid; one wave per queued pixel: it walks the union boxes (8 faces each)
// containing the pixel, evaluates those faces (lane per face, record loads software-prefetched), compacts
// the candidates into LDS in face order, finds the K-th smallest depth exactly (histogram over a linear quantisation
// of the depth range, narrowed to <= 64 entries, then exact ranks) and multiplies the K nearest (1 - p) in a fixed order.
constexpr int kCandCap = 1024;            // candidates per pixel kept in LDS; beyond: multi-pass re-evaluation
constexpr int kHitCap = 1024;             // union boxes containing a pixel kept in LDS (aliases the candidate buffer)
// faces whose box covers the pixel, kept in LDS (u16 ids).  Round 3: 11 KB of LDS per wave -> 7 workgroups (14 waves) per CU at
// <= 128 registers; a pixel with more covering faces walks every face instead, which costs about as many rounds as the three-stage
// scan of such a pixel
constexpr int kCoverCap = 1024;

constexpr int kSelSlots = 2;              // rounds of face records in flight per wave while a pixel's covering faces are evaluated (4 measured the same as 2, with 14 more VGPRs)

// one queued pixel, by one wave (see the kernel below): the exact K nearest from scratch.  Returns (lane 0) the pixel's weighted
// |sil - target| in 2^-40 fixed point.  L: this wave's LDS (histogram, candidates, cover list).
struct SelCtx {
  int F, S, M;
  WinMap win;
  float w_sil;
  const float4* frec; const float* zc; const int4* brect; const int2* fbox;
  SilTarget tsil;
  float* sil_out; float2* gz; float2* zband; unsigned char* pcount;
  int dbg, band_fill;
};
struct SelLds { unsigned* hist /*[256]*/; float2* cand /*[kCandCap]*/; unsigned short* fids /*[kCoverCap]*/; };
constexpr int kSelLdsBytes = 256 * 4 + kCandCap * 8 + kCoverCap * 2;     // per wave
__device__ __forceinline__ SelLds sel_lds(unsigned char* base) {
  return SelLds{reinterpret_cast<unsigned*>(base), reinterpret_cast<float2*>(base + 256 * 4),
                reinterpret_cast<unsigned short*>(base + 256 * 4 + kCandCap * 8)};
}
__device__ __forceinline__ long long select_pixel(const SelCtx& c, const SelLds& L, int gp) {
  // the union-box hit list is consumed (stage A) before the first candidate is written (stage B): share storage
  int* hits = reinterpret_cast<int*>(L.cand);
  static_assert(kHitCap <= 2 * kCandCap, "hit list must fit in the candidate buffer");
  constexpr int K = kFacesPerPixel;
  constexpr int RC = kCandCap / 64;
  constexpr int RPI = 64 / kRectFaces;      // union boxes handled per wave iteration
  const int lane = threadIdx.x & 63;
  const int F = c.F, S = c.S, M = c.M;
  (void)M;
  const int nrect = rect_count(F);
  const float inv_s = 1.0f / (float)S;
  const int npix = S * S;
  long long loss_fp = 0;
  const int n = gp / npix, pix = gp % npix;
  const int pcol = pix % S, prow = pix / S;
  const float ppx = pix_to_ndc(pcol, inv_s), ppy = pix_to_ndc(prow, inv_s);
  const float zcn = c.zc[n];
  // the pixel's own operands are requested here, at the head of the chain of dependent trips, not where they are used
  const float hi_old = c.zband[(size_t)gp].y;            // the far bound the forward sweep applied to this pixel
  const float ts = c.tsil ? c.tsil[(size_t)gp] : 0.f;
  const int4* br = c.brect + (size_t)n * nrect;
  const float4* fr = c.frec + (size_t)n * F * kRecVecs;
  // union boxes containing the pixel (ascending); 8 independent loads in flight per round
  int nh = 0;
  for (int r0 = 0; r0 < nrect; r0 += 512) {
    int4 b[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int ri = r0 + u * 64 + lane;
      b[u] = (ri < nrect) ? br[ri] : make_int4(1, 0, 1, 0);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const bool hit = b[u].x <= pcol && pcol <= b[u].y && b[u].z <= prow && prow <= b[u].w;
      const unsigned long long bal = __ballot(hit);
      if (hit) { const int pos = nh + __popcll(bal & ((1ull << lane) - 1ull)); if (pos < kHitCap) hits[pos] = r0 + u * 64 + lane; }
      nh += __popcll(bal);
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  if (SMALFIT_PROBE(c.dbg, 1)) return 0;
  // faces whose pixel box covers the pixel (ascending ids): 8-byte box test only, nothing evaluated yet
  const int2* fb = c.fbox + (size_t)n * F;
  int ncov = 0;
  if (nh <= kHitCap) {
    for (int j = 0; j < nh; j += 8 * RPI) {
      int ff[8];
      int2 bx[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int hj = j + u * RPI + lane / kRectFaces;
        ff[u] = -1;
        bx[u] = make_int2(1, 1);
        if (hj < nh) {
          const int f = hits[hj] * kRectFaces + (lane & (kRectFaces - 1));
          if (f < F) { ff[u] = f; bx[u] = fb[f]; }
        }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const bool cov = ff[u] >= 0 && box_contains(bx[u], pcol, prow);
        const unsigned long long bal = __ballot(cov);
        if (cov) { const int pos = ncov + __popcll(bal & ((1ull << lane) - 1ull)); if (pos < kCoverCap) L.fids[pos] = (unsigned short)ff[u]; }
        ncov += __popcll(bal);
      }
    }
  }
  if (SMALFIT_PROBE(c.dbg, 2)) return 0;
  // compact: the cover list fids[] is valid.  Stage B below overwrites its head with the candidates' face ids (slot
  // <= source index, so nothing unread is lost) -- when the candidates overflow their buffer and have to be
  // re-evaluated, the list is gone and the pixel falls back to walking every face (pathological pixels only).
  bool compact = (nh <= kHitCap) && (ncov <= kCoverCap) && (F <= 65536);
  const bool had_list = compact;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  // visit every candidate of the pixel in face order: fn(valid, pz, d, face) is called wave-wide
  auto scan_candidates = [&](auto&& fn) {
    if (compact) {
      // records of kSelSlots rounds (64 faces each) in flight: the scan is a chain of dependent record loads, and how many
      // rounds are outstanding sets how many trips to L2 a pixel's ~300-900 covering faces cost
      float4 pa[kSelSlots], pb[kSelSlots], pc[kSelSlots], pd[kSelSlots];
      bool plive[kSelSlots];
      auto prefetch = [&](int j, int slot) {
        plive[slot] = (j + lane) < ncov;
        if (plive[slot]) {
          const int ff = L.fids[j + lane];
          const float4* p = fr + (size_t)ff * kRecVecs;
          pa[slot] = p[0]; pb[slot] = p[1]; pc[slot] = p[2]; pd[slot] = p[3];
        }
      };
      auto consume = [&](int j, int slot) {
        const float4 a = pa[slot], b = pb[slot], c = pc[slot], d = pd[slot];
        const bool live = plive[slot];
        const int cur_ff = live ? (int)L.fids[j + lane] : 0;
        if (j + 64 * kSelSlots < ncov) prefetch(j + 64 * kSelSlots, slot);
        bool ok = false;
        PixEval e; e.pz = 0.f; e.d = 0.f;
        if (live) {
          FaceRec r;
          unpack_face_rec(a, b, c, d, r);
          ok = face_pixel_candidate(r, ppx, ppy, e.d);       // decision + signed distance only (face_pixel_bary / face_pixel_edges, as face_pixel_eval)
          e.pz = face_pixel_depth(r, ppx, ppy);
        }
        fn(ok, e.pz - zcn, e.d, cur_ff);
      };
#pragma unroll
      for (int k = 0; k < kSelSlots; ++k)
        if (64 * k < ncov) prefetch(64 * k, k);
      for (int j = 0; j < ncov; j += 64 * kSelSlots) {
#pragma unroll
        for (int k = 0; k < kSelSlots; ++k)
          if (j + 64 * k < ncov) consume(j + 64 * k, k);
      }
    } else {                      // pathological: walk every face
      for (int f0 = 0; f0 < F; f0 += 64) {
        const int ff = f0 + lane;
        bool ok = false;
        PixEval e; e.pz = 0.f; e.d = 0.f;
        if (ff < F) {
          FaceRec r;
          const int2 box = fb[ff];
          load_face_rec(fr + (size_t)ff * kRecVecs, r);
          if (box_contains(box, pcol, prow)) { ok = face_pixel_candidate(r, ppx, ppy, e.d); e.pz = face_pixel_depth(r, ppx, ppy); }
        }
        fn(ok, e.pz - zcn, e.d, ff);
      }
    }
  };
  int nc = 0;
  const float kInf = __int_as_float(0x7f800000);
  float zmn = kInf, zmx = -kInf;                      // depth range of the candidates
  scan_candidates([&](bool ok, float pz, float d, int ff) {
    const unsigned long long bal = __ballot(ok);
    if (ok) {
      const int pos = nc + __popcll(bal & ((1ull << lane) - 1ull));
      if (pos < kCandCap) {
        L.cand[pos] = make_float2(pz, one_minus_prob(d));
        if (had_list) L.fids[pos] = (unsigned short)ff;      // candidate -> face id, in place (see `compact`)
      }
      zmn = fminf(zmn, pz); zmx = fmaxf(zmx, pz);
    }
    nc += __popcll(bal);
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { zmn = fminf(zmn, __shfl_xor(zmn, o, 64)); zmx = fmaxf(zmx, __shfl_xor(zmx, o, 64)); }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  if (SMALFIT_PROBE(c.dbg, 4)) return 0;
  const bool cached = nc <= kCandCap;
  if (!cached) compact = false;                       // the head of the cover list now holds candidate ids
  // visit every candidate wave-wide: fn(valid, depth, 1 - p); from LDS, or by re-evaluation when they did not fit
  auto visit = [&](auto&& fn) {
    if (cached) {
#pragma unroll 4
      for (int i = 0; i < RC; ++i) {
        const int j = lane + 64 * i;
        if (64 * i >= nc) break;
        const float2 ev = (j < nc) ? L.cand[j] : make_float2(0.f, 1.f);
        fn(j < nc, ev.x, ev.y);
      }
    } else {
      scan_candidates([&](bool ok, float pz, float d, int ff) { (void)ff; fn(ok, pz, ok ? one_minus_prob(d) : 1.0f); });
    }
  };
  // ---- depth of the K-th nearest: histogram over a linear quantisation of the current depth range (monotone, so the
  // K-th lies in the bin where the running count crosses K), narrowed until that bin holds at most 64 candidates,
  // which are then ranked exactly.  Usually one histogram pass.
  float zk = kInf;
  if (nc > K) {
    float rlo = zmn, rhi = zmx;
    int need = K;
    float* sel = reinterpret_cast<float*>(&L.hist[0]);
    for (int round = 0; round < 64; ++round) {
      if (!(rhi > rlo)) { zk = rlo; break; }            // everything left has the same depth
      const float scale = 256.0f / (rhi - rlo);
#pragma unroll
      for (int i = 0; i < 4; ++i) L.hist[lane * 4 + i] = 0u;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      visit([&](bool ok, float z, float omp) {
        (void)omp;
        if (ok && z >= rlo && z <= rhi) atomicAdd(&L.hist[min(255, (int)((z - rlo) * scale))], 1u);
      });
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const unsigned h0 = L.hist[lane * 4], h1 = L.hist[lane * 4 + 1], h2 = L.hist[lane * 4 + 2], h3 = L.hist[lane * 4 + 3];
      const int s4 = (int)(h0 + h1 + h2 + h3);
      int incl = s4;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int v = __shfl_up(incl, d, 64);
        if (lane >= d) incl += v;
      }
      const int excl = incl - s4;
      const bool mine = (excl < need) && (need <= incl);
      int digit = 0, below = 0, cnt = 0;
      if (mine) {
        int cm = excl;
        if (cm + (int)h0 >= need) { digit = lane * 4; below = cm; cnt = (int)h0; }
        else { cm += (int)h0;
          if (cm + (int)h1 >= need) { digit = lane * 4 + 1; below = cm; cnt = (int)h1; }
          else { cm += (int)h1;
            if (cm + (int)h2 >= need) { digit = lane * 4 + 2; below = cm; cnt = (int)h2; }
            else { cm += (int)h2; digit = lane * 4 + 3; below = cm; cnt = (int)h3; } } }
      }
      const unsigned long long balm = __ballot(mine);
      const int srcl = __ffsll((long long)balm) - 1;
      digit = __shfl(digit, srcl, 64);
      below = __shfl(below, srcl, 64);
      cnt = __shfl(cnt, srcl, 64);
      need -= below;
      __builtin_amdgcn_wave_barrier();
      if (cnt <= 64) {
        // the bin's members into sel[] (the histogram is no longer needed), then exact ranks
        int ns = 0;
        visit([&](bool ok, float z, float omp) {
          (void)omp;
          const bool in = ok && z >= rlo && z <= rhi && min(255, (int)((z - rlo) * scale)) == digit;
          const unsigned long long bal = __ballot(in);
          if (in) sel[ns + __popcll(bal & ((1ull << lane) - 1ull))] = z;
          ns += __popcll(bal);
        });
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const float key = (lane < ns) ? sel[lane] : kInf;
        int rank = 0;
        for (int q = 0; q < ns; ++q) { const float o = sel[q]; rank += (o < key || (o == key && q < lane)) ? 1 : 0; }
        const unsigned long long balk = __ballot(lane < ns && rank == need - 1);
        zk = __shfl(key, __ffsll((long long)balk) - 1, 64);
        __builtin_amdgcn_wave_barrier();
        break;
      }
      // narrow the range to the members of that bin
      float nlo = kInf, nhi = -kInf;
      visit([&](bool ok, float z, float omp) {
        (void)omp;
        if (ok && z >= rlo && z <= rhi && min(255, (int)((z - rlo) * scale)) == digit) { nlo = fminf(nlo, z); nhi = fmaxf(nhi, z); }
      });
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) { nlo = fminf(nlo, __shfl_xor(nlo, o, 64)); nhi = fmaxf(nhi, __shfl_xor(nhi, o, 64)); }
      rlo = nlo; rhi = nhi;
    }
  }
  // ---- one pass: product of the included factors, the nearest depth beyond the K-th, and the band population
  // for kBandTries candidate half-widths (delta, delta/2, delta/4, ...)
  constexpr int kBandTries = 6;
  const float delta0 = (nc > K) ? kBandHalf * (zk - zmn) * (1.0f / (float)K) : 0.f;
  float a = 1.0f, znext = kInf;
  // The half-widths' bounds are wave-uniform: held in scalar registers, and each population is counted with a ballot (scalar
  // adds) -- a third of the vector instructions of per-lane counters, and nothing to reduce afterwards.  How many candidates
  // lie BEYOND a half-width needs no count at all: none do exactly when the farthest candidate (zmx) does not.
  float tlo[kBandTries], thi[kBandTries];
  int cbs[kBandTries];
  {
    float dl = delta0;
#pragma unroll
    for (int i = 0; i < kBandTries; ++i) {
      tlo[i] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(zk - dl)));
      thi[i] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(zk + dl)));
      cbs[i] = 0;
      dl *= 0.5f;
    }
  }
  visit([&](bool ok, float z, float omp) {
    if (ok) { if (z <= zk) a *= omp; else znext = fminf(znext, z); }
#pragma unroll
    for (int i = 0; i < kBandTries; ++i) cbs[i] += __popcll(__ballot(ok && z > tlo[i] && z <= thi[i]));
  });
  a = wave_prod(a);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) znext = fminf(znext, __shfl_xor(znext, o, 64));
  // backward threshold: midway between the K-th and the (K+1)-th nearest depth
  float zmid = zk;
  if (nc > K && znext < kInf) {
    zmid = 0.5f * (zk + znext);
    if (!(zmid >= zk && zmid < znext)) zmid = zk;
  }
  // bounds for the next evaluations: lo < K-th <= hi, the band (lo, hi] sized to at most kBandFill candidates, so
  // that the K nearest stay provable from counts while depths drift by up to the band's half-width
  float blo = kInf, bhi = kInf;
  if (nc > K) {
    blo = bhi = zmid;
    const int fill = c.band_fill;
    float delta = delta0;
    bool chosen = false;
#pragma unroll
    for (int i = 0; i < kBandTries; ++i) {
      if (!chosen && cbs[i] <= fill && zk - delta < zk) {
        blo = zk - delta; bhi = (zmx > thi[i]) ? zk + delta : kInf; chosen = true;
      }
      delta *= 0.5f;
    }
  }
  // Candidates among the K nearest that lie beyond the far bound the forward sweep used were dropped there
  // unevaluated, so they are missing from their faces' candidate lists: those faces walk their whole box in the
  // backward gather (idempotent byte stores, no atomics).  Only a "short" miss -- the K-th nearest beyond a finite
  // far bound -- produces any.
  if (hi_old < kInf && zk > hi_old) {
    unsigned char* pc = c.pcount + (size_t)n * F;
    if (cached && had_list) {
      for (int i = lane; i < nc; i += 64) {
        const float z = L.cand[i].x;
        if (z > hi_old && z <= zk) pc[L.fids[i]] = kNoList;
      }
    } else {
      scan_candidates([&](bool ok, float pz, float d, int ff) { (void)d; if (ok && pz > hi_old && pz <= zk) pc[ff] = kNoList; });
    }
  }
  if (lane == 0) {
    const size_t pi = (size_t)gp;
    PixelSeed p = pixel_no_target(a);
    if (c.sil_out) c.sil_out[pi] = p.sil;
    float l = 0.f;
    if (c.tsil) {
      const float wn = c.w_sil / ((float)frame_window_size(n, c.win) * (float)S * (float)S);
      p = pixel_seed(a, ts, wn);
      l = p.adiff * wn;
    }
    c.gz[pi] = make_float2(p.gx, zmid);
    c.zband[pi] = make_float2(blo, bhi);
    loss_fp = (long long)(l * kLossFix);
  }
  __builtin_amdgcn_wave_barrier();
  return loss_fp;
}

// 4 waves per SIMD: <= 128 VGPRs (133 unconstrained; 12 bytes of scratch), LDS admits 14 waves per CU
template <bool kFrameLoss>
__global__ void __launch_bounds__(64 * kSelWaves, 4)
raster_select_kernel(int F, int S, int M, WinMap win, float w_sil, const float4* __restrict__ frec, const float* __restrict__ zc,
                     const int4* __restrict__ brect, const int2* __restrict__ fbox, int* __restrict__ qcount,
                     const int* __restrict__ queue, SilTarget tsil,
                     float* __restrict__ sil_out, float2* __restrict__ gz, float2* __restrict__ zband,
                     unsigned char* __restrict__ pcount /*[M][F]: set to kNoList for faces the forward sweep's lists may miss*/,
                     long long* __restrict__ qloss /*[gridDim.x]: weighted |sil - target| per block in 2^-40 fixed point, or null*/, int dbg,
                     unsigned long long* __restrict__ floss /*kFrameLoss: [M][kFrameLossStride], the same loss per frame*/) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[kSelWaves][kSelLdsBytes];
  __shared__ long long wloss[kSelWaves];
  long long lacc = 0;
  FrameLoss fl{0, 0};
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int nq = *qcount;                                   // resolve's pixels + the band kernel's failures
  // how many candidates the new bands may hold: wide bands survive large parameter steps (stage 1) but cost list
  // appends and band sorting in every later evaluation, narrow ones are cheap while the pose barely moves.  The share
  // of bounded pixels that needed this kernel in the current evaluation decides.
  const int nbandq = qcount[1];
  const float miss = (float)nq / (float)max(nq + nbandq, 1);
  SelCtx c;
  c.F = F; c.S = S; c.M = M; c.win = win; c.w_sil = w_sil; c.frec = frec; c.zc = zc; c.brect = brect; c.fbox = fbox; c.tsil = tsil;
  c.sil_out = sil_out; c.gz = gz; c.zband = zband; c.pcount = pcount; c.dbg = dbg;
  c.band_fill = (miss > 0.12f) ? kBandFillWide : ((miss > 0.02f) ? kBandFill : kBandFillNarrow);
  const SelLds L = sel_lds(&lds[w][0]);
  // XCD-affine split of the queue: workgroups are dealt to the 8 XCDs round-robin, and the queue is roughly
  // frame-ordered (resolve blocks of a frame append together), so XCD x takes the x-th eighth of it and its L2 only
  // has to hold the face records of ~M/8 frames instead of all of them.  Within its eighth a wave draws pixels by ticket
  // (one atomic per pixel on the XCD's counter, requested a pixel ahead together with the queue entry it selects): a pixel
  // costs between a few hundred and a few thousand instructions, and with a fixed deal of ~40 pixels per wave the launch
  // ended with its unluckiest wave.  Which wave takes which pixel changes nothing: a pixel's result is its own, and the
  // loss partials are integers.
  const int xcd = blockIdx.x & 7, grp = (int)(blockIdx.x >> 3) % kSelGroups;
  const int q_lo = (int)(((long long)nq * xcd) >> 3), q_hi = (int)(((long long)nq * (xcd + 1)) >> 3);
  int* ticket = qcount + kTicketBase + (xcd * kSelGroups + grp) * kTicketStride;
  // Tickets are drawn in batches of B per wave.  The draw is a returning atomic by lane 0, and the compiler waits for it at the end
  // of the branch that issues it (tools/isa_loads.py: "A w0"): a full trip to the memory side (~2 us) that nothing hides.  With
  // B = 1 that is ~15 % of a ~13 us pixel; a batch pays it once per B pixels at the price of a tail of at most B - 1 pixels for
  // the last wave.  B follows the queue: 1 while a wave gets about one pixel anyway (steady state), up to kTicketBatch when
  // there are dozens per wave (cold cache, large parameter steps).  The decision is the same in every wave of the launch.
  constexpr int kTicketBatch = 4;
  const int group_waves = (((int)gridDim.x >> 3) / kSelGroups) * kSelWaves;            // waves drawing from this counter
  const int per_wave = ((q_hi - q_lo) / kSelGroups) / max(group_waves, 1);             // pixels per wave if dealt evenly
  const int B = min(max(per_wave / 8, 1), kTicketBatch);
  auto entry = [&](int tk) { const int qi = q_lo + grp + tk * kSelGroups; return (qi < q_hi) ? queue[qi] : -1; };
  for (;;) {
    int tk = 0;
    if (lane == 0) tk = atomicAdd(ticket, B);
    tk = __builtin_amdgcn_readfirstlane(tk);
    int gp = entry(tk);
    if (gp < 0) break;                                       // tickets only grow: nothing left for this group
    bool more = true;
#pragma unroll 1
    for (int i = 0; i < B; ++i) {
      const int gp_next = (i + 1 < B) ? entry(tk + i + 1) : -1;     // in flight while this pixel is selected
      const long long lp = select_pixel(c, L, gp);
      lacc += lp;
      if constexpr (kFrameLoss) { if (lane == 0) frame_loss_add(floss, fl, gp / (S * S), lp); }
      __builtin_amdgcn_wave_barrier();
      gp = gp_next;
      if (gp < 0) { more = (i + 1 == B); break; }            // end of the batch, or the batch ran past the end of the share
    }
    if (!more) break;
  }
  if constexpr (kFrameLoss) { if (lane == 0) frame_loss_flush(floss, fl); }
  if (qloss) {
    if (lane == 0) wloss[w] = lacc;
    __syncthreads();
    if (t == 0) { long long tot = 0; for (int i = 0; i < kSelWaves; ++i) tot += wloss[i]; qloss[blockIdx.x] = tot; }
  }
}

// (Round 3 also built band + selection as ONE launch -- selection workgroups of 4 waves, band workgroups, LDS carved per role,
// band failures redone by the workgroup's own select_pixel: bit-identical, but the band role inherits the selection's 53 KB /
// 133 registers (3 workgroups per CU) and 4-wave selection workgroups end with their slowest wave: 2200 vs 2294 it/s, stage 1
// 1515 vs 1675.  tools/experiments/r3_band_select_merged_launch.patch, profiles/r3_ab_band_select_merged_launch.txt.)

// gz = (dsil * (-(1 - sil) / sigma), zthr)   (component API: arbitrary upstream gradient)
__global__ void gpix_from_dsil_kernel(size_t total, const float* __restrict__ sil, const float* __restrict__ dsil,
                                      float2* __restrict__ gz) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total) gz[i].x = -dsil[i] * (1.0f - sil[i]) * (1.0f / kSigma);
}

// 5e: backward, face-parallel gather (deterministic, no atomics).  16 lanes per face walk the face's pixel box
// row-major like the forward sweep; d(signed dist^2)/d(vertex) flows through the nearest edge only.
static_assert(kBwdLanes == 16, "mask lists are laid out for 16 lanes per face");
// faces per workgroup of the backward gather (16 lanes each).  One wave per workgroup measured best (4 / 8 / 16 / 32 / 64 faces:
// 90 / 92 / 93 / 100 / 111 us): a wave that is done frees its slot at once instead of waiting for its block mates
static_assert(kSweepFaces % 16 == 0 && kBwdFaces * kBwdLanes == 64,
              "a sweep round is 16 faces of 16 lanes, and the four faces of a sweep wave are the four faces of a backward wave");
// kUnclampedT (smalfit_engine_set_option SMALFIT_OPT_UNCLAMPED_EDGE_T; SURVEY App. B, last row): the adjoint of the point-segment
// distance with the edge parameter t NOT clamped to [0, 1] -- q = p - (a + t (b - a)) on the infinite line, weights (1 - t), t --
// which is what some pytorch3d 0.2.x sources are recalled to compute in PointLineDistanceBackward.  It differs from the exact
// gradient (the default) only at pixels whose nearest point of the nearest edge is one of its end points.  The forward, and with
// it which edge is the nearest, is the same either way.
template <bool kUnclampedT>
__global__ void __launch_bounds__(kBwdLanes * kBwdFaces)
raster_bwd_kernel(int F, int M, int S, float inv_s /*1 / S, divided on the host: the same bits, and no division sequence in every wave*/,
                  const float4* __restrict__ frec, const int2* __restrict__ fbox, const float* __restrict__ zc, const float2* __restrict__ gz,
                  const unsigned char* __restrict__ plist /*[M][F][kListCap]*/, const unsigned char* __restrict__ pcount /*[M][F]*/,
                  float* __restrict__ dface /*[M][F][6]*/) {
  int n, bxi;
  xcd_block(raster_bwd_blocks_per_frame(F), n, bxi);
  const bool frame_ok = n < M;
  if (!frame_ok) n = 0;
  const int f = frame_ok ? bxi * kBwdFaces + ((int)threadIdx.x / kBwdLanes) : F;
  const int sub = threadIdx.x & (kBwdLanes - 1);
  float ga[2] = {0.f, 0.f}, gb[2] = {0.f, 0.f}, gc[2] = {0.f, 0.f};
  // (pin: knowing the sums are zero in the two peeled rounds, the compiler multiplies into fresh registers there and moves six
  // zeros at each of pair's three exits; opaque, every round accumulates in place like the rolled loop)
  asm volatile("" : "+v"(ga[0]), "+v"(ga[1]), "+v"(gb[0]), "+v"(gb[1]), "+v"(gc[0]), "+v"(gc[1]));
  // Everything keyed by the face is addressed as (the frame's base, uniform over the workgroup: scalar registers) + (an unsigned
  // 32-bit byte offset of the face in its frame: one vector register), the form the loads take without any 64-bit lane arithmetic.
  // The largest offset is the list's, f kListCap + 127 < 2^32: kMaxModelFaces (smalfit_plan.h)
  static_assert((unsigned long long)kMaxModelFaces * kListCap <= (1ull << 32), "a face's byte offset in its frame's lists fits 32 bits");
  const size_t nF = (size_t)n * F;
  const unsigned char* lst_n = plist + nF * kListCap;
  const unsigned char* cnt_n = pcount + nF;
  const char* rec_n = reinterpret_cast<const char*>(frec + nF * kRecVecs);
  const char* box_n = reinterpret_cast<const char*>(fbox + nF);
  char* out_n = reinterpret_cast<char*>(dface + nF * 6);
  SMALFIT_WORK(int wb_vis = 0; int wb_live = 0; int wb_eval = 0; int wb_in = 0; int wb_trips = 0; int wb_deadr = 0; int wb_r = 0;
               const unsigned long long wb_t0 = __builtin_amdgcn_s_memtime(); unsigned long long wb_t1 = wb_t0;
               int wb_a12 = 0; int wb_a24 = 0; int wb_a40 = 0; float wb_amax = 0.f;)
  float zcn = zc[n];                   // requested with everything else below; in a vector register: a float subtract with a
  asm volatile("" : "+v"(zcn));        // scalar operand issues at half rate
  if (f < F) {
    // everything whose address depends on the face id alone is requested in one go: the record, the list's flag / length, its
    // first two rounds of entries (most lists are shorter) and the lane's candidate mask (the same 128 bytes read the other way) --
    // one trip to memory, not three
    const unsigned uf = (unsigned)f, lst_off = uf * (unsigned)kListCap;
    int cnt = cnt_n[uf];
    int q_first = lst_n[lst_off + (unsigned)sub], q_second = lst_n[lst_off + (unsigned)(sub + kBwdLanes)];
    unsigned long long lmask = *reinterpret_cast<const unsigned long long*>(lst_n + (lst_off + (unsigned)sub * 8u));
    const float4* fr = reinterpret_cast<const float4*>(rec_n + uf * (unsigned)(kRecVecs * sizeof(float4)));
    float4 ra = fr[0], rb = fr[1], rc = fr[2], rd = fr[3];
    int2 box = *reinterpret_cast<const int2*>(box_n + uf * (unsigned)sizeof(int2));
    // (pin: the compiler would otherwise sink each load to its first use, behind the branches, and serialise the trips)
    {
      unsigned mlo = (unsigned)lmask, mhi = (unsigned)(lmask >> 32);
      asm volatile("" : "+v"(cnt), "+v"(q_first), "+v"(q_second), "+v"(mlo), "+v"(mhi), "+v"(box.x), "+v"(box.y), "+v"(ra.x), "+v"(ra.y), "+v"(ra.z), "+v"(ra.w), "+v"(rb.x),
                   "+v"(rb.y), "+v"(rb.z), "+v"(rb.w), "+v"(rc.x), "+v"(rc.y), "+v"(rc.z), "+v"(rc.w), "+v"(rd.x), "+v"(rd.y), "+v"(rd.z), "+v"(rd.w));
      lmask = ((unsigned long long)mhi << 32) | mlo;
    }
    FaceRec r;
    unpack_face_rec(ra, rb, rc, rd, r);
    const int c0 = box.x & 0xffff, c1 = box.x >> 16, r0 = box.y & 0xffff, r1 = box.y >> 16;
    SMALFIT_WORK(if (c0 <= c1 + 70000) wb_t1 = __builtin_amdgcn_s_memtime();)
    if (c0 <= c1) {
      const float2* gp = gz + (size_t)n * S * S;
      const int bw = c1 - c0 + 1, npx = bw * (r1 - r0 + 1);
      // one (face, pixel) pair: adjoint seed, depth against the pixel's K-th nearest, distance maths, accumulate
      // (seed, K-th depth) of a pixel as ONE 8-byte load: left to itself the compiler fetches the depth only after the
      // branch on the seed -- a second dependent trip to L2 per pair
      // Pixel coordinates are carried as floats holding small integers exactly (round 4, like the forward sweep: conversions,
      // integer multiplies and 64-bit shift-adds issue at half the rate of float multiply-adds here): row / column from the
      // box-relative index by a multiply-add, a floor and a multiply-add, the pixel's byte offset by one more.
      const float bwf = (float)bw, ibw = __builtin_amdgcn_rcpf(bwf), hbw = 0.5f * ibw;
      const float r0f = (float)r0, c0f = (float)c0, s8 = 8.0f * (float)S;
      const float ndc_a = -2.0f * inv_s, ndc_b = 1.0f - inv_s;        // pix_to_ndc(i) = fma(i, ndc_a, ndc_b): the same bits
      auto load_seed = [&](float rowf, float colf) {
        const unsigned long long v = *reinterpret_cast<const unsigned long long*>(reinterpret_cast<const char*>(gp) + (unsigned)fmaf(rowf, s8, 8.0f * colf));
        return make_float2(__uint_as_float((unsigned)v), __uint_as_float((unsigned)(v >> 32)));
      };
      auto pair = [&](float rowf, float colf, const float2 g) {
        SMALFIT_WORK(++wb_vis; ++wb_trips; { const unsigned long long act = __ballot(1), lv = __ballot(g.x != 0.f);
                     if ((int)(threadIdx.x & 63) == __ffsll((long long)act) - 1) { ++wb_r; if (!lv) ++wb_deadr; } })
        if (g.x == 0.f) return;
        SMALFIT_WORK(++wb_live;)
        // depth first: it is five instructions and rejects the far side of the animal before the distance maths
        // (face_depth, as in face_pixel_eval, so the comparison agrees bitwise with the forward's)
        const float ppx = fmaf(colf, ndc_a, ndc_b), ppy = fmaf(rowf, ndc_a, ndc_b);
        if (face_pixel_depth(r, ppx, ppy) - zcn > g.y) return;           // not among the pixel's K nearest
        SMALFIT_WORK(++wb_eval;)
        PixEval e;
        if (!face_pixel_eval(r, ppx, ppy, e)) return;
        SMALFIT_WORK(++wb_in; { const float al = fabsf(g.x) / g_probe_seed_scale; wb_amax = fmaxf(wb_amax, al);
                     if (al < 2.4414e-4f) ++wb_a12; if (al < 5.96e-8f) ++wb_a24; if (al < 9.09e-13f) ++wb_a40; })
        // dL/dd = gpix * p ;  d = -+dist ;  d dist/d(u) = -2 q (1 - tc), d dist/d(w) = -2 q tc
        const float gd = g.x * prob_fast(e.d) * (e.inside ? -1.0f : 1.0f) * -2.0f;
        if constexpr (kUnclampedT) {
          // the nearest edge's parameter as the forward forms it, before the clamp (a degenerate edge keeps its end point: t = 1)
          const float ox = ppx - r.ax - ((e.edge == 2) ? r.e1x : 0.f), oy = ppy - r.ay - ((e.edge == 2) ? r.e1y : 0.f);
          const float ex = (e.edge == 0) ? r.e1x : ((e.edge == 1) ? r.e2x : r.e3x), ey = (e.edge == 0) ? r.e1y : ((e.edge == 1) ? r.e2y : r.e3y);
          const float il = (e.edge == 0) ? r.il1 : ((e.edge == 1) ? r.il2 : r.il3), t0 = (e.edge == 0) ? r.t01 : ((e.edge == 1) ? r.t02 : r.t03);
          e.tc = fmaf(fmaf(oy, ey, ox * ex), il, t0);
          e.qx = fmaf(-e.tc, ex, ox); e.qy = fmaf(-e.tc, ey, oy);
        }
        const float ku = 1.0f - e.tc, kw = e.tc;
        const float ca = (e.edge == 2) ? 0.f : ku;
        const float cb = (e.edge == 0) ? kw : ((e.edge == 2) ? ku : 0.f);
        const float cc = (e.edge == 0) ? 0.f : kw;
        const float gx = gd * e.qx, gy = gd * e.qy;
        ga[0] = fmaf(ca, gx, ga[0]); ga[1] = fmaf(ca, gy, ga[1]);
        gb[0] = fmaf(cb, gx, gb[0]); gb[1] = fmaf(cb, gy, gb[1]);
        gc[0] = fmaf(cc, gx, gc[0]); gc[1] = fmaf(cc, gy, gc[1]);
      };
      SMALFIT_WORK(if (sub == 0) { atomicAdd(&g_work[cnt <= kListCap ? 21 : (cnt == kMaskList ? 22 : 23)], 1ull); if (cnt == kNoList) atomicAdd(&g_work[24], (unsigned long long)npx); })
      // (one pixel per lane and round: requesting the seeds of 2 or 4 pixels per lane before the first pair is evaluated measured the
      // same within noise on both scenes -- the gather is bound by its rounds' instructions, not by the seed loads)
      auto coords = [&](float qf, float& rowf, float& colf) {
        const float ryf = floorf(fmaf(qf, ibw, hbw));    // q / bw: (q + 1/2) / bw is >= 1/2048 from any integer, the reciprocal good to 1 ulp
        rowf = r0f + ryf; colf = c0f + fmaf(-ryf, bwf, qf);
      };
      if (cnt <= kListCap) {
        // the forward sweep's compacted candidate list: box-relative pixel indices, 16 at a time
        for (int i = sub; i < cnt; i += kBwdLanes) {
          const float qf = (float)((i < kBwdLanes) ? q_first : ((i < 2 * kBwdLanes) ? q_second : (int)lst_n[lst_off + (unsigned)i]));
          float rowf, colf;
          coords(qf, rowf, colf);
          pair(rowf, colf, load_seed(rowf, colf));
        }
      } else if (cnt == kMaskList) {
        // the forward sweep's candidate masks: bit r of the lane's word = pixel 16 r + sub of the box
        while (lmask) {
          const float qf = (float)(((__ffsll((long long)lmask) - 1) * kBwdLanes) + sub);
          lmask &= lmask - 1ull;
          float rowf, colf;
          coords(qf, rowf, colf);
          pair(rowf, colf, load_seed(rowf, colf));
        }
      } else {
        // neither: the box's pixels in row-major order, 16 at a time, like the forward sweep
        const float npxf = (float)npx;
        for (float qf = (float)sub; qf < npxf; qf += (float)kBwdLanes) {
          float rowf, colf;
          coords(qf, rowf, colf);
          pair(rowf, colf, load_seed(rowf, colf));
        }
      }
    }
  }
  SMALFIT_WORK(const unsigned long long wb_t2 = __builtin_amdgcn_s_memtime();)
  // The six sums over the face's 16 lanes, as a reduce-scatter.  An xor butterfly (o = 8, 4, 2, 1) adds a + b in one partner and
  // b + a in the other, the same float: after every step all lanes of a coset hold one value, and only lane 0's was ever stored.
  // So a lane keeps the half of its values its side of the step owns and sends the other half -- 3, 2, 1, 1 exchanges instead of
  // 6 per step, every sum the same tree of the same additions -- and each sum ends in a lane of its own, which stores it:
  //   o = 8: bit 3 of the lane picks (ga0, ga1, gb0) or (gb1, gc0, gc1) as (x, y, z);  o = 4: x in both halves, bit 2 picks y or z
  //   as w;  o = 2: bit 1 picks x or w;  o = 1: the pair of lanes holds one sum.  Lanes 0, 2, 6 | 8, 10, 14 store dface[0..2 | 3..5]
  // (idle 16-lane groups of the last wave, and whole waves past the last frame, shuffle zeros among themselves and store nothing)
  {
    const bool b3 = sub & 8, b2 = sub & 4, b1 = sub & 2;
    float x = b3 ? gb[1] : ga[0], y = b3 ? gc[0] : ga[1], z = b3 ? gc[1] : gb[0];
    x += __shfl_xor(b3 ? ga[0] : gb[1], 8, 64);
    y += __shfl_xor(b3 ? ga[1] : gc[0], 8, 64);
    z += __shfl_xor(b3 ? gb[0] : gc[1], 8, 64);
    x += __shfl_xor(x, 4, 64);
    float w = b2 ? z : y;
    w += __shfl_xor(b2 ? y : z, 4, 64);
    float v = b1 ? w : x;
    v += __shfl_xor(b1 ? x : w, 2, 64);
    v += __shfl_xor(v, 1, 64);
    const int k = (b3 ? 3 : 0) + (b1 ? (b2 ? 2 : 1) : 0);
    if (f < F && (sub & 1) == 0 && (b1 || !b2))
      *reinterpret_cast<float*>(out_n + ((unsigned)f * (unsigned)(6 * sizeof(float)) + (unsigned)k * (unsigned)sizeof(float))) = v;
  }
  SMALFIT_WORK({ const int anylive = wb_live > 0 ? 1 : 0; int fl = anylive;
                 for (int o = 8; o > 0; o >>= 1) fl |= __shfl_xor(fl, o, 64);
                 const int wmax = wave_max_i(wb_trips);
                 work_add(8, wb_vis); work_add(9, wb_live); work_add(10, wb_eval); work_add(11, wb_in);
                 work_add(12, (threadIdx.x & 63) == 0 ? wmax : 0); work_add(13, wb_r); work_add(14, wb_deadr);
                 work_add(15, (sub == 0 && f < F) ? fl : 0); work_add(16, (sub == 0 && f < F) ? 1 : 0);
                 for (int o = 8; o > 0; o >>= 1) wb_amax = fmaxf(wb_amax, __shfl_xor(wb_amax, o, 64));
                 work_add(17, wb_a12); work_add(18, wb_a24); work_add(19, wb_a40);
                 work_add(29, (sub == 0 && f < F && wb_amax < 5.96e-8f) ? 1 : 0); work_add(30, (sub == 0 && f < F && wb_amax < 2.4414e-4f) ? 1 : 0);
                 if ((threadIdx.x & 63) == 0) { const unsigned long long wb_t3 = __builtin_amdgcn_s_memtime();
                   atomicAdd(&g_work[25], wb_t1 - wb_t0); atomicAdd(&g_work[26], wb_t2 - wb_t1); atomicAdd(&g_work[27], wb_t3 - wb_t2);
                   atomicAdd(&g_work[28], 1ull); } })
}

// smalfit_render_backward only.  d(sil)/d(world verts): gather incident-face adjoints, camera adjoint, write interleaved (M,V,3)
__global__ void raster_vertex_grad_kernel(ModelDev m, const float* __restrict__ proj, const float* __restrict__ dface,
                                          float* __restrict__ dverts) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x, n = blockIdx.y;
  if (v >= m.V) return;
  float gxn = 0.f, gyn = 0.f;
  const float* df = dface + (size_t)n * m.F * 6;
  for (int i = m.vf_off[v]; i < m.vf_off[v + 1]; ++i) {
    gxn += df[m.vf_idx[i] * 2];
    gyn += df[m.vf_idx[i] * 2 + 1];
  }
  const float* pv = proj + (size_t)n * 3 * m.Vp;
  float g[3];
  world_to_ndc_bwd(pv[v], pv[m.Vp + v], pv[2 * m.Vp + v], gxn, gyn, g[0], g[1], g[2]);
  float* o = dverts + ((size_t)n * m.V + v) * 3;
  o[0] = g[0]; o[1] = g[1]; o[2] = g[2];
}
