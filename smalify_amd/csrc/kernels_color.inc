// hard-Phong colour render for visualisation (K5') -- part of smalfit_kernels.hip (included inside namespace smalfit; not a translation unit of its own)

// ------------------------------------------------------------------------------------------------
// K5': colour render for visualisation (p3d_renderer.py:41-59,70-72: blur_radius 0, faces_per_pixel 1, HardPhongShader,
// one point light at (0,0,3), constant vertex colour, white background).  Not on the optimisation path.
//   vnormal_kernel      pytorch3d Meshes.verts_normals_packed (area-weighted incident face normals, normalised)
//   color_zbuf_kernel   face-parallel z-buffer: (order-preserving depth key << 32 | face) with one 64-bit atomicMin
//   color_shade_kernel  thread per pixel: screen-space barycentrics of the winning face, Phong terms
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
vnormal_kernel(ModelDev m, int M, const float* __restrict__ verts /*[M][3][Vp] world*/, float* __restrict__ vn /*[M][3][Vp]*/) {
  const int v = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y, Vp = m.Vp;
  if (v >= Vp) return;
  const float* p = verts + (size_t)n * 3 * Vp;
  float acc[3] = {0.f, 0.f, 0.f};
  if (v < m.V) {
    for (int i = m.vf_off[v]; i < m.vf_off[v + 1]; ++i) {
      const int f = m.vf_idx[i] / 3;
      const int i0 = m.faces[f * 3], i1 = m.faces[f * 3 + 1], i2 = m.faces[f * 3 + 2];
      const float ux = p[i1] - p[i0], uy = p[Vp + i1] - p[Vp + i0], uz = p[2 * Vp + i1] - p[2 * Vp + i0];
      const float wx = p[i2] - p[i0], wy = p[Vp + i2] - p[Vp + i0], wz = p[2 * Vp + i2] - p[2 * Vp + i0];
      acc[0] += uy * wz - uz * wy; acc[1] += uz * wx - ux * wz; acc[2] += ux * wy - uy * wx;
    }
    const float inv = 1.0f / fmaxf(sqrtf(acc[0] * acc[0] + acc[1] * acc[1] + acc[2] * acc[2]), 1e-6f);
    acc[0] *= inv; acc[1] *= inv; acc[2] *= inv;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) vn[((size_t)n * 3 + a) * Vp + v] = acc[a];
}

// The hard rasterisation both entry points share (smalfit_render_color, smalfit_fit_metrics), so that the collage and the score
// cannot drift apart: lane `sub` of the 16 that take face f walks the face's pixel box, clipped to the image, and calls
// hit(row, col, e) at every pixel whose centre the face covers (blur_radius 0: inside, in front of the camera)
template <class Hit>
__device__ __forceinline__ void face_box_walk(const ModelDev& m, int S, const float* __restrict__ px /*[3][Vp] of the frame*/, int f, int sub, Hit hit) {
  const int Vp = m.Vp;
  const int i0 = m.faces[f * 3], i1 = m.faces[f * 3 + 1], i2 = m.faces[f * 3 + 2];
  const float ax = px[i0], ay = px[Vp + i0], az = px[2 * Vp + i0];
  const float bx = px[i1], by = px[Vp + i1], bz = px[2 * Vp + i1];
  const float cx = px[i2], cy = px[Vp + i2], cz = px[2 * Vp + i2];
  FaceRec r;
  if (!make_face_rec(ax, ay, az, bx, by, bz, cx, cy, cz, r)) return;
  const float xlo = fminf(ax, fminf(bx, cx)), xhi = fmaxf(ax, fmaxf(bx, cx));
  const float ylo = fminf(ay, fminf(by, cy)), yhi = fmaxf(ay, fmaxf(by, cy));
  if (!(xlo == xlo && xhi == xhi && ylo == ylo && yhi == yhi) || xhi < -1.0f || xlo > 1.0f || yhi < -1.0f || ylo > 1.0f) return;
  const float fs = (float)S;
  const int c0 = (int)fminf(fmaxf(floorf(((1.0f - xhi) * fs - 1.0f) * 0.5f), 0.f), fs - 1.f);
  const int c1 = (int)fminf(fmaxf(ceilf(((1.0f - xlo) * fs - 1.0f) * 0.5f), 0.f), fs - 1.f);
  const int r0 = (int)fminf(fmaxf(floorf(((1.0f - yhi) * fs - 1.0f) * 0.5f), 0.f), fs - 1.f);
  const int r1 = (int)fminf(fmaxf(ceilf(((1.0f - ylo) * fs - 1.0f) * 0.5f), 0.f), fs - 1.f);
  const int bw = c1 - c0 + 1, npx = bw * (r1 - r0 + 1);
  const float inv_s = 1.0f / fs;
  for (int q = sub; q < npx; q += 16) {
    const int row = r0 + q / bw, col = c0 + q % bw;
    PixEval e;
    if (!face_pixel_eval(r, pix_to_ndc(col, inv_s), pix_to_ndc(row, inv_s), e) || !e.inside) continue;
    hit(row, col, e);
  }
}

__global__ void __launch_bounds__(256)
color_zbuf_kernel(ModelDev m, int S, const float* __restrict__ proj, unsigned long long* __restrict__ zbuf /*[M][S*S], preset to ~0*/) {
  const int n = blockIdx.y, f = blockIdx.x * 16 + (threadIdx.x >> 4), sub = threadIdx.x & 15;
  if (f >= m.F) return;
  unsigned long long* zb = zbuf + (size_t)n * S * S;
  face_box_walk(m, S, proj + (size_t)n * 3 * m.Vp, f, sub, [&](int row, int col, const PixEval& e) {
    atomicMin(&zb[row * S + col], ((unsigned long long)orderable(e.pz) << 32) | (unsigned)f);
  });
}

__global__ void __launch_bounds__(256)
color_shade_kernel(ModelDev m, int S, const float* __restrict__ proj, const float* __restrict__ verts /*[M][3][Vp] world*/,
                   const float* __restrict__ vn, const unsigned long long* __restrict__ zbuf, float cr, float cg, float cb,
                   float* __restrict__ image /*[M][3][S][S]*/) {
  const int pix = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y, Vp = m.Vp;
  if (pix >= S * S) return;
  float rgb[3] = {1.0f, 1.0f, 1.0f};                       // BlendParams default background
  const unsigned long long key = zbuf[(size_t)n * S * S + pix];
  if (key != ~0ull) {
    const int f = (int)(key & 0xffffffffull);
    const int idx[3] = {m.faces[f * 3], m.faces[f * 3 + 1], m.faces[f * 3 + 2]};
    const float* px = proj + (size_t)n * 3 * Vp;
    FaceRec r;
    make_face_rec(px[idx[0]], px[Vp + idx[0]], px[2 * Vp + idx[0]], px[idx[1]], px[Vp + idx[1]], px[2 * Vp + idx[1]],
                  px[idx[2]], px[Vp + idx[2]], px[2 * Vp + idx[2]], r);
    const float inv_s = 1.0f / (float)S;
    const float dx = pix_to_ndc(pix % S, inv_s) - r.ax, dy = pix_to_ndc(pix / S, inv_s) - r.ay;
    const float c1 = fmaf(dx, r.e1y, -(dy * r.e1x)), c2 = fmaf(dx, r.e2y, -(dy * r.e2x));
    const float w[3] = {((c2 - c1) + r.area) * r.inv_den, -c2 * r.inv_den, c1 * r.inv_den};
    const float* pw = verts + (size_t)n * 3 * Vp;
    const float* pn = vn + (size_t)n * 3 * Vp;
    float pos[3] = {0.f, 0.f, 0.f}, nr[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int a = 0; a < 3; ++a) { pos[a] = fmaf(w[k], pw[a * Vp + idx[k]], pos[a]); nr[a] = fmaf(w[k], pn[a * Vp + idx[k]], nr[a]); }
    const float inn = 1.0f / fmaxf(sqrtf(nr[0] * nr[0] + nr[1] * nr[1] + nr[2] * nr[2]), 1e-6f);
    nr[0] *= inn; nr[1] *= inn; nr[2] *= inn;
    float ld[3] = {0.0f - pos[0], 0.0f - pos[1], 3.0f - pos[2]};           // PointLights(location = (0, 0, 3))
    const float inl = 1.0f / fmaxf(sqrtf(ld[0] * ld[0] + ld[1] * ld[1] + ld[2] * ld[2]), 1e-6f);
    ld[0] *= inl; ld[1] *= inl; ld[2] *= inl;
    const float cosang = nr[0] * ld[0] + nr[1] * ld[1] + nr[2] * ld[2];
    const float diffuse = 0.3f * fmaxf(cosang, 0.f);
    float vd[3] = {0.0f - pos[0], 0.0f - pos[1], kCamDist - pos[2]};       // camera centre
    const float inv_v = 1.0f / fmaxf(sqrtf(vd[0] * vd[0] + vd[1] * vd[1] + vd[2] * vd[2]), 1e-6f);
    float va = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) va += vd[a] * inv_v * (-ld[a] + 2.0f * cosang * nr[a]);
    const float alpha = (cosang > 0.f) ? fmaxf(va, 0.f) : 0.f;
    const float spec = 0.2f * powf(alpha, 64.0f);
    const float amb = 0.5f + diffuse;
    rgb[0] = amb * cr + spec; rgb[1] = amb * cg + spec; rgb[2] = amb * cb + spec;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) image[((size_t)n * 3 + a) * S * S + pix] = rgb[a];
}

// ------------------------------------------------------------------------------------------------
// smalfit_fit_metrics: hard coverage, its overlap with the target silhouette, keypoint distances (include/smalfit.h holds the
// definitions; no counterpart in the reference)
//   cover_kernel        color_zbuf_kernel's walk without depth: a covered pixel gets a plain byte store of 1 (every writer stores
//                       the same value: no atomic, no dependence on the order)
//   sil_counts_kernel   pixels in mask & target, mask | target, mask, target per frame: integer adds, the same bits in any order
//   pck_kernel          one wave per frame: lane k's keypoint distance over sqrt(target pixels), counts by ballot
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
cover_kernel(ModelDev m, int S, const float* __restrict__ proj, unsigned char* __restrict__ mask /*[M][S*S], preset to 0*/) {
  const int n = blockIdx.y, f = blockIdx.x * 16 + (threadIdx.x >> 4), sub = threadIdx.x & 15;
  if (f >= m.F) return;
  unsigned char* mk = mask + (size_t)n * S * S;
  face_box_walk(m, S, proj + (size_t)n * 3 * m.Vp, f, sub, [&](int row, int col, const PixEval&) { mk[row * S + col] = 1; });
}

// the four counters of one pixel pair / of four pixels a byte each (mask bytes are 0 / 1, target bytes on from 128)
struct SilCounts {
  unsigned c[4];
  __device__ void pixel(unsigned m, bool t) { c[0] += m & (unsigned)t; c[1] += m | (unsigned)t; c[2] += m; c[3] += (unsigned)t; }
  __device__ void word(unsigned mw, unsigned tbits /*bit 0 of each byte*/) {
    c[0] += __popc(mw & tbits); c[1] += __popc(mw | tbits); c[2] += __popc(mw); c[3] += __popc(tbits);
  }
};
__device__ __forceinline__ bool sil_target_on(float t) { return t > 0.5f; }
__device__ __forceinline__ bool sil_target_on(unsigned char b) { return b >= 128; }
__device__ __forceinline__ unsigned sil_target_bits(float a, float b, float c, float d) {
  return (unsigned)sil_target_on(a) | ((unsigned)sil_target_on(b) << 8) | ((unsigned)sil_target_on(c) << 16) | ((unsigned)sil_target_on(d) << 24);
}

// Grid (sil_count_slabs(S), M), 256 threads.  A frame's pixels start at byte n S^2 of the mask, which is no multiple of 16 when S is
// odd: the frame is [head: up to the mask's next 16-byte boundary | chunks of kSilCountPixels pixels, one 16-byte read of the mask
// each | tail].  The target's chunk is read as one 16-byte word (bytes) / four (floats) when the caller's pointer happens to be
// aligned with the mask's, pixel by pixel otherwise.  Head and tail: at most 15 pixels each, taken by slab 0's first 32 threads.
template <class T>
__global__ void __launch_bounds__(256)
sil_counts_kernel(int S, const unsigned char* __restrict__ mask, const T* __restrict__ target, unsigned* __restrict__ counts /*[M][4], preset to 0*/) {
  static_assert(kSilCountPixels == 16, "a chunk is one 16-byte read of the mask");
  const int n = blockIdx.y, npx = S * S, tid = threadIdx.x;
  const unsigned char* mk = mask + (size_t)n * npx;
  const T* tg = target + (size_t)n * npx;
  const int head = min(npx, (int)((16u - (unsigned)((uintptr_t)mk & 15u)) & 15u));
  const int nchunk = (npx - head) / 16, tail0 = head + nchunk * 16;
  const bool aligned = ((uintptr_t)(tg + head) & 15u) == 0;            // uniform over the block
  SilCounts k = {{0u, 0u, 0u, 0u}};
  for (int c = blockIdx.x * 256 + tid; c < nchunk; c += gridDim.x * 256) {
    const int p = head + c * 16;
    const uint4 mw = *reinterpret_cast<const uint4*>(mk + p);
    if (aligned) {
      if constexpr (sizeof(T) == 1) {
        const uint4 tw = *reinterpret_cast<const uint4*>(tg + p);
        k.word(mw.x, (tw.x >> 7) & 0x01010101u); k.word(mw.y, (tw.y >> 7) & 0x01010101u);
        k.word(mw.z, (tw.z >> 7) & 0x01010101u); k.word(mw.w, (tw.w >> 7) & 0x01010101u);
      } else {
        const float4* tf = reinterpret_cast<const float4*>(tg + p);
        const float4 a = tf[0], b = tf[1], cc = tf[2], d = tf[3];
        k.word(mw.x, sil_target_bits(a.x, a.y, a.z, a.w)); k.word(mw.y, sil_target_bits(b.x, b.y, b.z, b.w));
        k.word(mw.z, sil_target_bits(cc.x, cc.y, cc.z, cc.w)); k.word(mw.w, sil_target_bits(d.x, d.y, d.z, d.w));
      }
    } else {
      const unsigned w[4] = {mw.x, mw.y, mw.z, mw.w};
#pragma unroll
      for (int i = 0; i < 16; ++i) k.pixel((w[i >> 2] >> (8 * (i & 3))) & 1u, sil_target_on(tg[p + i]));
    }
  }
  if (blockIdx.x == 0 && tid < 32) {
    const int p = tid < 16 ? (tid < head ? tid : -1) : (tail0 + tid - 16 < npx ? tail0 + tid - 16 : -1);
    if (p >= 0) k.pixel(mk[p] & 1u, sil_target_on(tg[p]));
  }
  __shared__ unsigned part[4][4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    unsigned v = k.c[q];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((tid & 63) == 0) part[tid >> 6][q] = v;
  }
  __syncthreads();
  if (tid < 4) atomicAdd(&counts[n * 4 + tid], part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid]);
}

struct PckThresholds { float t[SMALFIT_MAX_PCK_THRESHOLDS]; };
// Grid M, one wave.  Stream-ordered after sil_counts_kernel: counts[n][3] is the frame's target pixels
__global__ void __launch_bounds__(64)
pck_kernel(const float* __restrict__ proj /*[M][25][2]*/, const float* __restrict__ target /*[M][25][2]*/, const float* __restrict__ visibility /*[M][25]*/,
           const unsigned* __restrict__ counts, int T, PckThresholds thr, float* __restrict__ dist_out /*[M][25] or null*/,
           int* __restrict__ pck /*[M][1 + T] or null*/) {
  const int n = blockIdx.x, k = threadIdx.x;
  const bool lane = k < SMALFIT_NUM_KEYPOINTS;
  float dist = 0.f;
  bool visible = false;
  if (lane) {
    const int i = n * SMALFIT_NUM_KEYPOINTS + k;
    const unsigned area = counts[n * 4 + 3];
    dist = area ? hypotf(proj[2 * i] - target[2 * i], proj[2 * i + 1] - target[2 * i + 1]) / sqrtf((float)area) : __builtin_inff();
    visible = visibility[i] > 0.f;
    if (dist_out) dist_out[i] = dist;
  }
  if (!pck) return;
  const int nvis = __popcll(__ballot(visible));
  if (k == 0) pck[n * (1 + T)] = nvis;
  for (int t = 0; t < T; ++t) {
    const int ok = __popcll(__ballot(visible && dist <= thr.t[t]));
    if (k == 0) pck[n * (1 + T) + 1 + t] = ok;
  }
}

