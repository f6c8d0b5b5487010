// Live-session kernels: the launches that bracket the captured frame graph when frames arrive one at a time from a
// camera (codd_amd/live.py).  Ingest and depth export are pure streaming kernels: no LDS, several pixels per thread,
// 16-byte stores, a scalar tail; the motion export moves 28-byte and 8- / 12-byte records and stages them in LDS.
// All run on the compute stream outside the graph.
#include "common.h"
#include "se3.h"

// ------------------------------------------------------------------------------------------------
// codd_ingest_pair: both views of one frame, uint8 HWC -> normalised reflect-padded fp32 CHW, optionally through a
// rectifying bilinear remap (reference datasets/transforms.py:147-161 Pad, :373-427 Normalize,
// datasets/formating.py:65-85, applied to img and r_img by datasets/custom_stereo_mf.py; the remap is the
// cv2.remap(INTER_LINEAR, BORDER_CONSTANT 0) a user of the reference runs on the host before either).
// ------------------------------------------------------------------------------------------------
struct IngestArgs {
  const unsigned char* img[2];
  const float* mx[2];
  const float* my[2];
  float* out[2];
  int h, w, H, W, bgr;
  float m0, m1, m2, s0, s1, s2;
};

#define INGEST_PX 4  // output pixels per thread: one 16-byte store per channel row, 12 source bytes = 3 dwords

// raw (un-normalised) channel values of rectified pixel (y, x) of the h x w image, in source channel order
__device__ __forceinline__ void ingest_sample(const unsigned char* __restrict__ img, const float* __restrict__ mx,
                                              const float* __restrict__ my, int h, int w, int y, int x, float* c) {
  const size_t o = (size_t)y * w + x;
  if (!mx) {
    const unsigned char* p = img + o * 3;
    c[0] = p[0]; c[1] = p[1]; c[2] = p[2];
    return;
  }
  const float sx = mx[o], sy = my[o];
  c[0] = c[1] = c[2] = 0.f;
  // every tap outside (this also catches NaN and +-inf: the comparisons are false) -> 0
  if (!(sx > -1.f && sx < (float)w && sy > -1.f && sy < (float)h)) return;
  const float fx0 = floorf(sx), fy0 = floorf(sy);
  const float ax = sx - fx0, ay = sy - fy0;
  const int x0 = (int)fx0, y0 = (int)fy0;
  const bool xin0 = x0 >= 0, xin1 = x0 + 1 < w, yin0 = y0 >= 0, yin1 = y0 + 1 < h;
  const unsigned char* p00 = img + ((ptrdiff_t)y0 * w + x0) * 3;
  const unsigned char* p10 = p00 + (ptrdiff_t)w * 3;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float v00 = (yin0 && xin0) ? (float)p00[k] : 0.f, v01 = (yin0 && xin1) ? (float)p00[3 + k] : 0.f;
    const float v10 = (yin1 && xin0) ? (float)p10[k] : 0.f, v11 = (yin1 && xin1) ? (float)p10[3 + k] : 0.f;
    const float top = v00 * (1.f - ax) + v01 * ax, bot = v10 * (1.f - ax) + v11 * ax;
    c[k] = top * (1.f - ay) + bot * ay;
  }
}

__global__ __launch_bounds__(256) void ingest_pair_kernel(IngestArgs a) {
  const int v = blockIdx.y;
  const unsigned char* __restrict__ img = a.img[v];
  const float* __restrict__ mx = a.mx[v];
  const float* __restrict__ my = a.my[v];
  float* __restrict__ out = a.out[v];
  const int h = a.h, w = a.w, H = a.H, W = a.W;
  const int W4 = (W + INGEST_PX - 1) / INGEST_PX;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)H * W4) return;
  const int y = (int)(t / W4), x4 = (int)(t - (long long)y * W4) * INGEST_PX;
  const int sy = y < h ? y : 2 * (h - 1) - y;  // reflect without edge repeat (cv2.BORDER_REFLECT_101)
  float c[INGEST_PX][3];
  bool loaded = false;
  if (!mx && x4 + INGEST_PX <= w && ((uintptr_t)img & 3) == 0) {
    // map-free interior: the 12 bytes of 4 packed pixels as dwords.  A row start is dword-aligned only when
    // sy * w is a multiple of 4, so read the aligned dwords around them and shift by the byte misalignment.
    const size_t off = ((size_t)sy * w + x4) * 3, total = (size_t)h * w * 3;
    const unsigned sh = (unsigned)(off & 3);
    const size_t a0 = off - sh;
    if (sh == 0 || a0 + 16 <= total) {  // (the 4th dword must lie inside the image)
      const unsigned* q = (const unsigned*)(img + a0);
      const unsigned d0 = q[0], d1 = q[1], d2 = q[2], d3 = sh ? q[3] : 0u;
      const unsigned s8 = sh * 8;
      const unsigned r0 = (unsigned)((((unsigned long long)d1 << 32) | d0) >> s8);
      const unsigned r1 = (unsigned)((((unsigned long long)d2 << 32) | d1) >> s8);
      const unsigned r2 = (unsigned)((((unsigned long long)d3 << 32) | d2) >> s8);
      c[0][0] = (float)(r0 & 255u); c[0][1] = (float)((r0 >> 8) & 255u); c[0][2] = (float)((r0 >> 16) & 255u);
      c[1][0] = (float)(r0 >> 24); c[1][1] = (float)(r1 & 255u); c[1][2] = (float)((r1 >> 8) & 255u);
      c[2][0] = (float)((r1 >> 16) & 255u); c[2][1] = (float)(r1 >> 24); c[2][2] = (float)(r2 & 255u);
      c[3][0] = (float)((r2 >> 8) & 255u); c[3][1] = (float)((r2 >> 16) & 255u); c[3][2] = (float)(r2 >> 24);
      loaded = true;
    }
  }
  if (!loaded) {
#pragma unroll
    for (int i = 0; i < INGEST_PX; ++i) {
      const int x = x4 + i;
      if (x < W) {
        const int sx = x < w ? x : 2 * (w - 1) - x;
        ingest_sample(img, mx, my, h, w, sy, sx, c[i]);
      } else {
        c[i][0] = c[i][1] = c[i][2] = 0.f;
      }
    }
  }
  const size_t N = (size_t)H * W, o = (size_t)y * W + x4;
  const float m0 = a.m0, m1 = a.m1, m2 = a.m2, s0 = a.s0, s1 = a.s1, s2 = a.s2;
  f32x4 r0, r1, r2;
#pragma unroll
  for (int i = 0; i < INGEST_PX; ++i) {
    const float c0 = a.bgr ? c[i][2] : c[i][0], c1 = c[i][1], c2 = a.bgr ? c[i][0] : c[i][2];
    r0[i] = (c0 - m0) / s0; r1[i] = (c1 - m1) / s1; r2[i] = (c2 - m2) / s2;  // preprocess_kernel's expression
  }
  if ((W & 3) == 0 && ((uintptr_t)out & 15) == 0) {  // (then x4 + 4 <= W and every row / plane offset is 16-byte aligned)
    *(f32x4*)(out + o) = r0; *(f32x4*)(out + N + o) = r1; *(f32x4*)(out + 2 * N + o) = r2;
  } else {
#pragma unroll
    for (int i = 0; i < INGEST_PX; ++i)
      if (x4 + i < W) { out[o + i] = r0[i]; out[N + o + i] = r1[i]; out[2 * N + o + i] = r2[i]; }
  }
}

extern "C" int codd_ingest_pair(const unsigned char* left, const unsigned char* right, int h, int w, int bgr,
                                const float* mean, const float* stdv, const float* lmap_x, const float* lmap_y,
                                const float* rmap_x, const float* rmap_y, int H, int W, float* out_left,
                                float* out_right, void* stream) {
  if (!left || !right || !mean || !stdv || !out_left || !out_right) return CODD_EINVAL;
  if (h <= 0 || w <= 0 || H < h || W < w || H - h >= h || W - w >= w) return CODD_EINVAL;
  if ((lmap_x == nullptr) != (lmap_y == nullptr) || (rmap_x == nullptr) != (rmap_y == nullptr)) return CODD_EINVAL;
  IngestArgs a;
  a.img[0] = left; a.img[1] = right;
  a.mx[0] = lmap_x; a.my[0] = lmap_y; a.mx[1] = rmap_x; a.my[1] = rmap_y;
  a.out[0] = out_left; a.out[1] = out_right;
  a.h = h; a.w = w; a.H = H; a.W = W; a.bgr = bgr;
  a.m0 = mean[0]; a.m1 = mean[1]; a.m2 = mean[2]; a.s0 = stdv[0]; a.s1 = stdv[1]; a.s2 = stdv[2];
  const long long threads = (long long)H * cdiv(W, INGEST_PX);
  ingest_pair_kernel<<<dim3(cdiv(threads, 256), 2), 256, 0, (hipStream_t)stream>>>(a);
  CODD_LAUNCH_CHECK();
  return CODD_OK;
}

// ------------------------------------------------------------------------------------------------
// codd_export_depth: the frame's padded disparity -> the cropped result in the caller's staging buffer (reference
// model/codd.py:370-377: `pred_disp = calib / pred_disp` under reciprocal, then the [:img_h, :img_w] crop; mode 2 is the
// KITTI devkit's uint16 PNG convention, disparity * 256).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float export_value(float d, int mode, float calib) {
  // torch evaluates `scalar / tensor` as tensor.reciprocal() * scalar: the same two roundings, so that the session's
  // depth carries the bits of estimator.inference(reciprocal=True)
  if (mode == CODD_EXPORT_DEPTH) return (1.f / d) * calib;
  if (mode == CODD_EXPORT_DISP_U16) {
    if (!(fabsf(d) < INFINITY)) return 0.f;  // NaN, +-inf
    return fminf(fmaxf(rintf(d * 256.f), 0.f), 65535.f);  // rintf: round to nearest even
  }
  return d;
}

__global__ __launch_bounds__(256) void export_depth_kernel(const float* __restrict__ disp, int W, int h, int w, int mode,
                                                           float calib, void* __restrict__ out) {
  const long long n = (long long)h * w;
  const long long i0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i0 >= n) return;
  int y = (int)(i0 / w), x = (int)(i0 - (long long)y * w);
  float v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[i] = (i0 + i < n) ? export_value(disp[(size_t)y * W + x], mode, calib) : 0.f;
    if (++x == w) { x = 0; ++y; }
  }
  const bool full = i0 + 4 <= n;
  if (mode == CODD_EXPORT_DISP_U16) {
    unsigned short* o = (unsigned short*)out + i0;
    if (full && ((uintptr_t)out & 7) == 0) {
      uint2 p;
      p.x = (unsigned)v[0] | ((unsigned)v[1] << 16);
      p.y = (unsigned)v[2] | ((unsigned)v[3] << 16);
      *(uint2*)o = p;
    } else {
      for (int i = 0; i < 4 && i0 + i < n; ++i) o[i] = (unsigned short)v[i];
    }
  } else {
    float* o = (float*)out + i0;
    if (full && ((uintptr_t)out & 15) == 0) {
      f32x4 p = {v[0], v[1], v[2], v[3]};
      *(f32x4*)o = p;
    } else {
      for (int i = 0; i < 4 && i0 + i < n; ++i) o[i] = v[i];
    }
  }
}

extern "C" int codd_export_depth(const float* disp, int H, int W, int h, int w, int mode, float calib, void* out,
                                 void* stream) {
  if (!disp || !out || h <= 0 || w <= 0 || H < h || W < w) return CODD_EINVAL;
  if (mode != CODD_EXPORT_DISP && mode != CODD_EXPORT_DEPTH && mode != CODD_EXPORT_DISP_U16) return CODD_EINVAL;
  const long long threads = ((long long)h * w + 3) / 4;
  export_depth_kernel<<<cdiv(threads, 256), 256, 0, (hipStream_t)stream>>>(disp, W, h, w, mode, calib, out);
  CODD_LAUNCH_CHECK();
  return CODD_OK;
}

// ------------------------------------------------------------------------------------------------
// codd_export_motion: the frame's up-sampled SE3 field -> per-pixel optical flow / flow + disparity change / 3-D scene
// flow on the previous frame's grid, cropped, in the caller's staging buffer; and the roll of the session's depth map
// (reference projective_ops.py:55-68 induced_flow, raft3d.py:268-270, motion.py:154-165 disparity -> depth,
// model/codd.py:519-575 the quantities the scene-flow metrics read).
// A workgroup owns MOTION_RUN consecutive pixels of one row.  Their T records (28 bytes each) are one contiguous
// span of memory and so are their output records (8 or 12 bytes): both pass through LDS and cross the memory
// interface as 16-byte accesses, with a scalar head and tail where the span does not start or end on a 16-byte
// boundary.  The LDS copy of a span starts at the span's own phase inside its 16-byte line, so that aligned global
// accesses are aligned LDS accesses too.  Lanes read their record at a 7-float stride (odd: conflict-free).
// ------------------------------------------------------------------------------------------------
#define MOTION_RUN 256

// floats [0, n) of a span: g -> s (TO_LDS) or s -> g, s already offset to g's phase: ((g - s) & 15) == 0 in bytes
template <bool TO_LDS>
__device__ __forceinline__ void motion_span_copy(float* __restrict__ g, float* __restrict__ s, int n) {
  const int head = min(n, (int)((4u - (unsigned)(((uintptr_t)g >> 2) & 3u)) & 3u));
  const int nv = (n - head) >> 2, tail0 = head + 4 * nv;
  for (int i = threadIdx.x; i < nv; i += MOTION_RUN) {
    if (TO_LDS) *(f32x4*)(s + head + 4 * i) = *(const f32x4*)(g + head + 4 * i);
    else *(f32x4*)(g + head + 4 * i) = *(const f32x4*)(s + head + 4 * i);
  }
  // (at most 3 + 3 floats)
  const int t = threadIdx.x;
  if (t < head) { if (TO_LDS) s[t] = g[t]; else g[t] = s[t]; }
  if (t >= 64 && t - 64 < n - tail0) { if (TO_LDS) s[tail0 + t - 64] = g[tail0 + t - 64]; else g[tail0 + t - 64] = s[tail0 + t - 64]; }
}

template <int MODE>
__global__ __launch_bounds__(MOTION_RUN) void export_motion_kernel(const float* __restrict__ T,
                                                                   const float* __restrict__ disp_cur,
                                                                   float* __restrict__ depth_prev, int W, int w, float fx,
                                                                   float fy, float cx, float cy, float bf, float scale,
                                                                   float* __restrict__ out) {
  constexpr int C = MODE == CODD_MOTION_FLOW2D ? 2 : 3;
  __shared__ __attribute__((aligned(16))) float sT[MOTION_RUN * 7 + 4];
  __shared__ __attribute__((aligned(16))) float sO[MOTION_RUN * C + 4];
  const int y = blockIdx.y, x0 = blockIdx.x * MOTION_RUN, x = x0 + (int)threadIdx.x;
  const int nv = min(MOTION_RUN, w - x0);  // pixels of this run (>= 1 by the grid)
  const size_t p0 = (size_t)y * W + x0;
  const bool in = (int)threadIdx.x < nv;
  // the two per-pixel planes: one dword per lane, consecutive lanes on consecutive addresses
  float dprev = 0.f, dcur = 0.f;
  if (in) { dprev = depth_prev[p0 + threadIdx.x]; dcur = disp_cur[p0 + threadIdx.x]; }
  if (T) {
    float* gT = const_cast<float*>(T) + p0 * 7;
    float* gO = out + ((size_t)y * w + x0) * C;
    float* lT = sT + (((uintptr_t)gT >> 2) & 3);
    float* lO = sO + (((uintptr_t)gO >> 2) & 3);
    motion_span_copy<true>(gT, lT, nv * 7);
    __syncthreads();
    if (in) {
      const V3 X0 = inv_project(dprev, x, y, fx, fy, cx, cy);
      const V3 X1 = se3_act(se3_load(lT + threadIdx.x * 7), X0);
      float r[3];
      if (MODE == CODD_MOTION_SCENEFLOW) {
        r[0] = scale * (X1.x - X0.x); r[1] = scale * (X1.y - X0.y); r[2] = scale * (X1.z - X0.z);
      } else {
        const V3 a = project(X1, fx, fy, cx, cy), c = project(X0, fx, fy, cx, cy);
        r[0] = a.x - c.x; r[1] = a.y - c.y; r[2] = bf * (a.z - c.z);
      }
      const bool valid = X0.z >= MIN_DEPTH && X1.z >= MIN_DEPTH;  // (NaN compares false)
#pragma unroll
      for (int k = 0; k < C; ++k) lO[threadIdx.x * C + k] = valid ? r[k] : NAN;
    }
    __syncthreads();
    motion_span_copy<false>(gO, lO, nv * C);
  }
  // the roll: this lane has read its element; disp_to_depth_kernel's expression
  if (in) depth_prev[p0 + threadIdx.x] = fminf(fmaxf(bf / (dcur + 1e-5f), 0.f), 210.f);
}

extern "C" int codd_export_motion(const float* T, const float* disp_cur, float* depth_prev, int H, int W, int h, int w,
                                  int mode, float fx, float fy, float cx, float cy, float bf, float scale, float* out,
                                  void* stream) {
  if (!disp_cur || !depth_prev || (T && !out)) return CODD_EINVAL;
  if (H <= 0 || W <= 0 || h <= 0 || w <= 0 || h > H || w > W) return CODD_EINVAL;
  if (mode != CODD_MOTION_FLOW2D && mode != CODD_MOTION_FLOW_DD && mode != CODD_MOTION_SCENEFLOW) return CODD_EINVAL;
  if (!(bf > 0.f)) return CODD_EINVAL;
  const dim3 grid(cdiv(w, MOTION_RUN), h);
  hipStream_t s = (hipStream_t)stream;
  if (mode == CODD_MOTION_FLOW2D)
    export_motion_kernel<CODD_MOTION_FLOW2D><<<grid, MOTION_RUN, 0, s>>>(T, disp_cur, depth_prev, W, w, fx, fy, cx, cy, bf, scale, out);
  else if (mode == CODD_MOTION_FLOW_DD)
    export_motion_kernel<CODD_MOTION_FLOW_DD><<<grid, MOTION_RUN, 0, s>>>(T, disp_cur, depth_prev, W, w, fx, fy, cx, cy, bf, scale, out);
  else
    export_motion_kernel<CODD_MOTION_SCENEFLOW><<<grid, MOTION_RUN, 0, s>>>(T, disp_cur, depth_prev, W, w, fx, fy, cx, cy, bf, scale, out);
  CODD_LAUNCH_CHECK();
  return CODD_OK;
}
