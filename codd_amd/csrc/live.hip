// Live-session export kernels: the launches that follow the captured frame graph when frames arrive one at a time from a
// camera (codd_amd/live.py); the ingest launch in front of it is ingest.hip.  The depth export is a pure streaming kernel:
// no LDS, several pixels per thread, 16-byte stores, a scalar tail; the motion export moves 28-byte and 8- / 12-byte
// records and stages them in LDS.  All run on the compute stream outside the graph.
#include "common.h"
#include "se3.h"

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
