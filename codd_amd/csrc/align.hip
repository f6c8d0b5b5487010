// codd_align_depth: one frame's disparity, on the rectified left camera's grid, as a depth map on the grid of another
// calibrated camera (codd_amd/live.py, align_to=): the z-buffered forward warp a user of the session's depth writes on
// the host to colour it or to lay it over another camera's image.  The reference has no such output.  The contract,
// fixed to the fp32 operation, is in include/codd_hip.h.
//
// Two launches on the caller's stream:
//   fill    depth_out = +inf, 16-byte stores between a scalar head and tail (the pointer needs float alignment only);
//   splat   a lane per source pixel: back-project, move into the target camera, project through its lens with
//           calib_distort (calib_map.h: the arithmetic the ingest kernels run), write the position to uv_out and offer the
//           bits of Z_t to the k x k target pixels nearest to it with a 32-bit integer atomic min.  Z_t is positive and
//           finite, such floats order like their bit patterns, +inf (0x7f800000) lies above them all, and a minimum does
//           not depend on arrival order: equal inputs give equal bytes.
// Consecutive lanes read consecutive disparities and write consecutive (sx, sy) pairs; the atomics of a wave go to about
// k rows of about 64 m columns each (m the map's magnification), no return value is used, so a lane never waits for one.
#include "calib_map.h"

#include <math.h>

#define ALIGN_THREADS 256

struct AlignArgs {
  const float* disp;
  float* depth;
  float* uv;
  int W, h, w, ht, wt, k;
  float f, cx, cy, calib;
  float r[9], t[3];  // X_t = R X + T
  float r2_max;
  CalibView cv;  // the target camera: fx, fy, cx, cy, k, model (m is not used)
};

__global__ __launch_bounds__(ALIGN_THREADS) void align_fill_kernel(float* __restrict__ out, int n, int head, int nvec) {
  const int t = blockIdx.x * ALIGN_THREADS + threadIdx.x;
  const f32x4 inf4 = {INFINITY, INFINITY, INFINITY, INFINITY};
  if (t < nvec) *(f32x4*)(out + head + 4 * (size_t)t) = inf4;
  if (t < head) out[t] = INFINITY;
  const int tail0 = head + 4 * nvec;  // (n - tail0 <= 3)
  if (t < n - tail0) out[tail0 + t] = INFINITY;
}

// the k columns (rows) nearest to position s, clipped to [0, n): [lo, hi], empty when lo > hi
__device__ __forceinline__ void align_span(float s, int k, int n, int& lo, int& hi) {
  // (a position further than 4 from [0, n) reaches no pixel with k <= 4; inside, the conversions below are exact)
  if (!(s > -4.f && s < (float)n + 4.f)) { lo = 0; hi = -1; return; }
  const int first = (k & 1) ? (int)rintf(s) - (k - 1) / 2 : (int)floorf(s) - (k / 2 - 1);
  lo = max(first, 0);
  hi = min(first + k - 1, n - 1);
}

__global__ __launch_bounds__(ALIGN_THREADS) void align_splat_kernel(AlignArgs a) {
  const unsigned i = blockIdx.x * ALIGN_THREADS + threadIdx.x;  // (h w < 2^31: the last block's lanes stay below 2^32)
  if (i >= (unsigned)(a.h * a.w)) return;
  const int v = (int)(i / (unsigned)a.w), u = (int)i - v * a.w;
  const float d = a.disp[(size_t)v * a.W + u];
  float sx = __builtin_nanf(""), sy = sx, Zt = 0.f;
  bool ok = d > 0.f && d < INFINITY;  // (NaN compares false)
  if (ok) {
    const float Z = __fmul_rn(__fdiv_rn(1.f, d), a.calib);  // export_value's expression: the session's depth bits
    const float X = __fmul_rn(__fdiv_rn(__fsub_rn((float)u, a.cx), a.f), Z);
    const float Y = __fmul_rn(__fdiv_rn(__fsub_rn((float)v, a.cy), a.f), Z);
    const float Xt = __fmaf_rn(a.r[0], X, __fmaf_rn(a.r[1], Y, __fmaf_rn(a.r[2], Z, a.t[0])));
    const float Yt = __fmaf_rn(a.r[3], X, __fmaf_rn(a.r[4], Y, __fmaf_rn(a.r[5], Z, a.t[1])));
    Zt = __fmaf_rn(a.r[6], X, __fmaf_rn(a.r[7], Y, __fmaf_rn(a.r[8], Z, a.t[2])));
    ok = Zt > 0.f && Zt < INFINITY;
    if (ok) {
      const float x = __fdiv_rn(Xt, Zt), y = __fdiv_rn(Yt, Zt);
      const float r2 = __fmaf_rn(y, y, __fmul_rn(x, x));  // (calib_distort's own r2: the same two operations)
      ok = r2 <= a.r2_max;                                // (false for NaN)
      if (ok) {
        float px, py;
        calib_distort(a.cv, x, y, px, py);
        ok = fabsf(px) < INFINITY && fabsf(py) < INFINITY;
        if (ok) { sx = px; sy = py; }
      }
    }
  }
  if (a.uv) {
    float* o = a.uv + 2 * (size_t)i;
    if (((uintptr_t)a.uv & 7) == 0) {
      *(float2*)o = make_float2(sx, sy);
    } else {
      o[0] = sx; o[1] = sy;
    }
  }
  if (!ok) return;
  int x0, x1, y0, y1;
  align_span(sx, a.k, a.wt, x0, x1);
  align_span(sy, a.k, a.ht, y0, y1);
  const unsigned bits = __float_as_uint(Zt);
  unsigned* __restrict__ zb = (unsigned*)a.depth;
  for (int yy = y0; yy <= y1; ++yy)
    for (int xx = x0; xx <= x1; ++xx) atomicMin(zb + (size_t)yy * a.wt + xx, bits);
}

static bool all_finite(const double* p, int n) {
  for (int i = 0; i < n; ++i)
    if (!isfinite(p[i])) return false;
  return true;
}

extern "C" int codd_align_depth(const float* disp, int H, int W, int h, int w, float f, float cx, float cy, float calib,
                                const codd_align_view* view, int ht, int wt, int footprint, float* depth_out,
                                float* uv_out, void* stream) {
  if (!disp || !view || !depth_out) return CODD_EINVAL;
  if (H <= 0 || W <= 0 || h <= 0 || w <= 0 || h > H || w > W || ht <= 0 || wt <= 0) return CODD_EINVAL;
  if ((long long)h * w >= (1LL << 31) || (long long)ht * wt >= (1LL << 31)) return CODD_EINVAL;
  if (!(f > 0.f && f < INFINITY && calib > 0.f && calib < INFINITY && fabsf(cx) < INFINITY && fabsf(cy) < INFINITY))
    return CODD_EINVAL;  // (a NaN compares false)
  if (footprint < 1 || footprint > CODD_ALIGN_MAX_FOOTPRINT) return CODD_EINVAL;
  if (view->model != CODD_CALIB_BROWN && view->model != CODD_CALIB_FISHEYE) return CODD_EINVAL;
  if (!all_finite(view->R, 9) || !all_finite(view->T, 3) || !all_finite(view->K, 4) || !all_finite(view->dist, 8) ||
      !isfinite(view->r2_max))
    return CODD_EINVAL;
  if (!(view->K[0] > 0.0 && view->K[1] > 0.0 && view->r2_max > 0.0)) return CODD_EINVAL;
  AlignArgs a = {};
  a.disp = disp; a.depth = depth_out; a.uv = uv_out;
  a.W = W; a.h = h; a.w = w; a.ht = ht; a.wt = wt; a.k = footprint;
  a.f = f; a.cx = cx; a.cy = cy; a.calib = calib;
  for (int i = 0; i < 9; ++i) a.r[i] = (float)view->R[i];
  for (int i = 0; i < 3; ++i) a.t[i] = (float)view->T[i];
  a.r2_max = (float)view->r2_max;  // (may round to +inf: then no point is beyond it)
  a.cv.fx = (float)view->K[0]; a.cv.fy = (float)view->K[1]; a.cv.cx = (float)view->K[2]; a.cv.cy = (float)view->K[3];
  for (int i = 0; i < 8; ++i) a.cv.k[i] = (float)view->dist[i];
  a.cv.model = view->model;
  // (still so in fp32)
  if (!(a.cv.fx > 0.f && a.cv.fx < INFINITY && a.cv.fy > 0.f && a.cv.fy < INFINITY && a.r2_max > 0.f)) return CODD_EINVAL;
  const int n = ht * wt;
  const int head = min(n, (int)(((16 - ((uintptr_t)depth_out & 15)) & 15) / 4));
  const int nvec = (n - head) / 4;
  align_fill_kernel<<<cdiv(nvec > 0 ? nvec : 1, ALIGN_THREADS), ALIGN_THREADS, 0, (hipStream_t)stream>>>(depth_out, n, head, nvec);
  CODD_LAUNCH_CHECK();
  align_splat_kernel<<<cdiv((long long)h * w, ALIGN_THREADS), ALIGN_THREADS, 0, (hipStream_t)stream>>>(a);
  CODD_LAUNCH_CHECK();
  return CODD_OK;
}
