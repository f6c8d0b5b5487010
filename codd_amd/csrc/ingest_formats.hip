// Live-session ingest of raw camera formats (codd_amd/live.py, pixel_format=): mono8, YUYV / UYVY, NV12 and the four
// Bayer mosaics, decoded to 8-bit RGB in integer registers inside the pass that normalises, rectifies and pads.  The
// contract is "decode, then codd_ingest_pair" (include/codd_hip.h: codd_ingest_frames): the decoded RGB image is never
// written to memory, and the output carries the bits codd_ingest_pair gives on it.  Same shape as ingest_pair_kernel
// (live.hip): a pure streaming kernel, no LDS, four output pixels per thread, 16-byte stores, a scalar tail.
#include "ingest_decode.h"

// raw (un-normalised) RGB of rectified pixel (y, x): the blend at the map entries of that pixel
template <int FMT>
__device__ __forceinline__ void frame_sample(const FrameArgs& a, const unsigned char* __restrict__ img,
                                             const float* __restrict__ mx, const float* __restrict__ my, int y, int x,
                                             float* c) {
  const size_t o = (size_t)y * a.w + x;
  frame_blend<FMT>(a, img, mx[o], my[o], c);
}

template <int FMT>
__global__ __launch_bounds__(256) void ingest_frames_kernel(FrameArgs a) {
  const int v = blockIdx.y;
  const unsigned char* __restrict__ img = a.img[v];
  const float* __restrict__ mx = a.mx[v];
  const float* __restrict__ my = a.my[v];
  float* __restrict__ out = a.out[v];
  const int h = a.h, w = a.w, H = a.H, W = a.W;
  const int W4 = (W + FRAME_PX - 1) / FRAME_PX;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)H * W4) return;
  const int y = (int)(t / W4), x4 = (int)(t - (long long)y * W4) * FRAME_PX;
  const int sy = y < h ? y : 2 * (h - 1) - y;  // reflect without edge repeat (cv2.BORDER_REFLECT_101)
  float c[FRAME_PX][3];
  if (!mx && x4 + FRAME_PX <= w) {  // map-free interior
    int ci[FRAME_PX][3];
    frame_px4<FMT>(a, img, sy, x4, ci);
#pragma unroll
    for (int i = 0; i < FRAME_PX; ++i) { c[i][0] = (float)ci[i][0]; c[i][1] = (float)ci[i][1]; c[i][2] = (float)ci[i][2]; }
  } else {
#pragma unroll
    for (int i = 0; i < FRAME_PX; ++i) {
      const int x = x4 + i;
      c[i][0] = c[i][1] = c[i][2] = 0.f;
      if (x < W) {
        const int sx = x < w ? x : 2 * (w - 1) - x;
        if (mx) {
          frame_sample<FMT>(a, img, mx, my, sy, sx, c[i]);
        } else {
          int ci[3];
          frame_px<FMT>(a, img, sy, sx, ci);
          c[i][0] = (float)ci[0]; c[i][1] = (float)ci[1]; c[i][2] = (float)ci[2];
        }
      }
    }
  }
  const size_t N = (size_t)H * W, o = (size_t)y * W + x4;
  const float m0 = a.m0, m1 = a.m1, m2 = a.m2, s0 = a.s0, s1 = a.s1, s2 = a.s2;
  f32x4 r0, r1, r2;
#pragma unroll
  for (int i = 0; i < FRAME_PX; ++i) {
    r0[i] = (c[i][0] - m0) / s0; r1[i] = (c[i][1] - m1) / s1; r2[i] = (c[i][2] - m2) / s2;  // ingest_pair_kernel's expression
  }
  if ((W & 3) == 0 && ((uintptr_t)out & 15) == 0) {  // (then x4 + 4 <= W and every row / plane offset is 16-byte aligned)
    *(f32x4*)(out + o) = r0; *(f32x4*)(out + N + o) = r1; *(f32x4*)(out + 2 * N + o) = r2;
  } else {
#pragma unroll
    for (int i = 0; i < FRAME_PX; ++i)
      if (x4 + i < W) { out[o + i] = r0[i]; out[N + o + i] = r1[i]; out[2 * N + o + i] = r2[i]; }
  }
}

extern "C" long long codd_frame_bytes(int fmt, int h, int w, long long pitch) {
  if (fmt < CODD_FMT_MONO8 || fmt > CODD_FMT_BAYER_BGGR || h <= 0 || w <= 0) return -1;
  if ((fmt_is_yuv422(fmt) || fmt == CODD_FMT_NV12) && (w & 1)) return -1;
  if (fmt == CODD_FMT_NV12 && (h & 1)) return -1;
  if (fmt_is_bayer(fmt) && (h < 2 || w < 2)) return -1;
  const long long row = fmt_is_yuv422(fmt) ? 2LL * w : w;
  if (pitch == 0) pitch = row;
  const long long rows = fmt == CODD_FMT_NV12 ? h + h / 2 : h;
  if (pitch < row || pitch > LLONG_MAX / rows) return -1;
  return pitch * rows;
}

extern "C" int codd_ingest_frames(const unsigned char* left, const unsigned char* right, int fmt, int yuv, int h, int w,
                                  long long pitch, const float* mean, const float* stdv, const float* lmap_x,
                                  const float* lmap_y, const float* rmap_x, const float* rmap_y, int H, int W,
                                  float* out_left, float* out_right, void* stream) {
  if (!left || !right || !mean || !stdv || !out_left || !out_right) return CODD_EINVAL;
  const long long bytes = codd_frame_bytes(fmt, h, w, pitch);
  if (bytes < 0) return CODD_EINVAL;
  const bool is_yuv = fmt_is_yuv422(fmt) || fmt == CODD_FMT_NV12;
  if (is_yuv && (yuv < 0 || yuv > 2)) return CODD_EINVAL;
  if (H < h || W < w || H - h >= h || W - w >= w) return CODD_EINVAL;
  if ((lmap_x == nullptr) != (lmap_y == nullptr) || (rmap_x == nullptr) != (rmap_y == nullptr)) return CODD_EINVAL;
  // yoff, then CY, CVR, CUG, CVG, CUB: bt601 and bt709 video range, BT.601 full range (jpeg)
  static const double coef[3][6] = {{16, 1.164, 1.596, 0.391, 0.813, 2.018},
                                    {16, 1.164, 1.793, 0.213, 0.533, 2.112},
                                    {0, 1.000, 1.402, 0.344, 0.714, 1.772}};
  const double* k = coef[is_yuv ? yuv : 0];
  FrameArgs a;
  a.img[0] = left; a.img[1] = right;
  a.mx[0] = lmap_x; a.my[0] = lmap_y; a.mx[1] = rmap_x; a.my[1] = rmap_y;
  a.out[0] = out_left; a.out[1] = out_right;
  a.pitch = bytes / (fmt == CODD_FMT_NV12 ? h + h / 2 : h); a.bytes = bytes;
  a.h = h; a.w = w; a.H = H; a.W = W;
  a.yoff = (int)k[0];
  a.cy = (int)lrint(k[1] * 1048576.0); a.cvr = (int)lrint(k[2] * 1048576.0); a.cug = (int)lrint(k[3] * 1048576.0);
  a.cvg = (int)lrint(k[4] * 1048576.0); a.cub = (int)lrint(k[5] * 1048576.0);
  a.m0 = mean[0]; a.m1 = mean[1]; a.m2 = mean[2]; a.s0 = stdv[0]; a.s1 = stdv[1]; a.s2 = stdv[2];
  const long long threads = (long long)H * cdiv(W, FRAME_PX);
  const dim3 grid(cdiv(threads, 256), 2);
  hipStream_t s = (hipStream_t)stream;
  switch (fmt) {
#define CODD_FRAMES_CASE(F) case F: ingest_frames_kernel<F><<<grid, 256, 0, s>>>(a); break
    CODD_FRAMES_CASE(CODD_FMT_MONO8);
    CODD_FRAMES_CASE(CODD_FMT_YUYV);
    CODD_FRAMES_CASE(CODD_FMT_UYVY);
    CODD_FRAMES_CASE(CODD_FMT_NV12);
    CODD_FRAMES_CASE(CODD_FMT_BAYER_RGGB);
    CODD_FRAMES_CASE(CODD_FMT_BAYER_GRBG);
    CODD_FRAMES_CASE(CODD_FMT_BAYER_GBRG);
    CODD_FRAMES_CASE(CODD_FMT_BAYER_BGGR);
#undef CODD_FRAMES_CASE
    default: return CODD_EINVAL;
  }
  CODD_LAUNCH_CHECK();
  return CODD_OK;
}
