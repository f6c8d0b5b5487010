// The per-pixel decoders D_F of the source formats (include/codd_hip.h: codd_ingest_frames; CODD_FMT_RGB8 is the packed
// 3-byte pixel of codd_ingest_pair) and the one bilinear blend on decoded taps, for ingest_kernel (ingest.hip).
#pragma once
#include "common.h"

#include <limits.h>
#include <math.h>

struct FrameArgs {
  const unsigned char* img[2];
  float* out[2];
  long long pitch, bytes;  // bytes per source row; bytes of one view (codd_frame_bytes)
  int h, w;                // the SOURCE frame: what the decoders index
  int rh, rw;              // the rectified image: what the maps cover and the padding reflects (== h, w with map arrays)
  int H, W;                // the padded output
  int bgr;                 // the source channel order of CODD_FMT_RGB8
  int yoff, cy, cvr, cug, cvg, cub;  // the yuv row, coefficients in units of 2^-20
  float m0, m1, m2, s0, s1, s2;
};

#define FRAME_PX 4  // output pixels per thread: one 16-byte store per channel row

constexpr bool fmt_is_yuv422(int f) { return f == CODD_FMT_YUYV || f == CODD_FMT_UYVY; }
constexpr bool fmt_is_bayer(int f) { return f >= CODD_FMT_BAYER_RGGB && f <= CODD_FMT_BAYER_BGGR; }

__device__ __forceinline__ int sat8(int v) { return min(max(v, 0), 255); }

// Every factor fits 24 signed bits (|Y - yoff|, |U - 128|, |V - 128| <= 255; the coefficients are below 2^22) and every
// product 32, so the full-rate 24-bit multiply gives the int32 product of the contract; the 32-bit one runs at a quarter
// of that rate, which shows in a launch this short.
__device__ __forceinline__ void yuv_rgb(const FrameArgs& a, int Y, int U, int V, int* c) {
  const int b = __mul24(max(Y - a.yoff, 0), a.cy) + (1 << 19);
  U -= 128; V -= 128;
  c[0] = sat8((b + __mul24(a.cvr, V)) >> 20);
  c[1] = sat8((b - __mul24(a.cug, U) - __mul24(a.cvg, V)) >> 20);
  c[2] = sat8((b + __mul24(a.cub, U)) >> 20);
}

// RGB of a mosaic site from its 3x3 window n[row][col]; on_ry / on_rx: the site lies on a row / a column that holds R
__device__ __forceinline__ void bayer_rgb(const int n[3][3], bool on_ry, bool on_rx, int* c) {
  const int own = n[1][1];
  if (on_ry == on_rx) {  // an R or a B site
    const int diag = (n[0][0] + n[0][2] + n[2][0] + n[2][2] + 2) >> 2;
    c[1] = (n[0][1] + n[2][1] + n[1][0] + n[1][2] + 2) >> 2;
    c[0] = on_ry ? own : diag;
    c[2] = on_ry ? diag : own;
  } else {  // a G site: on R's row its row neighbours are R and its column neighbours B, on B's row the other way round
    const int hor = (n[1][0] + n[1][2] + 1) >> 1, ver = (n[0][1] + n[2][1] + 1) >> 1;
    c[1] = own;
    c[0] = on_ry ? hor : ver;
    c[2] = on_ry ? ver : hor;
  }
}

// index i in [-2, n + 1] of an axis of n >= 2 mosaic sites -> the reflect-101 source index (-1 -> 1, n -> n - 2); the
// clamp only serves indices two outside, which belong to taps that are themselves outside and are never used
__device__ __forceinline__ int reflect101(int i, int n) {
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * (n - 1) - i : i;
  return min(max(i, 0), n - 1);
}

// D_F at one pixel, byte loads only: the borders, the tail, the taps of a remap
template <int FMT>
__device__ __forceinline__ void frame_px(const FrameArgs& a, const unsigned char* __restrict__ img, int y, int x, int* c) {
  const long long p = a.pitch;
  if (FMT == CODD_FMT_RGB8) {  // packed 3-byte pixels in source channel order
    const unsigned char* q = img + y * p + (long long)x * 3;
    c[0] = q[0]; c[1] = q[1]; c[2] = q[2];
  } else if (FMT == CODD_FMT_MONO8) {
    c[0] = c[1] = c[2] = img[y * p + x];
  } else if (fmt_is_yuv422(FMT)) {
    constexpr int yo = FMT == CODD_FMT_YUYV ? 0 : 1;  // Y0 U Y1 V | U Y0 V Y1
    const unsigned char* q = img + y * p + (long long)(x >> 1) * 4;
    yuv_rgb(a, q[yo + 2 * (x & 1)], q[1 - yo], q[3 - yo], c);
  } else if (FMT == CODD_FMT_NV12) {
    const unsigned char* q = img + (a.h + (long long)(y >> 1)) * p + (x >> 1) * 2;
    yuv_rgb(a, img[y * p + x], q[0], q[1], c);
  } else {
    constexpr int RY = (FMT - CODD_FMT_BAYER_RGGB) >> 1, RX = (FMT - CODD_FMT_BAYER_RGGB) & 1;  // where R sits in the 2x2 cell
    const int ys[3] = {y == 0 ? 1 : y - 1, y, y == a.h - 1 ? a.h - 2 : y + 1};
    const int xs[3] = {x == 0 ? 1 : x - 1, x, x == a.w - 1 ? a.w - 2 : x + 1};
    int n[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) n[i][j] = img[ys[i] * p + xs[j]];
    bayer_rgb(n, (y & 1) == RY, (x & 1) == RX, c);
  }
}

// the 4 bytes at q (any alignment) as one little-endian dword, through aligned dword loads where they stay inside
// [lo, hi) -- the view's own bytes -- and through byte loads where they would not
__device__ __forceinline__ unsigned load4(const unsigned char* __restrict__ q, const unsigned char* lo, const unsigned char* hi) {
  const unsigned sh = (unsigned)((uintptr_t)q & 3);
  const unsigned char* a0 = q - sh;
  if (sh == 0) return *(const unsigned*)a0;
  if (a0 >= lo && a0 + 8 <= hi) {
    const unsigned d0 = ((const unsigned*)a0)[0], d1 = ((const unsigned*)a0)[1];
    return (unsigned)((((unsigned long long)d1 << 32) | d0) >> (sh * 8));
  }
  return (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16) | ((unsigned)q[3] << 24);
}

// D_F at the four pixels (y, x4 .. x4 + 3), x4 a multiple of 4 and x4 + 4 <= w: the source as whole dwords
template <int FMT>
__device__ __forceinline__ void frame_px4(const FrameArgs& a, const unsigned char* __restrict__ img, int y, int x4,
                                          int c[FRAME_PX][3]) {
  const long long p = a.pitch;
  const unsigned char* hi = img + a.bytes;
  if (FMT == CODD_FMT_RGB8) {  // 12 bytes = 3 dwords
    const unsigned char* q = img + y * p + (long long)x4 * 3;
    const unsigned d0 = load4(q, img, hi), d1 = load4(q + 4, img, hi), d2 = load4(q + 8, img, hi);
    c[0][0] = (int)(d0 & 255u); c[0][1] = (int)((d0 >> 8) & 255u); c[0][2] = (int)((d0 >> 16) & 255u);
    c[1][0] = (int)(d0 >> 24); c[1][1] = (int)(d1 & 255u); c[1][2] = (int)((d1 >> 8) & 255u);
    c[2][0] = (int)((d1 >> 16) & 255u); c[2][1] = (int)(d1 >> 24); c[2][2] = (int)(d2 & 255u);
    c[3][0] = (int)((d2 >> 8) & 255u); c[3][1] = (int)((d2 >> 16) & 255u); c[3][2] = (int)(d2 >> 24);
  } else if (FMT == CODD_FMT_MONO8) {
    const unsigned d = load4(img + y * p + x4, img, hi);
#pragma unroll
    for (int i = 0; i < FRAME_PX; ++i) c[i][0] = c[i][1] = c[i][2] = (int)((d >> (8 * i)) & 255u);
  } else if (fmt_is_yuv422(FMT)) {
    constexpr int yo = FMT == CODD_FMT_YUYV ? 0 : 1;
    const unsigned char* q = img + y * p + (long long)x4 * 2;
#pragma unroll
    for (int j = 0; j < 2; ++j) {  // one dword per pixel pair
      const unsigned d = load4(q + 4 * j, img, hi);
      const int U = (int)((d >> (8 * (1 - yo))) & 255u), V = (int)((d >> (8 * (3 - yo))) & 255u);
      yuv_rgb(a, (int)((d >> (8 * yo)) & 255u), U, V, c[2 * j]);
      yuv_rgb(a, (int)((d >> (8 * (yo + 2))) & 255u), U, V, c[2 * j + 1]);
    }
  } else if (FMT == CODD_FMT_NV12) {
    const unsigned dy = load4(img + y * p + x4, img, hi);
    const unsigned duv = load4(img + (a.h + (long long)(y >> 1)) * p + x4, img, hi);  // U0 V0 U1 V1 of pairs x4/2, x4/2 + 1
#pragma unroll
    for (int i = 0; i < FRAME_PX; ++i)
      yuv_rgb(a, (int)((dy >> (8 * i)) & 255u), (int)((duv >> (16 * (i >> 1))) & 255u),
              (int)((duv >> (16 * (i >> 1) + 8)) & 255u), c[i]);
  } else {
    constexpr int RY = (FMT - CODD_FMT_BAYER_RGGB) >> 1, RX = (FMT - CODD_FMT_BAYER_RGGB) & 1;
    const int ys[3] = {y == 0 ? 1 : y - 1, y, y == a.h - 1 ? a.h - 2 : y + 1};
    int win[3][FRAME_PX + 2];  // columns x4 - 1 .. x4 + 4 of the three rows
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const unsigned char* row = img + ys[i] * p;
      const unsigned d = load4(row + x4, img, hi);
#pragma unroll
      for (int j = 0; j < FRAME_PX; ++j) win[i][1 + j] = (int)((d >> (8 * j)) & 255u);
      // the two outer columns: a reflected one is a byte of the dword (-1 -> 1, w -> w - 2 = x4 + 2)
      win[i][0] = x4 == 0 ? win[i][2] : (int)row[x4 - 1];
      win[i][FRAME_PX + 1] = x4 + FRAME_PX == a.w ? win[i][FRAME_PX - 1] : (int)row[x4 + FRAME_PX];
    }
#pragma unroll
    for (int j = 0; j < FRAME_PX; ++j) {
      int n[3][3];
#pragma unroll
      for (int i = 0; i < 3; ++i) { n[i][0] = win[i][j]; n[i][1] = win[i][j + 1]; n[i][2] = win[i][j + 2]; }
      bayer_rgb(n, (y & 1) == RY, ((x4 + j) & 1) == RX, c[j]);
    }
  }
}

// THE BLEND of include/codd_hip.h in its stated fp32 operation order: every product that is not inside an fma rounds on
// its own, so nothing is left for -ffp-contract to decide
__device__ __forceinline__ float blend4(float v00, float v01, float v10, float v11, float ax, float ay) {
  const float w0 = __fsub_rn(1.f, ax), w1 = __fsub_rn(1.f, ay);
  const float top = __fmaf_rn(v00, w0, __fmul_rn(v01, ax)), bot = __fmaf_rn(v10, w0, __fmul_rn(v11, ax));
  return __fmaf_rn(top, w1, __fmul_rn(bot, ay));
}

// raw (un-normalised) channels of the source at position (sx, sy): the blend of the four taps, each D_F at the integer
// source pixel, or 0 outside
template <int FMT>
__device__ __forceinline__ void frame_blend(const FrameArgs& a, const unsigned char* __restrict__ img, float sx, float sy,
                                            float* c) {
  const int h = a.h, w = a.w;
  c[0] = c[1] = c[2] = 0.f;
  // every tap outside (this also catches NaN and +-inf: the comparisons are false) -> 0
  if (!(sx > -1.f && sx < (float)w && sy > -1.f && sy < (float)h)) return;
  const float fx0 = floorf(sx), fy0 = floorf(sy);
  const float ax = sx - fx0, ay = sy - fy0;
  const int x0 = (int)fx0, y0 = (int)fy0;
  const bool in[2][2] = {{y0 >= 0 && x0 >= 0, y0 >= 0 && x0 + 1 < w}, {y0 + 1 < h && x0 >= 0, y0 + 1 < h && x0 + 1 < w}};
  int t[2][2][3];
  if (fmt_is_bayer(FMT)) {
    // the four taps' 3x3 windows overlap in one 4x4 window of the reflect-extended mosaic: 16 loads, not 36
    constexpr int RY = (FMT - CODD_FMT_BAYER_RGGB) >> 1, RX = (FMT - CODD_FMT_BAYER_RGGB) & 1;
    int win[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned char* row = img + reflect101(y0 - 1 + i, h) * a.pitch;
#pragma unroll
      for (int j = 0; j < 4; ++j) win[i][j] = row[reflect101(x0 - 1 + j, w)];
    }
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        int n[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int j = 0; j < 3; ++j) n[i][j] = win[dy + i][dx + j];
        bayer_rgb(n, ((y0 + dy) & 1) == RY, ((x0 + dx) & 1) == RX, t[dy][dx]);
        if (!in[dy][dx]) t[dy][dx][0] = t[dy][dx][1] = t[dy][dx][2] = 0;
      }
  } else {
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        t[dy][dx][0] = t[dy][dx][1] = t[dy][dx][2] = 0;
        if (in[dy][dx]) frame_px<FMT>(a, img, y0 + dy, x0 + dx, t[dy][dx]);
      }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k)
    c[k] = blend4((float)t[0][0][k], (float)t[0][1][k], (float)t[1][0][k], (float)t[1][1][k], ax, ay);
}
