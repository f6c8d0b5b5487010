// THE MAP FUNCTION of include/codd_hip.h in its stated fp32 operation order, shared by the ingest kernels (ingest.hip:
// rectified pixel -> source position) and by codd_align_depth (align.hip: a 3-D point -> its position in a target camera).
// Every operation is pinned (__fmaf_rn and friends), so that every caller gives the same bits on the same numbers.
#pragma once
#include "common.h"

// one view's fp32 constants (computed in fp64 and rounded once by calib_constants): uniform per view -> scalar registers
struct CalibView {
  float m[9];  // M = R_rect^T K'^-1, row-major: (X, Y, W) = M (u, v, 1)
  float fx, fy, cx, cy;
  float k[8];
  int model;
};

// the lens half of the map function: normalised pinhole coordinates (x, y) -> the position (sx, sy) in the camera's image
__device__ __forceinline__ void calib_distort(const CalibView& c, float x, float y, float& sx, float& sy) {
  const float xx = __fmul_rn(x, x), yy = __fmul_rn(y, y), r2 = __fmaf_rn(y, y, xx);
  float xd, yd;
  if (c.model == CODD_CALIB_BROWN) {  // (wave-uniform)
    const float num = __fmaf_rn(__fmaf_rn(__fmaf_rn(c.k[4], r2, c.k[1]), r2, c.k[0]), r2, 1.f);
    const float den = __fmaf_rn(__fmaf_rn(__fmaf_rn(c.k[7], r2, c.k[6]), r2, c.k[5]), r2, 1.f);
    const float kr = __fdiv_rn(num, den), xy2 = __fmul_rn(__fadd_rn(x, x), y);
    xd = __fmaf_rn(x, kr, __fmaf_rn(c.k[2], xy2, __fmul_rn(c.k[3], __fmaf_rn(2.f, xx, r2))));
    yd = __fmaf_rn(y, kr, __fmaf_rn(c.k[3], xy2, __fmul_rn(c.k[2], __fmaf_rn(2.f, yy, r2))));
  } else {
    const float r = __fsqrt_rn(r2), t = atanf(r), t2 = __fmul_rn(t, t);
    const float td = __fmul_rn(t, __fmaf_rn(__fmaf_rn(__fmaf_rn(__fmaf_rn(c.k[3], t2, c.k[2]), t2, c.k[1]), t2, c.k[0]), t2, 1.f));
    const float s = r > 1e-8f ? __fdiv_rn(td, r) : 1.f;
    xd = __fmul_rn(x, s);
    yd = __fmul_rn(y, s);
  }
  sx = __fmaf_rn(c.fx, xd, c.cx);
  sy = __fmaf_rn(c.fy, yd, c.cy);
}

__device__ __forceinline__ void calib_map(const CalibView& c, int ui, int vi, float& sx, float& sy) {
  const float u = (float)ui, v = (float)vi;
  const float X = __fmaf_rn(c.m[0], u, __fmaf_rn(c.m[1], v, c.m[2]));
  const float Y = __fmaf_rn(c.m[3], u, __fmaf_rn(c.m[4], v, c.m[5]));
  const float W = __fmaf_rn(c.m[6], u, __fmaf_rn(c.m[7], v, c.m[8]));
  if (!(W > 0.f && W < INFINITY)) {
    sx = sy = __builtin_nanf("");
    return;
  }
  const float iw = __fdiv_rn(1.f, W);
  calib_distort(c, __fmul_rn(X, iw), __fmul_rn(Y, iw), sx, sy);
}
