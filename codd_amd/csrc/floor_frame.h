// The ground frame of codd_objects' "per pixel" paragraph (include/codd_hip.h), shared by codd_range_scan (scan.hip) and
// codd_local_map (localmap.hip): both project a pixel onto the floor by these expressions and no others, so the scan and
// the map live in the frame of obj_f's extents bit for bit.  The including file sets `#pragma clang fp contract(off)`
// before this header: every operation rounds once.
#pragma once
#include "common.h"

struct ScanFrame {
  float r0, r1, r2, f0, f1, f2;
};

// rec: the 32 doubles of codd_ground_plane; r = f x n in fp64, each product and each difference rounded on its own
__device__ __forceinline__ ScanFrame scan_frame(const double* rec) {
  const double nx = rec[8], ny = rec[9], nz = rec[10], f0d = rec[22], f1d = rec[23], f2d = rec[24];
  ScanFrame g;
  g.r0 = (float)(f1d * nz - f2d * ny); g.r1 = (float)(f2d * nx - f0d * nz); g.r2 = (float)(f0d * ny - f1d * nx);
  g.f0 = (float)f0d; g.f1 = (float)f1d; g.f2 = (float)f2d;
  return g;
}

// a: any argument block with the fp32 members fx, fy, cx, cy, calib
template <typename Args>
__device__ __forceinline__ void scan_ground(const Args& a, const ScanFrame& g, int y, int x, float d, float* gx, float* gz) {
  const float p0 = (float)x - a.cx, p1 = (float)y - a.cy;
  const float Z = a.calib / d;
  const float X0 = Z * (p0 / a.fx), X1 = Z * (p1 / a.fy);
  *gx = (g.r0 * X0 + g.r1 * X1) + g.r2 * Z;
  *gz = (g.f0 * X0 + g.f1 * X1) + g.f2 * Z;
}
