// The rolling window of codd_local_map (include/codd_hip.h), shared by localmap.hip and the layers registered to it
// (heightmap.hip): the state's slots, the limits, the toroidal address of a world cell and the window cell of a pixel.
// A layer that lives cell for cell on the map's window takes these expressions and no others, so that its cells are the
// map's bit for bit.  The including file sets `#pragma clang fp contract(off)` before this header: every operation rounds
// once.
#pragma once
#include "common.h"
#include "floor_frame.h"  // ScanFrame, scan_frame, scan_ground

#define MAP_BW 8   // a wave's block: MAP_BW x MAP_BW pixels
#define MAP_TW 32  // a workgroup's tile: four blocks side by side
#define MAP_MAX_SIDE 4096
#define MAP_MAX_CELLS (1 << 22)

// the state's 32 doubles (include/codd_hip.h)
enum {
  ST_EXISTS = 0, ST_PX = 1, ST_PZ = 2, ST_HX = 3, ST_HZ = 4, ST_IX0 = 5, ST_IZ0 = 6, ST_FRAMES = 7, ST_RESTARTS = 8,
  ST_N = 9, ST_HC = 12, ST_F = 13, ST_PIX0 = 16, ST_PIZ0 = 17, ST_CLEARED = 18, ST_INTEGRATED = 19, ST_LINKED = 20,
  ST_DX = 21, ST_DZ = 22
};

__device__ __forceinline__ int map_mod(long long v, int n) {
  const int m = (int)(v % n);
  return m < 0 ? m + n : m;
}

static inline bool map_shape_ok(int gh, int gw) {
  return gh >= 1 && gh <= MAP_MAX_SIDE && gw >= 1 && gw <= MAP_MAX_SIDE && (long long)gh * gw <= MAP_MAX_CELLS;
}

// Launch 3 of codd_local_map from the floor coordinates on: the window cell (jz, jx) of a pixel whose (gx, gz) scan_ground
// gave, false for a pixel outside the range or the window.  a: any argument block with gh, gw and the fp32 members cell,
// range_min, range_max; st: the state as launch 1 left it.  (The caller projects the pixel itself, by scan_frame and
// scan_ground of floor_frame.h: with the projection in here the compiler commutes one addition of map_pixel_kernel, the
// same bits but not the parent's instruction stream.)
template <typename Args>
__device__ __forceinline__ bool map_pixel_cell(const Args& a, const double* st, float gx, float gz, int* jzo, int* jxo) {
  const float rho = sqrtf((gx * gx) + (gz * gz));
  if (rho >= a.range_min && rho < a.range_max) {
    const double cell = (double)a.cell;
    const float oxf = (float)(st[ST_PX] - st[ST_IX0] * cell), ozf = (float)(st[ST_PZ] - st[ST_IZ0] * cell);
    const float hxf = (float)st[ST_HX], hzf = (float)st[ST_HZ];
    const float wx = (gx * hzf + gz * hxf) + oxf, wz = (gz * hzf - gx * hxf) + ozf;
    const float jx = floorf(wx / a.cell), jz = floorf(wz / a.cell);
    if (jx >= 0.f && jx < (float)a.gw && jz >= 0.f && jz < (float)a.gh) {  // (NaN is outside)
      *jzo = (int)jz;
      *jxo = (int)jx;
      return true;
    }
  }
  return false;
}
