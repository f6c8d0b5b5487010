// codd_local_map: what is around me, and what was?  (codd_amd/live.py, localmap=)  A rolling occupancy map with integer
// log-odds in a fixed floor-aligned frame that follows the camera: codd_ego_motion's record says how the camera moved,
// codd_ground_plane's record and labels say where the floor is and which pixels stand on it, and this entry joins them over
// time.  The reference has no such output; what this replaces is downloading labels and disparity every frame, composing
// the poses on the host and rasterising every pixel there.  The contract is in include/codd_hip.h.
//
// Four launches on one stream, no allocation, no host synchronisation, integer atomics only:
//   1 pose     one wave (one lane works), fp64 in a fixed order: the planar step of the camera's foot point and heading from
//              G and the two floor frames, LOST and its policy, the new window origin; everything the later launches need is
//              left in the state;
//   2 cells    per window cell: a cell that was not in the old window (or every cell after a reset) gets logodds 0 and age
//              255 in the toroidal storage; the count tables O, F and the counters of the scratch are zeroed;
//   3 pixels   a wave takes an 8 x 8 block of pixels, four waves a 32 x 8 tile (scan_pixel_kernel's scheme): every lane
//              forms its pixel's (cell, floor | obstacle) key, the wave walks its DISTINCT keys -- neighbouring pixels fall
//              into a handful of cells -- counts each key's lanes by ballot and one lane adds the count;
//   4 update   per window cell the integer update rule, the unrolled outputs, and the counts of the record: a ballot per
//              wave, one integer add per wave and count, and the last block to finish writes the 16 doubles.
// Sums are integer: the aggregation of launch 3 changes no byte against one atomic per lane.  That variant is this file
// compiled with -DLOCALMAP_LANE_ATOMICS (tools/live_localmap_bench.py times it; profiles/live_localmap.md has the numbers).
// No workgroup-level LDS stage was built.
#include "common.h"

#pragma clang fp contract(off)  // every operation of the contract rounds once

#include "floor_frame.h"  // ScanFrame, scan_frame, scan_ground: the ground frame of codd_objects' "per pixel" paragraph
#include "map_window.h"   // the state's slots, the limits, map_mod, map_pixel_cell: shared with the layers on this window

struct MapArgs {
  const float* disp;
  const unsigned char* labels;
  const double* rec;
  const float* ego;  // may be NULL
  double* state;
  short* L;            // [gh][gw], toroidal
  unsigned char* age;  // [gh][gw], toroidal
  int* O;              // scratch: [gh][gw] in window order
  int* F;
  int* cnt;            // scratch: pixels, occupied, free, never seen, ticket
  short* map_out;
  unsigned char* age_out;
  double* record;
  unsigned select;
  int W, h, w, gh, gw, min_pixels, l_occ, l_free, l_min, l_max, decay, occ_level, free_level, lost, fresh;
  float fx, fy, cx, cy, calib, cell, range_min, range_max;
};

// ---- 1: the pose
__global__ __launch_bounds__(64) void map_pose_kernel(MapArgs a) {
  if (threadIdx.x != 0) return;
  double* st = a.state;
  const double* rec = a.rec;
  const double cell = (double)a.cell;
  const bool exists = st[ST_EXISTS] != 0.0;
  const bool cur = rec[3] != 0.0;
  const double pix0 = st[ST_IX0], piz0 = st[ST_IZ0];
  double px = st[ST_PX], pz = st[ST_PZ], hx = st[ST_HX], hz = st[ST_HZ];
  double n0 = 0, n1 = 0, n2 = 0, Hc = 0, f0 = 0, f1 = 0, f2 = 0, dx = 0, dz = 0;
  bool linked = false;
  if (exists && a.ego != nullptr && !a.fresh && a.ego[7] != 0.f) {
    const double t0 = (double)a.ego[0], t1 = (double)a.ego[1], t2 = (double)a.ego[2];
    double qx = (double)a.ego[3], qy = (double)a.ego[4], qz = (double)a.ego[5], qw = (double)a.ego[6];
    const double qq = ((qx * qx + qy * qy) + qz * qz) + qw * qw;
    const double qn = sqrt(qq);
    bool good = qn > 0.0 && qn < INFINITY;  // (false for NaN)
    if (good) {
      qx = qx / qn; qy = qy / qn; qz = qz / qn; qw = qw / qn;
      const double R00 = 1.0 - 2.0 * (qy * qy + qz * qz), R01 = 2.0 * (qx * qy - qz * qw), R02 = 2.0 * (qx * qz + qy * qw);
      const double R10 = 2.0 * (qx * qy + qz * qw), R11 = 1.0 - 2.0 * (qx * qx + qz * qz), R12 = 2.0 * (qy * qz - qx * qw);
      const double R20 = 2.0 * (qx * qz - qy * qw), R21 = 2.0 * (qy * qz + qx * qw), R22 = 1.0 - 2.0 * (qx * qx + qy * qy);
      const double np0 = st[ST_N], np1 = st[ST_N + 1], np2 = st[ST_N + 2], Hp = st[ST_HC];
      const double fp0 = st[ST_F], fp1 = st[ST_F + 1], fp2 = st[ST_F + 2];
      if (cur) {
        n0 = rec[8]; n1 = rec[9]; n2 = rec[10]; Hc = rec[11]; f0 = rec[22]; f1 = rec[23]; f2 = rec[24];
      } else {  // the stored floor frame, carried through G
        n0 = (R00 * np0 + R01 * np1) + R02 * np2;
        n1 = (R10 * np0 + R11 * np1) + R12 * np2;
        n2 = (R20 * np0 + R21 * np1) + R22 * np2;
        Hc = Hp - ((n0 * t0 + n1 * t1) + n2 * t2);
        const double g0 = -n2 * n0, g1 = -n2 * n1, g2 = 1.0 - n2 * n2;
        const double gn = sqrt((g0 * g0 + g1 * g1) + g2 * g2);
        good = gn >= 1e-3;  // (false for NaN)
        f0 = g0 / gn; f1 = g1 / gn; f2 = g2 / gn;
      }
      if (good) {
        const double r0 = fp1 * np2 - fp2 * np1, r1 = fp2 * np0 - fp0 * np2, r2 = fp0 * np1 - fp1 * np0;  // r_p = f_p x n_p
        const double c0 = -((R00 * t0 + R10 * t1) + R20 * t2), c1 = -((R01 * t0 + R11 * t1) + R21 * t2);
        const double c2 = -((R02 * t0 + R12 * t1) + R22 * t2);  // c = -R^T t: the current camera in the previous frame
        const double v0 = (R00 * f0 + R10 * f1) + R20 * f2, v1 = (R01 * f0 + R11 * f1) + R21 * f2;
        const double v2 = (R02 * f0 + R12 * f1) + R22 * f2;  // v = R^T f_c
        const double ddx = (r0 * c0 + r1 * c1) + r2 * c2, ddz = (fp0 * c0 + fp1 * c1) + fp2 * c2;
        const double ca = (r0 * v0 + r1 * v1) + r2 * v2, cb = (fp0 * v0 + fp1 * v1) + fp2 * v2;
        const double m = sqrt(ca * ca + cb * cb);
        if (m >= 1e-6) {  // (false for NaN)
          const double qx1 = (px + ddx * hz) + ddz * hx, qz1 = (pz - ddx * hx) + ddz * hz;
          const double ux = (ca * hz + cb * hx) / m, uz = (cb * hz - ca * hx) / m;
          const double un = sqrt(ux * ux + uz * uz);
          const double lim = 1073741824.0;
          if (fabs(qx1 / cell) < lim && fabs(qz1 / cell) < lim && un > 0.0 && un < INFINITY) {  // (false for NaN)
            px = qx1; pz = qz1; hx = ux / un; hz = uz / un; dx = ddx; dz = ddz;
            linked = true;
          }
        }
      }
    }
  }
  bool cleared = false, integrated = false, now = exists;
  double frames = st[ST_FRAMES], restarts = st[ST_RESTARTS];
  if (linked) {
    integrated = cur;
    frames += 1.0;
  } else if (exists && !a.fresh && a.lost == CODD_MAP_HOLD) {  // LOST, held: as if the camera stood still
    dx = 0.0; dz = 0.0;
    integrated = cur;
    frames += 1.0;
    if (cur) {
      n0 = rec[8]; n1 = rec[9]; n2 = rec[10]; Hc = rec[11]; f0 = rec[22]; f1 = rec[23]; f2 = rec[24];
    } else {
      n0 = st[ST_N]; n1 = st[ST_N + 1]; n2 = st[ST_N + 2]; Hc = st[ST_HC]; f0 = st[ST_F]; f1 = st[ST_F + 1]; f2 = st[ST_F + 2];
    }
  } else {  // LOST, reset (or nothing to lose yet)
    if (exists || a.fresh) restarts += 1.0;
    cleared = true;
    px = 0.0; pz = 0.0; hx = 0.0; hz = 1.0; dx = 0.0; dz = 0.0; frames = 0.0;
    now = cur;
    integrated = cur;
    if (cur) {
      n0 = rec[8]; n1 = rec[9]; n2 = rec[10]; Hc = rec[11]; f0 = rec[22]; f1 = rec[23]; f2 = rec[24];
    } else {
      n0 = n1 = n2 = Hc = f0 = f1 = f2 = 0.0;
    }
  }
  st[ST_EXISTS] = now ? 1.0 : 0.0;
  st[ST_PX] = px; st[ST_PZ] = pz; st[ST_HX] = hx; st[ST_HZ] = hz;
  st[ST_IX0] = floor(px / cell) - (double)(a.gw / 2);
  st[ST_IZ0] = floor(pz / cell) - (double)(a.gh / 2);
  st[ST_FRAMES] = frames; st[ST_RESTARTS] = restarts;
  st[ST_N] = n0; st[ST_N + 1] = n1; st[ST_N + 2] = n2; st[ST_HC] = Hc;
  st[ST_F] = f0; st[ST_F + 1] = f1; st[ST_F + 2] = f2;
  st[ST_PIX0] = pix0; st[ST_PIZ0] = piz0;
  st[ST_CLEARED] = cleared ? 1.0 : 0.0;
  st[ST_INTEGRATED] = integrated ? 1.0 : 0.0;
  st[ST_LINKED] = linked ? 1.0 : 0.0;
  st[ST_DX] = dx; st[ST_DZ] = dz;
  for (int k = 23; k < 32; ++k) st[k] = 0.0;
}

// ---- 2: cells that entered the window; the tables
__global__ __launch_bounds__(256) void map_enter_kernel(MapArgs a) {
  const double* st = a.state;
  const long long ix0 = (long long)st[ST_IX0], iz0 = (long long)st[ST_IZ0];
  const long long pix0 = (long long)st[ST_PIX0], piz0 = (long long)st[ST_PIZ0];
  const bool cleared = st[ST_CLEARED] != 0.0;
  const int cells = a.gh * a.gw;
  for (int k = blockIdx.x * 256 + threadIdx.x; k < cells; k += gridDim.x * 256) {
    const int j = k / a.gw, i = k - j * a.gw;
    const long long wx = ix0 + i, wz = iz0 + j;
    const bool kept = !cleared && wx >= pix0 && wx < pix0 + a.gw && wz >= piz0 && wz < piz0 + a.gh;
    if (!kept) {
      const int s = map_mod(wz, a.gh) * a.gw + map_mod(wx, a.gw);
      a.L[s] = 0;
      a.age[s] = 255;
    }
    a.O[k] = 0;
    a.F[k] = 0;
  }
  if (blockIdx.x == 0 && threadIdx.x < 8) a.cnt[threadIdx.x] = 0;
}

// ---- 3: every pixel into its cell
__global__ __launch_bounds__(256) void map_pixel_kernel(MapArgs a) {
  const double* st = a.state;
  if (st[ST_INTEGRATED] == 0.0) return;  // (no floor this frame: nothing is integrated)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tiles_x = (a.w + MAP_TW - 1) / MAP_TW;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int x = tx * MAP_TW + wave * MAP_BW + (lane & (MAP_BW - 1)), y = ty * MAP_BW + lane / MAP_BW;
  int key = -1;  // 2 * (jz * gw + jx) + (1 for an obstacle pixel)
  if (x < a.w && y < a.h) {
    const unsigned lab = a.labels[(size_t)y * a.w + x];
    const float d = a.disp[(size_t)y * a.W + x];
    const bool obst = lab < 32u && ((a.select >> lab) & 1u);
    if ((lab == CODD_GROUND_FLOOR || obst) && d > 0.f && d < INFINITY) {  // (NaN compares false)
      const ScanFrame g = scan_frame(a.rec);
      float gx, gz;
      scan_ground(a, g, y, x, d, &gx, &gz);
      int jz, jx;
      if (map_pixel_cell(a, st, gx, gz, &jz, &jx)) key = 2 * (jz * a.gw + jx) + (obst ? 1 : 0);
    }
  }
#ifdef LOCALMAP_LANE_ATOMICS
  if (key >= 0) atomicAdd(((key & 1) ? a.O : a.F) + (key >> 1), 1);  // (the timing variant: one atomic per lane)
#else
  unsigned long long rest = __ballot(key >= 0);
  while (rest) {  // (wave-uniform: one round per distinct key of the wave)
    const int first = __ffsll((long long)rest) - 1;
    const int k0 = __shfl(key, first, 64);
    const unsigned long long m = __ballot(key == k0);
    if (lane == first) atomicAdd(((k0 & 1) ? a.O : a.F) + (k0 >> 1), __popcll(m));
    rest &= ~m;
  }
#endif
}

// ---- 4: the update rule, the unrolled outputs, the record
__global__ __launch_bounds__(256) void map_update_kernel(MapArgs a) {
  const double* st = a.state;
  const long long ix0 = (long long)st[ST_IX0], iz0 = (long long)st[ST_IZ0];
  const int cells = a.gh * a.gw;
  const int lane = threadIdx.x & 63;
  int pixels = 0, n_occ = 0, n_free = 0, n_never = 0;
  for (int k = blockIdx.x * 256 + threadIdx.x; k < cells; k += gridDim.x * 256) {
    const int j = k / a.gw, i = k - j * a.gw;
    const int s = map_mod(iz0 + j, a.gh) * a.gw + map_mod(ix0 + i, a.gw);
    int L = a.L[s], g = a.age[s];
    const int o = a.O[k], f = a.F[k];
    if (o >= a.min_pixels) {
      L = min(L + a.l_occ, a.l_max);
      g = 0;
    } else if (f >= a.min_pixels) {
      L = max(L - a.l_free, a.l_min);
      g = 0;
    } else {
      if (g != 255) g = min(g + 1, 254);
      if (a.decay > 0) L = L > 0 ? max(L - a.decay, 0) : min(L + a.decay, 0);
    }
    a.L[s] = (short)L;
    a.age[s] = (unsigned char)g;
    a.map_out[k] = (short)L;
    a.age_out[k] = (unsigned char)g;
    pixels += o + f;
    n_occ += L >= a.occ_level;
    n_free += L <= a.free_level;
    n_never += g == 255;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    pixels += __shfl_xor(pixels, o, 64);
    n_occ += __shfl_xor(n_occ, o, 64);
    n_free += __shfl_xor(n_free, o, 64);
    n_never += __shfl_xor(n_never, o, 64);
  }
  if (lane == 0) {
    if (pixels) atomicAdd(a.cnt + 0, pixels);
    if (n_occ) atomicAdd(a.cnt + 1, n_occ);
    if (n_free) atomicAdd(a.cnt + 2, n_free);
    if (n_never) atomicAdd(a.cnt + 3, n_never);
  }
  // the record: fit_sums.h's ticket -- every thread's adds are performed device-wide before it passes the barrier, thread 0
  // draws the ticket behind it, and the workgroup that draws the last one reads the counters by device-scope atomics
  __threadfence();
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (atomicAdd(a.cnt + 4, 1) != (int)gridDim.x - 1) return;
  __threadfence();
  double* r = a.record;
  r[0] = st[ST_INTEGRATED]; r[1] = st[ST_LINKED]; r[2] = st[ST_RESTARTS]; r[3] = st[ST_FRAMES];
  r[4] = st[ST_PX]; r[5] = st[ST_PZ]; r[6] = st[ST_HX]; r[7] = st[ST_HZ];
  r[8] = st[ST_IX0]; r[9] = st[ST_IZ0];
  r[10] = (double)atomicAdd(a.cnt + 0, 0); r[11] = (double)atomicAdd(a.cnt + 1, 0);
  r[12] = (double)atomicAdd(a.cnt + 2, 0); r[13] = (double)atomicAdd(a.cnt + 3, 0);
  r[14] = st[ST_DX]; r[15] = st[ST_DZ];
}

// ---- the scratch: O, F, the counters; 16-byte aligned by the call itself
extern "C" long long codd_local_map_scratch(int gh, int gw) {
  if (!map_shape_ok(gh, gw)) return -1;
  return 16 + 8LL * gh * gw + 32;
}

extern "C" int codd_local_map(const float* disp, int H, int W, int h, int w, float fx, float fy, float cx, float cy,
                              float calib, const unsigned char* labels, const double* ground_record,
                              const float* ego_record, int fresh, int gh, int gw, float cell, float range_min,
                              float range_max, unsigned select, int min_pixels, int l_occ, int l_free, int l_min, int l_max,
                              int decay, int occ_level, int free_level, int lost, double* state, short* logodds,
                              unsigned char* age, void* scratch, long long scratch_bytes, short* map_out,
                              unsigned char* age_out, double* record, void* stream) {
  if (!disp || !labels || !ground_record || !state || !logodds || !age || !scratch || !map_out || !age_out || !record)
    return CODD_EINVAL;
  if (H <= 0 || W <= 0 || h <= 0 || w <= 0 || h > H || w > W || (long long)h * w >= (1LL << 31)) return CODD_EINVAL;
  if (!map_shape_ok(gh, gw)) return CODD_EINVAL;
  if (!(fx > 0.f && fx < INFINITY) || !(fy > 0.f && fy < INFINITY) || !(calib > 0.f && calib < INFINITY)) return CODD_EINVAL;
  if (!(fabsf(cx) < INFINITY) || !(fabsf(cy) < INFINITY)) return CODD_EINVAL;
  if (!(cell > 0.f && cell < INFINITY)) return CODD_EINVAL;
  if (!(range_max > 0.f && range_max < INFINITY) || !(range_min >= 0.f && range_min < range_max)) return CODD_EINVAL;
  if ((select & (1u << CODD_GROUND_FLOOR)) || min_pixels < 1) return CODD_EINVAL;
  if (l_occ < 0 || l_occ > 32767 || l_free < 0 || l_free > 32767 || decay < 0 || decay > 32767) return CODD_EINVAL;
  if (l_min < -32768 || l_min > 0 || l_max < 0 || l_max > 32767) return CODD_EINVAL;
  if (lost != CODD_MAP_RESET && lost != CODD_MAP_HOLD) return CODD_EINVAL;
  if (scratch_bytes < codd_local_map_scratch(gh, gw)) return CODD_EINVAL;
  const long long cells = (long long)gh * gw;
  char* base = (char*)(((uintptr_t)scratch + 15) & ~(uintptr_t)15);
  MapArgs a;
  a.disp = disp; a.labels = labels; a.rec = ground_record; a.ego = ego_record; a.state = state;
  a.L = logodds; a.age = age;
  a.O = (int*)base;
  a.F = (int*)(base + 4 * cells);
  a.cnt = (int*)(base + 8 * cells);
  a.map_out = map_out; a.age_out = age_out; a.record = record;
  a.select = select;
  a.W = W; a.h = h; a.w = w; a.gh = gh; a.gw = gw; a.min_pixels = min_pixels;
  a.l_occ = l_occ; a.l_free = l_free; a.l_min = l_min; a.l_max = l_max; a.decay = decay;
  a.occ_level = occ_level; a.free_level = free_level; a.lost = lost; a.fresh = fresh ? 1 : 0;
  a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.calib = calib;
  a.cell = cell; a.range_min = range_min; a.range_max = range_max;
  hipStream_t s = (hipStream_t)stream;
  const long long cw = (cells + 255) / 256;
  const unsigned cell_blocks = (unsigned)(cw < 1024 ? cw : 1024);
  const long long tiles = (long long)((w + MAP_TW - 1) / MAP_TW) * ((h + MAP_BW - 1) / MAP_BW);
  map_pose_kernel<<<1, 64, 0, s>>>(a);
  CODD_LAUNCH_CHECK();
  map_enter_kernel<<<cell_blocks, 256, 0, s>>>(a);
  CODD_LAUNCH_CHECK();
  map_pixel_kernel<<<(unsigned)tiles, 256, 0, s>>>(a);
  CODD_LAUNCH_CHECK();
  map_update_kernel<<<cell_blocks, 256, 0, s>>>(a);
  CODD_LAUNCH_CHECK();
  return CODD_OK;
}
