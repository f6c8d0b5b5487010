// codd_height_map: how high is it, and do I fit?  (codd_amd/live.py, heightmap=)  A rolling 2.5-D elevation layer registered
// cell for cell to codd_local_map's window: per cell the highest and the lowest surface seen (top, bot) and the lowest
// thing hanging over it (ceil), as integers in units of h_res above the floor plane of the frame that saw them, kept across
// frames in toroidal storage like the map's log-odds.  It runs right behind codd_local_map and reads the pose and the
// window that call left in its state; it computes no pose of its own.  The reference has no such output; what this
// replaces is downloading labels, disparity and heights every frame and rasterising every pixel on the host.  The contract
// is in include/codd_hip.h.
//
// Four launches on one stream, no allocation, no host synchronisation, integer atomics only:
//   1 enter    per window cell: a cell that was not in the old window (every cell when CLEARED) gets the sentinels and age
//              255 in the toroidal storage; the tables Tmax, Tmin, Tn, Cmin, Cn and the counters of the scratch are set;
//   2 pixels   map_pixel_kernel's tiling (a wave an 8 x 8 block, four waves a 32 x 8 tile): every lane forms its pixel's
//              (cell, surface | overhead) key by map_window.h's expressions and its quantised height; the wave walks its
//              DISTINCT keys, reduces max, min and count of each key's lanes among themselves and one lane issues the
//              atomics;
//   3 update   per window cell the integer update rule on the toroidal storage and the unrolled layers;
//   4 derive   per window cell, on the unrolled layers launch 3 left: the step to the lowest known 8-neighbour, the flags,
//              and the counts and extrema of the record: a reduction per wave, one integer atomic per wave and figure, and
//              the workgroup that draws the last ticket writes the 16 doubles (localmap.hip's fence, barrier, ticket order).
// Maxima, minima and sums of integers do not depend on the order: the aggregation of launch 2 changes no byte against one
// atomic per lane and table.  That variant is this file compiled with -DHEIGHTMAP_LANE_ATOMICS (tools/
// live_heightmap_bench.py times it; profiles/live_heightmap.md has the numbers); nothing of it is in the library.
#include "common.h"

#include <climits>

#pragma clang fp contract(off)  // every operation of the contract rounds once

#include "floor_frame.h"  // ScanFrame, scan_frame, scan_ground
#include "map_window.h"   // the state's slots, the limits, map_mod, map_pixel_cell: the map's cells, bit for bit

#define HM_NONE (-32768)   // top, bot: no surface seen inside the current window
#define HM_NO_CEIL 32767   // ceil: nothing seen hanging over the cell
#define HM_Q_MAX 32000     // |q| of a quantised height, and the largest threshold

// the counters of the scratch
enum { HC_SURFACE = 0, HC_OVERHEAD = 1, HC_OBSERVED = 2, HC_KNOWN = 3, HC_STEP = 4, HC_HEADROOM = 5, HC_HOLE = 6, HC_TOP = 7,
       HC_BOT = 8, HC_TICKET = 9, HC_COUNT = 16 };

struct HeightArgs {
  const float* disp;
  const unsigned char* labels;
  const double* rec;
  const double* state;
  short* top;           // [gh][gw], toroidal
  short* bot;
  short* ceil;
  unsigned char* hage;
  int* Tmax;            // scratch: [gh][gw] in window order
  int* Tmin;
  int* Tn;
  int* Cmin;
  int* Cn;
  int* cnt;             // scratch: HC_COUNT counters
  short* top_out;
  short* bot_out;
  short* ceil_out;
  unsigned char* hage_out;
  unsigned short* step_out;
  unsigned char* flags_out;
  double* record;
  unsigned select;
  int W, h, w, gh, gw, min_pixels, alpha, max_step_q, robot_height_q, max_drop_q;
  float fx, fy, cx, cy, calib, cell, range_min, range_max, h_res;
};

// ---- 1: cells that entered the window; the tables
__global__ __launch_bounds__(256) void height_enter_kernel(HeightArgs a) {
  const double* st = a.state;
  const long long ix0 = (long long)st[ST_IX0], iz0 = (long long)st[ST_IZ0];
  const long long pix0 = (long long)st[ST_PIX0], piz0 = (long long)st[ST_PIZ0];
  const bool cleared = st[ST_CLEARED] != 0.0;
  const int cells = a.gh * a.gw;
  for (int k = blockIdx.x * 256 + threadIdx.x; k < cells; k += gridDim.x * 256) {
    const int j = k / a.gw, i = k - j * a.gw;
    const long long wx = ix0 + i, wz = iz0 + j;
    const bool kept = !cleared && wx >= pix0 && wx < pix0 + a.gw && wz >= piz0 && wz < piz0 + a.gh;
    if (!kept) {  // (map_enter_kernel's rule)
      const int s = map_mod(wz, a.gh) * a.gw + map_mod(wx, a.gw);
      a.top[s] = HM_NONE;
      a.bot[s] = HM_NONE;
      a.ceil[s] = HM_NO_CEIL;
      a.hage[s] = 255;
    }
    a.Tmax[k] = INT_MIN;
    a.Tmin[k] = INT_MAX;
    a.Tn[k] = 0;
    a.Cmin[k] = INT_MAX;
    a.Cn[k] = 0;
  }
  if (blockIdx.x == 0 && threadIdx.x < HC_COUNT)
    a.cnt[threadIdx.x] = threadIdx.x == HC_TOP ? INT_MIN : threadIdx.x == HC_BOT ? INT_MAX : 0;
}

// ---- 2: every pixel into its cell
__global__ __launch_bounds__(256) void height_pixel_kernel(HeightArgs a) {
  const double* st = a.state;
  if (st[ST_INTEGRATED] == 0.0) return;  // (no floor this frame: nothing is integrated)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tiles_x = (a.w + MAP_TW - 1) / MAP_TW;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int x = tx * MAP_TW + wave * MAP_BW + (lane & (MAP_BW - 1)), y = ty * MAP_BW + lane / MAP_BW;
  int key = -1, q = 0;  // key: 2 * (jz * gw + jx) + (1 for an overhead pixel)
  if (x < a.w && y < a.h) {
    const unsigned lab = a.labels[(size_t)y * a.w + x];
    const float d = a.disp[(size_t)y * a.W + x];
    const bool surf = lab < 32u && ((a.select >> lab) & 1u);
    const bool over = lab == CODD_GROUND_OVERHEAD;  // (select does not contain it: a pixel is one or the other)
    if ((surf || over) && d > 0.f && d < INFINITY) {  // (NaN compares false)
      const ScanFrame g = scan_frame(a.rec);
      float gx, gz;
      scan_ground(a, g, y, x, d, &gx, &gz);
      int jz, jx;
      if (map_pixel_cell(a, st, gx, gz, &jz, &jx)) {
        // the height of codd_ground_plane's "per pixel" paragraph
        const float c0 = (float)a.rec[0], c1 = (float)a.rec[1], c2 = (float)a.rec[2], Hc = (float)a.rec[11];
        const float p0 = (float)x - a.cx, p1 = (float)y - a.cy;
        const float e = d - ((c0 * p0 + c1 * p1) + c2);
        const float hgt = (Hc * e) / d;
        if (fabsf(hgt) < INFINITY) {  // (false for NaN)
          q = (int)fminf(fmaxf(rintf(hgt / a.h_res), -(float)HM_Q_MAX), (float)HM_Q_MAX);
          key = 2 * (jz * a.gw + jx) + (over ? 1 : 0);
        }
      }
    }
  }
#ifdef HEIGHTMAP_LANE_ATOMICS
  if (key >= 0) {  // (the timing variant: one atomic per lane and table)
    const int c = key >> 1;
    if (key & 1) {
      atomicMin(a.Cmin + c, q);
      atomicAdd(a.Cn + c, 1);
    } else {
      atomicMax(a.Tmax + c, q);
      atomicMin(a.Tmin + c, q);
      atomicAdd(a.Tn + c, 1);
    }
  }
#else
  unsigned long long rest = __ballot(key >= 0);
  while (rest) {  // (wave-uniform: one round per distinct key of the wave)
    const int first = __ffsll((long long)rest) - 1;
    const int k0 = __shfl(key, first, 64);
    const bool mine = key == k0;
    const unsigned long long m = __ballot(mine);
    int hi = mine ? q : INT_MIN, lo = mine ? q : INT_MAX;
    if (m & (m - 1)) {  // (wave-uniform: more than one lane has the key)
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        hi = max(hi, __shfl_xor(hi, o, 64));
        lo = min(lo, __shfl_xor(lo, o, 64));
      }
    }
    if (lane == first) {
      const int c = k0 >> 1, n = __popcll(m);
      if (k0 & 1) {
        atomicMin(a.Cmin + c, lo);
        atomicAdd(a.Cn + c, n);
      } else {
        atomicMax(a.Tmax + c, hi);
        atomicMin(a.Tmin + c, lo);
        atomicAdd(a.Tn + c, n);
      }
    }
    rest &= ~m;
  }
#endif
}

// v + (alpha (t - v)) / 256, the division truncating toward zero: |t - v| <= 64000 and alpha <= 256 stay far inside an int
__device__ __forceinline__ int height_blend(int v, int t, int alpha) { return v + (alpha * (t - v)) / 256; }

// ---- 3: the update rule and the unrolled layers
__global__ __launch_bounds__(256) void height_update_kernel(HeightArgs a) {
  const double* st = a.state;
  const long long ix0 = (long long)st[ST_IX0], iz0 = (long long)st[ST_IZ0];
  const int cells = a.gh * a.gw;
  for (int k = blockIdx.x * 256 + threadIdx.x; k < cells; k += gridDim.x * 256) {
    const int j = k / a.gw, i = k - j * a.gw;
    const int s = map_mod(iz0 + j, a.gh) * a.gw + map_mod(ix0 + i, a.gw);
    int top = a.top[s], bot = a.bot[s], ceil = a.ceil[s], g = a.hage[s];
    const bool surf = a.Tn[k] >= a.min_pixels, over = a.Cn[k] >= a.min_pixels;
    if (surf) {
      const int hi = a.Tmax[k], lo = a.Tmin[k];
      top = top == HM_NONE ? hi : height_blend(top, hi, a.alpha);
      bot = bot == HM_NONE ? lo : height_blend(bot, lo, a.alpha);
    }
    if (over) {
      const int lo = a.Cmin[k];
      ceil = ceil == HM_NO_CEIL ? lo : height_blend(ceil, lo, a.alpha);
    }
    if (surf || over) g = 0;
    else if (g != 255) g = min(g + 1, 254);
    a.top[s] = (short)top;
    a.bot[s] = (short)bot;
    a.ceil[s] = (short)ceil;
    a.hage[s] = (unsigned char)g;
    a.top_out[k] = (short)top;
    a.bot_out[k] = (short)bot;
    a.ceil_out[k] = (short)ceil;
    a.hage_out[k] = (unsigned char)g;
  }
}

// ---- 4: steps, flags, the record
__global__ __launch_bounds__(256) void height_derive_kernel(HeightArgs a) {
  const double* st = a.state;
  const int cells = a.gh * a.gw;
  const int lane = threadIdx.x & 63;
  int sum[7] = {0, 0, 0, 0, 0, 0, 0}, hi = INT_MIN, lo = INT_MAX;
  for (int k = blockIdx.x * 256 + threadIdx.x; k < cells; k += gridDim.x * 256) {
    const int j = k / a.gw, i = k - j * a.gw;
    const int top = a.top_out[k];
    int step = 0, flags = 255;
    if (top != HM_NONE) {  // a KNOWN cell
      int low = INT_MAX;  // the lowest known neighbour of the window: beyond its edge there is none, nothing wraps
      for (int dj = -1; dj <= 1; ++dj) {
        for (int di = -1; di <= 1; ++di) {
          const int jj = j + dj, ii = i + di;
          if ((dj | di) != 0 && jj >= 0 && jj < a.gh && ii >= 0 && ii < a.gw) {
            const int t = a.top_out[jj * a.gw + ii];
            if (t != HM_NONE) low = min(low, t);
          }
        }
      }
      if (low != INT_MAX) step = max(0, top - low);
      const int bot = a.bot_out[k], ceil = a.ceil_out[k];
      flags = (step > a.max_step_q ? 1 : 0) | (ceil != HM_NO_CEIL && ceil - top < a.robot_height_q ? 2 : 0) |
              (bot < -a.max_drop_q ? 4 : 0);
      sum[HC_KNOWN] += 1;
      sum[HC_STEP] += flags & 1;
      sum[HC_HEADROOM] += (flags >> 1) & 1;
      sum[HC_HOLE] += (flags >> 2) & 1;
      hi = max(hi, top);
      lo = min(lo, bot);
    }
    a.step_out[k] = (unsigned short)step;
    a.flags_out[k] = (unsigned char)flags;
    sum[HC_SURFACE] += a.Tn[k];
    sum[HC_OVERHEAD] += a.Cn[k];
    sum[HC_OBSERVED] += a.hage_out[k] == 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int c = 0; c < 7; ++c) sum[c] += __shfl_xor(sum[c], o, 64);
    hi = max(hi, __shfl_xor(hi, o, 64));
    lo = min(lo, __shfl_xor(lo, o, 64));
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 7; ++c)
      if (sum[c]) atomicAdd(a.cnt + c, sum[c]);
    if (hi != INT_MIN) atomicMax(a.cnt + HC_TOP, hi);
    if (lo != INT_MAX) atomicMin(a.cnt + HC_BOT, lo);
  }
  // the record: fit_sums.h's ticket -- every thread's atomics are performed device-wide before it passes the barrier,
  // thread 0 draws the ticket behind it, and the workgroup that draws the last one reads the counters by device-scope atomics
  __threadfence();
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (atomicAdd(a.cnt + HC_TICKET, 1) != (int)gridDim.x - 1) return;
  __threadfence();
  double* r = a.record;
  r[0] = st[ST_INTEGRATED];
  for (int c = 0; c < 7; ++c) r[1 + c] = (double)atomicAdd(a.cnt + c, 0);
  const bool any = r[1 + HC_KNOWN] != 0.0;
  r[8] = any ? (double)atomicAdd(a.cnt + HC_TOP, 0) : 0.0;
  r[9] = any ? (double)atomicAdd(a.cnt + HC_BOT, 0) : 0.0;
  r[10] = st[ST_IX0]; r[11] = st[ST_IZ0];
  r[12] = 0.0; r[13] = 0.0; r[14] = 0.0; r[15] = 0.0;
}

// ---- the scratch: Tmax, Tmin, Tn, Cmin, Cn, the counters; 16-byte aligned by the call itself
extern "C" long long codd_height_map_scratch(int gh, int gw) {
  if (!map_shape_ok(gh, gw)) return -1;
  return 16 + 20LL * gh * gw + 4 * HC_COUNT;
}

extern "C" int codd_height_map(const float* disp, int H, int W, int h, int w, float fx, float fy, float cx, float cy,
                               float calib, const unsigned char* labels, const double* ground_record, const double* state,
                               int gh, int gw, float cell, float range_min, float range_max, float h_res, unsigned select,
                               int min_pixels, int alpha, int max_step_q, int robot_height_q, int max_drop_q, short* top,
                               short* bot, short* ceil, unsigned char* hage, void* scratch, long long scratch_bytes,
                               short* top_out, short* bot_out, short* ceil_out, unsigned char* hage_out,
                               unsigned short* step_out, unsigned char* flags_out, double* record, void* stream) {
  if (!disp || !labels || !ground_record || !state || !top || !bot || !ceil || !hage || !scratch || !top_out || !bot_out ||
      !ceil_out || !hage_out || !step_out || !flags_out || !record)
    return CODD_EINVAL;
  if (H <= 0 || W <= 0 || h <= 0 || w <= 0 || h > H || w > W || (long long)h * w >= (1LL << 31)) return CODD_EINVAL;
  if (!map_shape_ok(gh, gw)) return CODD_EINVAL;
  if (!(fx > 0.f && fx < INFINITY) || !(fy > 0.f && fy < INFINITY) || !(calib > 0.f && calib < INFINITY)) return CODD_EINVAL;
  if (!(fabsf(cx) < INFINITY) || !(fabsf(cy) < INFINITY)) return CODD_EINVAL;
  if (!(cell > 0.f && cell < INFINITY)) return CODD_EINVAL;
  if (!(range_max > 0.f && range_max < INFINITY) || !(range_min >= 0.f && range_min < range_max)) return CODD_EINVAL;
  if (!(h_res > 0.f && h_res < INFINITY)) return CODD_EINVAL;
  if ((select & (1u << CODD_GROUND_OVERHEAD)) || min_pixels < 1 || alpha < 1 || alpha > 256) return CODD_EINVAL;
  if (max_step_q < 0 || max_step_q > HM_Q_MAX || robot_height_q < 0 || robot_height_q > HM_Q_MAX || max_drop_q < 0 ||
      max_drop_q > HM_Q_MAX)
    return CODD_EINVAL;
  if (scratch_bytes < codd_height_map_scratch(gh, gw)) return CODD_EINVAL;
  const void* const p16[] = {top, bot, ceil, top_out, bot_out, ceil_out, step_out};
  for (const void* p : p16)
    if ((uintptr_t)p & 1) return CODD_EINVAL;
  const void* const p64[] = {ground_record, state, record};
  for (const void* p : p64)
    if ((uintptr_t)p & 7) return CODD_EINVAL;
  const long long cells = (long long)gh * gw;
  char* base = (char*)(((uintptr_t)scratch + 15) & ~(uintptr_t)15);
  HeightArgs a;
  a.disp = disp; a.labels = labels; a.rec = ground_record; a.state = state;
  a.top = top; a.bot = bot; a.ceil = ceil; a.hage = hage;
  a.Tmax = (int*)base;
  a.Tmin = (int*)(base + 4 * cells);
  a.Tn = (int*)(base + 8 * cells);
  a.Cmin = (int*)(base + 12 * cells);
  a.Cn = (int*)(base + 16 * cells);
  a.cnt = (int*)(base + 20 * cells);
  a.top_out = top_out; a.bot_out = bot_out; a.ceil_out = ceil_out; a.hage_out = hage_out;
  a.step_out = step_out; a.flags_out = flags_out; a.record = record;
  a.select = select;
  a.W = W; a.h = h; a.w = w; a.gh = gh; a.gw = gw; a.min_pixels = min_pixels; a.alpha = alpha;
  a.max_step_q = max_step_q; a.robot_height_q = robot_height_q; a.max_drop_q = max_drop_q;
  a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.calib = calib;
  a.cell = cell; a.range_min = range_min; a.range_max = range_max; a.h_res = h_res;
  hipStream_t s = (hipStream_t)stream;
  const long long cw = (cells + 255) / 256;
  const unsigned cell_blocks = (unsigned)(cw < 1024 ? cw : 1024);
  const long long tiles = (long long)((w + MAP_TW - 1) / MAP_TW) * ((h + MAP_BW - 1) / MAP_BW);
  height_enter_kernel<<<cell_blocks, 256, 0, s>>>(a);
  CODD_LAUNCH_CHECK();
  height_pixel_kernel<<<(unsigned)tiles, 256, 0, s>>>(a);
  CODD_LAUNCH_CHECK();
  height_update_kernel<<<cell_blocks, 256, 0, s>>>(a);
  CODD_LAUNCH_CHECK();
  height_derive_kernel<<<cell_blocks, 256, 0, s>>>(a);
  CODD_LAUNCH_CHECK();
  return CODD_OK;
}
