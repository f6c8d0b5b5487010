// codd_range_scan: how far can I go?  (codd_amd/live.py, scan=)  A planar range scan in the ground grid's frame: every
// floor and obstacle pixel of codd_ground_plane's label map is projected onto the floor (the gx, gz of codd_objects, bit
// for bit), binned by bearing (a table of beam edges) and by range, and per beam the nearest range bin with enough obstacle
// pixels is the hit, with the nearest pixel of that bin, its object, and how far the floor was seen in front of it.  The
// reference has no such output; what this replaces is downloading the label map and the disparity every frame, projecting
// every pixel on the host, atan2 and np.minimum.at.  The contract is in include/codd_hip.h.
//
// Three launches on one stream, no allocation, no host synchronisation, integer atomics only:
//   1 clear    the tables O, F (int32) and N (uint64) of the scratch, [beam][bin], and scan_count;
//   2 pixel    a wave takes an 8 x 8 block of pixels, four waves a 32 x 8 tile: 8 columns lie in two or three beams where 64
//              pixels of a row lie in seventeen, and 8 rows of floor in a few range bins.  Every lane forms its pixel's
//              (beam, bin, floor | obstacle) key; the wave then walks its DISTINCT keys (at most 64 rounds, on a wall or
//              a floor two to six): the lanes of a key are counted by ballot and one lane adds the count; for an obstacle key
//              the smallest range of those lanes is found by a butterfly over the range's bits and the first lane that
//              holds it -- the lanes of a wave ascend in raster order -- issues the one 64-bit minimum;
//   3 resolve  a wave per beam walks the beam's bins: the hit bin, the free range, the floor count, the row of both tables,
//              and four integer adds into scan_count.
// Sums are integer and the minimum is order-free: the aggregation of launch 2 changes no byte against one atomic per lane
// (tools/live_scan_bench.py times that variant; profiles/live_scan.md has the numbers).
#include "common.h"

#pragma clang fp contract(off)  // every operation of the contract rounds once

#include "floor_frame.h"  // ScanFrame, scan_frame, scan_ground: the ground frame of codd_objects' "per pixel" paragraph

#define SCAN_BW 8   // a wave's block: SCAN_BW x SCAN_BW pixels
#define SCAN_TW 32  // a workgroup's tile: four blocks side by side
#define SCAN_MAX_BEAMS 2048
#define SCAN_MAX_BINS 1024
#define SCAN_MAX_CELLS (1 << 20)

struct ScanArgs {
  const float* disp;
  const unsigned char* labels;
  const double* rec;
  const unsigned short* ids;
  const float* edges;        // [beams + 1][2] = (sin, cos)
  unsigned long long* N;     // scratch: [beams][bins]
  int* O;                    //          [beams][bins]
  int* F;                    //          [beams][bins]
  int* count;
  int* scan_i;
  float* scan_f;
  unsigned select;
  int W, h, w, beams, bins, min_pixels;
  float fx, fy, cx, cy, calib, range_min, range_max, bin_w;
};

// ---- 1: clear
__global__ __launch_bounds__(256) void scan_clear_kernel(ScanArgs a) {
  const int cells = a.beams * a.bins;
  for (int k = blockIdx.x * 256 + threadIdx.x; k < cells; k += gridDim.x * 256) {
    a.N[k] = ~0ull;
    a.O[k] = 0;
    a.F[k] = 0;
  }
  if (blockIdx.x == 0 && threadIdx.x < 4) a.count[threadIdx.x] = 0;
}

// ---- 2: every pixel into its (beam, bin)
__global__ __launch_bounds__(256) void scan_pixel_kernel(ScanArgs a) {
  if (a.rec[3] == 0.0) return;  // (no floor: every beam stays unknown)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tiles_x = (a.w + SCAN_TW - 1) / SCAN_TW;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int x = tx * SCAN_TW + wave * SCAN_BW + (lane & (SCAN_BW - 1)), y = ty * SCAN_BW + lane / SCAN_BW;
  int key = -1;  // 2 * (beam * bins + k) + (1 for an obstacle pixel)
  unsigned rb = 0u;
  if (x < a.w && y < a.h) {
    const unsigned lab = a.labels[(size_t)y * a.w + x];
    const float d = a.disp[(size_t)y * a.W + x];
    const bool obst = lab < 32u && ((a.select >> lab) & 1u);
    if ((lab == CODD_GROUND_FLOOR || obst) && d > 0.f && d < INFINITY) {  // (NaN compares false)
      const ScanFrame g = scan_frame(a.rec);
      float gx, gz;
      scan_ground(a, g, y, x, d, &gx, &gz);
      if (gz > 0.f) {
        const float rho = sqrtf((gx * gx) + (gz * gz));
        if (rho >= a.range_min && rho < a.range_max) {
          int k = (int)floorf(rho / a.bin_w);
          k = k >= a.bins ? a.bins - 1 : k;
          // the number of edges with side >= 0: the signs do not increase along the table, so the first negative one is
          // found by bisection
          int lo = 0, hi = a.beams + 1;
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            const float side = (a.edges[2 * mid + 1] * gx) - (a.edges[2 * mid] * gz);
            if (side >= 0.f) lo = mid + 1; else hi = mid;
          }
          if (lo > 0 && lo < a.beams + 1) {
            key = 2 * ((lo - 1) * a.bins + k) + (obst ? 1 : 0);
            rb = __float_as_uint(rho);
          }
        }
      }
    }
  }
  unsigned long long rest = __ballot(key >= 0);
  while (rest) {  // (wave-uniform: one round per distinct key of the wave)
    const int first = __ffsll((long long)rest) - 1;
    const int k0 = __shfl(key, first, 64);
    const bool mine = key == k0;
    const unsigned long long m = __ballot(mine);
    const int cell = k0 >> 1;
    if (k0 & 1) {
      unsigned v = mine ? rb : 0xFFFFFFFFu;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, o, 64));
      const unsigned long long mm = __ballot(mine && rb == v);
      if (lane == __ffsll((long long)mm) - 1) {
        atomicAdd(a.O + cell, __popcll(m));
        atomicMin(a.N + cell, ((unsigned long long)rb << 32) | (unsigned)(y * a.w + x));
      }
    } else if (lane == first) {
      atomicAdd(a.F + cell, __popcll(m));
    }
    rest &= ~m;
  }
}

// ---- 3: a wave per beam
__global__ __launch_bounds__(256) void scan_resolve_kernel(ScanArgs a) {
  const int lane = threadIdx.x & 63, beam = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (beam >= a.beams) return;
  const int* O = a.O + (size_t)beam * a.bins;
  const int* F = a.F + (size_t)beam * a.bins;
  int kh = a.bins, all = 0;
  for (int k = lane; k < a.bins; k += 64) {
    const int o = O[k];
    all += o;
    if (o >= a.min_pixels && k < kh) kh = k;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    kh = min(kh, __shfl_xor(kh, o, 64));
    all += __shfl_xor(all, o, 64);
  }
  int kf = -1, floor_px = 0;
  for (int k = lane; k < kh; k += 64) {  // (kh is the limit: bins without a hit)
    const int f = F[k];
    floor_px += f;
    if (f >= a.min_pixels) kf = k;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    kf = max(kf, __shfl_xor(kf, o, 64));
    floor_px += __shfl_xor(floor_px, o, 64);
  }
  if (lane != 0) return;
  const float free_r = kf >= 0 ? (float)(kf + 1) * a.bin_w : 0.f;
  int* ri = a.scan_i + 4 * beam;
  float* rf = a.scan_f + 4 * beam;
  int state;
  if (kh < a.bins) {
    const unsigned long long n = a.N[(size_t)beam * a.bins + kh];
    const int idx = (int)(unsigned)n;
    const int y = idx / a.w, x = idx - y * a.w;
    float gx, gz;
    scan_ground(a, scan_frame(a.rec), y, x, a.disp[(size_t)y * a.W + x], &gx, &gz);
    int obj = -1;
    if (a.ids) {
      const unsigned short id = a.ids[idx];
      obj = id == 0xFFFFu ? -1 : (int)id;
    }
    rf[0] = __uint_as_float((unsigned)(n >> 32)); rf[1] = free_r; rf[2] = gx; rf[3] = gz;
    ri[0] = idx; ri[1] = obj; ri[2] = O[kh]; ri[3] = floor_px;
    state = 0;
  } else {
    const bool clear = free_r > 0.f;
    rf[0] = __uint_as_float(clear ? 0x7f800000u : 0x7fc00000u); rf[1] = clear ? free_r : 0.f; rf[2] = 0.f; rf[3] = 0.f;
    ri[0] = -1; ri[1] = -1; ri[2] = 0; ri[3] = floor_px;
    state = clear ? 1 : 2;
  }
  atomicAdd(a.count + state, 1);
  if (all) atomicAdd(a.count + 3, all);
}

// ---- the scratch: N, O, F; 16-byte aligned by the call itself
static inline bool scan_shape_ok(int beams, int bins) {
  return beams >= 1 && beams <= SCAN_MAX_BEAMS && bins >= 1 && bins <= SCAN_MAX_BINS && (long long)beams * bins <= SCAN_MAX_CELLS;
}

extern "C" long long codd_range_scan_scratch(int beams, int bins) {
  if (!scan_shape_ok(beams, bins)) return -1;
  return 16 + 16LL * beams * bins;
}

extern "C" int codd_range_scan(const float* disp, int H, int W, int h, int w, float fx, float fy, float cx, float cy,
                               float calib, const unsigned char* labels, const double* ground_record,
                               const unsigned short* ids, const float* edges, int beams, int bins, float range_min,
                               float range_max, unsigned select, int min_pixels, void* scratch, long long scratch_bytes,
                               int* scan_count, int* scan_i, float* scan_f, void* stream) {
  if (!disp || !labels || !ground_record || !edges || !scratch || !scan_count || !scan_i || !scan_f) return CODD_EINVAL;
  if (H <= 0 || W <= 0 || h <= 0 || w <= 0 || h > H || w > W || (long long)h * w >= (1LL << 31)) return CODD_EINVAL;
  if (!scan_shape_ok(beams, bins)) return CODD_EINVAL;
  if (!(fx > 0.f && fx < INFINITY) || !(fy > 0.f && fy < INFINITY) || !(calib > 0.f && calib < INFINITY)) return CODD_EINVAL;
  if (!(fabsf(cx) < INFINITY) || !(fabsf(cy) < INFINITY)) return CODD_EINVAL;
  if (!(range_max > 0.f && range_max < INFINITY) || !(range_min >= 0.f && range_min < range_max)) return CODD_EINVAL;
  if (select == 0u || (select & (1u << CODD_GROUND_FLOOR)) || min_pixels < 1) return CODD_EINVAL;
  if (scratch_bytes < codd_range_scan_scratch(beams, bins)) return CODD_EINVAL;
  const long long cells = (long long)beams * bins;
  char* base = (char*)(((uintptr_t)scratch + 15) & ~(uintptr_t)15);
  ScanArgs a;
  a.disp = disp; a.labels = labels; a.rec = ground_record; a.ids = ids; a.edges = edges;
  a.N = (unsigned long long*)base;
  a.O = (int*)(base + 8 * cells);
  a.F = (int*)(base + 12 * cells);
  a.count = scan_count; a.scan_i = scan_i; a.scan_f = scan_f;
  a.select = select;
  a.W = W; a.h = h; a.w = w; a.beams = beams; a.bins = bins; a.min_pixels = min_pixels;
  a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.calib = calib;
  a.range_min = range_min; a.range_max = range_max; a.bin_w = range_max / (float)bins;
  hipStream_t s = (hipStream_t)stream;
  const long long cw = (cells + 255) / 256;
  const long long tiles = (long long)((w + SCAN_TW - 1) / SCAN_TW) * ((h + SCAN_BW - 1) / SCAN_BW);
  scan_clear_kernel<<<(unsigned)(cw < 1024 ? cw : 1024), 256, 0, s>>>(a);
  CODD_LAUNCH_CHECK();
  scan_pixel_kernel<<<(unsigned)tiles, 256, 0, s>>>(a);
  CODD_LAUNCH_CHECK();
  scan_resolve_kernel<<<(unsigned)((beams + 3) / 4), 256, 0, s>>>(a);
  CODD_LAUNCH_CHECK();
  return CODD_OK;
}
