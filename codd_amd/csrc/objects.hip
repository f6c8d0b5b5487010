// codd_objects: what are the obstacles?  (codd_amd/live.py, objects=)  Connected components of the pixels that
// codd_ground_plane labelled (by default: obstacle), joined along 4-neighbour edges whose disparity step is small, and
// per component the pixel count, the image box, the nearest pixel and the extents in disparity, in height above the floor
// and in the ground grid's frame; the components that are large and tall enough become the objects, numbered in raster
// order of their first pixel.  The reference has no such output; what this replaces is downloading the label map and the
// disparity every frame and a connected-components pass on the host.  The contract is in include/codd_hip.h.
//
// Seven launches on one stream (six without the id map), no allocation, no host synchronisation, integer atomics only:
//   1 local    one 16 x 64 tile per workgroup: foreground test, union-find of the tile's edges in LDS, the tile's trees
//              flattened and written as global raster indices (background: -1);
//   2 border   the edges that cross a tile border, united in global memory;
//   3 flatten  every foreground pixel's parent becomes its root; a root clears its own statistics slot;
//   4 stats    every foreground pixel adds itself to its root's slot; a wave whose foreground lanes share one root (the
//              common case: 64 consecutive pixels of a row) reduces in registers and issues one set of atomics;
//   5 count    every workgroup counts the passing roots, the roots and the foreground pixels of its chunk of the raster
//              and writes one row; no ticket and no fence: the next launch reads the rows;
//   6 number   every workgroup adds launch 5's rows itself (as the fits of fit_sums.h add their partial rows): the chunks
//              before its own give its offset, all of them `count`; it numbers the passing roots of its chunk in raster
//              order behind that offset, writes the rows of the first max_objects of them and notes the number in the
//              root's slot; rows >= n are cleared;
//   7 ids      every pixel looks its root's number up.
// Parents only ever decrease (atomicMin), so whatever a racing load returns is an ancestor, and every chase ends at a
// root after fewer steps than there are pixels.  Within launches 2 and 3 parents are read and written with relaxed
// agent-scope atomics (a plain load may stay stale in a CU's vector cache for the whole kernel); everything else
// relies on the kernel boundaries.  Minima, maxima and counts are integer atomics: no order of arrival changes a byte.
#include "common.h"

#define OBJ_TH 16       // tile rows
#define OBJ_TW 64       // tile columns: one wave reads one row of the tile
#define OBJ_NB 1024     // at most this many chunks in launches 5 and 6
#define OBJ_SLOT 16     // int32 words per statistics slot
static_assert(OBJ_TW == 64 && OBJ_TH % 4 == 0, "obj_local_kernel: 256 threads, a wave per tile row, four rows at a time");
// slot: [0] pixels [1] x0 [2] y0 [3] x1 [4] y1 [5] the object number or -1 [6:8] nearest (one 64-bit word, 8-byte aligned)
//       [8] d_min [9] d_max [10] hgt_min [11] hgt_max [12] gx_min [13] gx_max [14] gz_min [15] gz_max (ordered images)
#define OBJ_RLX(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

struct ObjArgs {
  const float* disp;
  const unsigned char* labels;
  const double* rec;
  int* part;  // [OBJ_NB][4]: passing roots, roots, foreground pixels of a chunk (the fourth word is unused)
  int* P;     // [h w]
  int* S;     // [h w][OBJ_SLOT]
  int* count;
  int* obj_i;
  float* obj_f;
  unsigned short* ids;
  unsigned select;
  int W, h, w, min_pixels, max_objects, chunk, nchunk;
  float fx, fy, cx, cy, calib, gap_px, gap_rel, min_height;
};

// the order-preserving integer image of a float and back (-0 below +0; a NaN orders by its bits)
__device__ __forceinline__ unsigned obj_ord(float v) {
  const unsigned u = __float_as_uint(v);
  return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float obj_unord(unsigned o) { return __uint_as_float((o >> 31) ? (o & 0x7fffffffu) : ~o); }

__device__ __forceinline__ bool obj_foreground(const ObjArgs& a, int y, int x, float* d) {
  const unsigned lab = a.labels[(size_t)y * a.w + x];
  const float v = a.disp[(size_t)y * a.W + x];
  *d = v;
  return lab < 32u && ((a.select >> lab) & 1u) && v > 0.f && v < INFINITY;  // (NaN compares false)
}

__device__ __forceinline__ bool obj_joined(const ObjArgs& a, float da, float db) {
  return fabsf(da - db) <= fmaxf(a.gap_px, a.gap_rel * fminf(da, db));
}

// ---- 1: tile-local union-find in LDS
__device__ __forceinline__ int obj_lds_find(int* P, int i) {
  int p;  // (strictly decreasing: at most OBJ_TH * OBJ_TW steps)
  while ((p = __hip_atomic_load(P + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != i) i = p;
  return i;
}

__device__ __forceinline__ void obj_lds_unite(int* P, int i, int j) {
  int a = obj_lds_find(P, i), b = obj_lds_find(P, j);
  while (a != b) {  // max(a, b) strictly decreases
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(P + a, b);
    if (old == a) break;
    a = old;
  }
}

__global__ __launch_bounds__(256) void obj_local_kernel(ObjArgs a) {
#pragma clang fp contract(off)
  __shared__ int sP[OBJ_TH * OBJ_TW];
  __shared__ float sD[OBJ_TH * OBJ_TW];  // the disparity of a foreground pixel, -1 elsewhere
  const int tid = threadIdx.x, lx = tid & 63, lr = tid >> 6;
  const int tiles_x = (a.w + OBJ_TW - 1) / OBJ_TW;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int x = tx * OBJ_TW + lx;
  const bool floor_ok = a.rec[3] != 0.0;
#pragma unroll
  for (int k = 0; k < OBJ_TH / 4; ++k) {
    const int ly = lr + 4 * k, y = ty * OBJ_TH + ly, i = ly * OBJ_TW + lx;
    float d = -1.f;
    if (floor_ok && x < a.w && y < a.h) {
      float v;
      if (obj_foreground(a, y, x, &v)) d = v;
    }
    sD[i] = d;
    sP[i] = i;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < OBJ_TH / 4; ++k) {
    const int ly = lr + 4 * k, i = ly * OBJ_TW + lx;
    const float d = sD[i];
    if (d > 0.f) {
      if (lx > 0) {
        const float e = sD[i - 1];
        if (e > 0.f && obj_joined(a, d, e)) obj_lds_unite(sP, i, i - 1);
      }
      if (ly > 0) {
        const float e = sD[i - OBJ_TW];
        if (e > 0.f && obj_joined(a, d, e)) obj_lds_unite(sP, i, i - OBJ_TW);
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < OBJ_TH / 4; ++k) {
    const int ly = lr + 4 * k, y = ty * OBJ_TH + ly, i = ly * OBJ_TW + lx;
    if (x < a.w && y < a.h) {
      int g = -1;
      if (sD[i] > 0.f) {
        const int r = obj_lds_find(sP, i);  // the tile's raster order is the image's: the smallest index stays the smallest
        g = (ty * OBJ_TH + r / OBJ_TW) * a.w + (tx * OBJ_TW + r % OBJ_TW);
      }
      a.P[(size_t)y * a.w + x] = g;
    }
  }
}

// ---- 2, 3: global memory
__device__ __forceinline__ int obj_find(int* P, int i) {
  int p;  // (strictly decreasing: fewer steps than pixels)
  while ((p = OBJ_RLX(P + i)) != i) i = p;
  return i;
}

// unites (y, x) with its neighbour (yb, xb) when the edge joins them
__device__ __forceinline__ void obj_link(const ObjArgs& a, int y, int x, int yb, int xb) {
#pragma clang fp contract(off)
  const int i = y * a.w + x, j = yb * a.w + xb;
  if (OBJ_RLX(a.P + i) < 0 || OBJ_RLX(a.P + j) < 0) return;  // (background stays -1)
  if (!obj_joined(a, a.disp[(size_t)y * a.W + x], a.disp[(size_t)yb * a.W + xb])) return;
  int p = obj_find(a.P, i), q = obj_find(a.P, j);
  while (p != q) {  // max(p, q) strictly decreases
    if (p < q) { const int t = p; p = q; q = t; }
    const int old = atomicMin(a.P + p, q);
    if (old == p) break;
    p = old;
  }
}

__global__ __launch_bounds__(256) void obj_border_kernel(ObjArgs a) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long rows = (a.h - 1) / OBJ_TH, cols = (a.w - 1) / OBJ_TW;  // tile borders inside the crop
  const long long nh = rows * a.w, n = nh + cols * a.h;
  if (e >= n) return;
  if (e < nh) {
    const int y = (int)(e / a.w + 1) * OBJ_TH, x = (int)(e % a.w);
    obj_link(a, y, x, y - 1, x);
  } else {
    const long long v = e - nh;
    const int x = (int)(v / a.h + 1) * OBJ_TW, y = (int)(v % a.h);
    obj_link(a, y, x, y, x - 1);
  }
}

__global__ __launch_bounds__(256) void obj_flatten_kernel(ObjArgs a) {
  const long long n = (long long)a.h * a.w, e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const int i = (int)e;
  if (OBJ_RLX(a.P + i) < 0) return;
  const int r = obj_find(a.P, i);
  __hip_atomic_store(a.P + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (an ancestor, whoever reads it)
  if (r == i) {
    int* s = a.S + (size_t)i * OBJ_SLOT;
    s[0] = 0; s[1] = 0x7fffffff; s[2] = 0x7fffffff; s[3] = -1; s[4] = -1; s[5] = -1; s[6] = 0; s[7] = 0;
    s[8] = -1; s[9] = 0; s[10] = -1; s[11] = 0; s[12] = -1; s[13] = 0; s[14] = -1; s[15] = 0;
  }
}

// ---- 4: statistics at the roots
__global__ __launch_bounds__(256) void obj_stats_kernel(ObjArgs a) {
#pragma clang fp contract(off)  // every operation of the contract rounds once
  const long long n = (long long)a.h * a.w, e = (long long)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int root = e < n ? a.P[e] : -1;
  const bool fg = root >= 0;
  if (!__ballot(fg)) return;
  const double* rec = a.rec;
  const double nx = rec[8], ny = rec[9], nz = rec[10], f0d = rec[22], f1d = rec[23], f2d = rec[24];
  const float c0 = (float)rec[0], c1 = (float)rec[1], c2 = (float)rec[2], Hc = (float)rec[11];
  const float f0 = (float)f0d, f1 = (float)f1d, f2 = (float)f2d;
  const float r0 = (float)(f1d * nz - f2d * ny), r1 = (float)(f2d * nx - f0d * nz), r2 = (float)(f0d * ny - f1d * nx);
  int cnt = 0, x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = -1, y1 = -1;
  unsigned long long near = 0ull;
  unsigned lo[4] = {~0u, ~0u, ~0u, ~0u}, hi[4] = {0u, 0u, 0u, 0u};  // d, hgt, gx, gz
  if (fg) {
    const int y = (int)(e / a.w), x = (int)(e - (long long)y * a.w);
    const float d = a.disp[(size_t)y * a.W + x];
    const float p0 = (float)x - a.cx, p1 = (float)y - a.cy;
    const float r = d - ((c0 * p0 + c1 * p1) + c2);
    const float hgt = (Hc * r) / d;
    const float Z = a.calib / d;
    const float X0 = Z * (p0 / a.fx), X1 = Z * (p1 / a.fy);
    const float gx = (r0 * X0 + r1 * X1) + r2 * Z, gz = (f0 * X0 + f1 * X1) + f2 * Z;
    cnt = 1; x0 = x1 = x; y0 = y1 = y;
    near = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)~(unsigned)e;
    lo[0] = hi[0] = obj_ord(d); lo[1] = hi[1] = obj_ord(hgt); lo[2] = hi[2] = obj_ord(gx); lo[3] = hi[3] = obj_ord(gz);
  }
  const int first = __ffsll((long long)__ballot(fg)) - 1;
  const int root0 = __shfl(root, first, 64);
  const bool uniform = __all(!fg || root == root0);
  bool issue = fg;
  if (uniform) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      cnt += __shfl_xor(cnt, o, 64);
      x0 = min(x0, __shfl_xor(x0, o, 64)); y0 = min(y0, __shfl_xor(y0, o, 64));
      x1 = max(x1, __shfl_xor(x1, o, 64)); y1 = max(y1, __shfl_xor(y1, o, 64));
      const unsigned long long on = __shfl_xor(near, o, 64);
      near = on > near ? on : near;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        lo[k] = min(lo[k], (unsigned)__shfl_xor((int)lo[k], o, 64));
        hi[k] = max(hi[k], (unsigned)__shfl_xor((int)hi[k], o, 64));
      }
    }
    issue = lane == first;
  }
  if (!issue) return;
  int* s = a.S + (size_t)(uniform ? root0 : root) * OBJ_SLOT;
  atomicAdd(s + 0, cnt);
  atomicMin(s + 1, x0); atomicMin(s + 2, y0); atomicMax(s + 3, x1); atomicMax(s + 4, y1);
  atomicMax((unsigned long long*)(s + 6), near);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    atomicMin((unsigned*)s + 8 + 2 * k, lo[k]);
    atomicMax((unsigned*)s + 9 + 2 * k, hi[k]);
  }
}

// ---- 5, 6: selection and ordered numbering
__device__ __forceinline__ bool obj_passes(const ObjArgs& a, const int* s) {
  return s[0] >= a.min_pixels && obj_unord((unsigned)s[11]) >= a.min_height;  // (false for a NaN hgt_max)
}

__global__ __launch_bounds__(256) void obj_count_kernel(ObjArgs a) {
  __shared__ int sRed[3][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long n = (long long)a.h * a.w;
  const long long lo = (long long)blockIdx.x * a.chunk, hi = lo + a.chunk < n ? lo + a.chunk : n;
  int pass = 0, comps = 0, fgs = 0;
  for (long long e = lo + tid; e < hi; e += 256) {
    const int p = a.P[e];
    if (p < 0) continue;
    ++fgs;
    if (p == (int)e) {
      ++comps;
      if (obj_passes(a, a.S + (size_t)e * OBJ_SLOT)) ++pass;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    pass += __shfl_xor(pass, o, 64); comps += __shfl_xor(comps, o, 64); fgs += __shfl_xor(fgs, o, 64);
  }
  if (lane == 0) { sRed[0][wave] = pass; sRed[1][wave] = comps; sRed[2][wave] = fgs; }
  __syncthreads();
  if (tid < 3) a.part[4 * blockIdx.x + tid] = sRed[tid][0] + sRed[tid][1] + sRed[tid][2] + sRed[tid][3];
}

__global__ __launch_bounds__(256) void obj_number_kernel(ObjArgs a) {
  __shared__ int sW[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long n = (long long)a.h * a.w;
  const long long lo = (long long)blockIdx.x * a.chunk, hi = lo + a.chunk < n ? lo + a.chunk : n;
  // launch 5's rows, added by every workgroup itself (integers: any order gives the same sums; thread t takes chunks t,
  // t + 256, ..): the passing roots of the chunks before this one -- its offset -- and the three totals
  __shared__ int sSum[4][4];
  int sum[4] = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < OBJ_NB / 256; ++k) {
    const int b = tid + 256 * k;
    if (b < a.nchunk) {
      const int p = a.part[4 * b];
      sum[0] += b < (int)blockIdx.x ? p : 0;
      sum[1] += p; sum[2] += a.part[4 * b + 1]; sum[3] += a.part[4 * b + 2];
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum[c] += __shfl_xor(sum[c], o, 64);
    if (lane == 0) sSum[c][wave] = sum[c];
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 4; ++c) sum[c] = sSum[c][0] + sSum[c][1] + sSum[c][2] + sSum[c][3];
  const int nobj = sum[1] < a.max_objects ? sum[1] : a.max_objects;
  if (blockIdx.x == 0 && tid == 0) { a.count[0] = nobj; a.count[1] = sum[1]; a.count[2] = sum[2]; a.count[3] = sum[3]; }
  // rows >= n of both tables: zero
  const int spare = (a.max_objects - nobj) * 8;
  for (int k = blockIdx.x * 256 + tid; k < spare; k += a.nchunk * 256) {
    a.obj_i[nobj * 8 + k] = 0;
    a.obj_f[nobj * 8 + k] = 0.f;
  }
  int running = sum[0];
  for (long long e0 = lo; e0 < hi; e0 += 256) {  // (the trip count is the workgroup's)
    const long long e = e0 + tid;
    int* s = a.S + (size_t)e * OBJ_SLOT;
    const bool flag = e < hi && a.P[e] == (int)e && obj_passes(a, s);
    const unsigned long long b = __ballot(flag);
    if (lane == 0) sW[wave] = __popcll(b);
    __syncthreads();
    int rank = running + __popcll(b & ((1ull << lane) - 1ull));
    for (int k = 0; k < wave; ++k) rank += sW[k];
    running += sW[0] + sW[1] + sW[2] + sW[3];
    __syncthreads();
    if (flag && rank < a.max_objects) {
      s[5] = rank;
      const int idx = (int)~(unsigned)s[6];  // the low word of the nearest pixel's (bits(d) << 32) | ~index
      int* oi = a.obj_i + 8 * rank;
      float* of = a.obj_f + 8 * rank;
      oi[0] = s[0]; oi[1] = s[1]; oi[2] = s[2]; oi[3] = s[3]; oi[4] = s[4];
      oi[5] = idx % a.w; oi[6] = idx / a.w; oi[7] = (int)e;
      of[0] = obj_unord((unsigned)s[12]); of[1] = obj_unord((unsigned)s[13]);
      of[2] = obj_unord((unsigned)s[14]); of[3] = obj_unord((unsigned)s[15]);
      of[4] = obj_unord((unsigned)s[10]); of[5] = obj_unord((unsigned)s[11]);
      of[6] = obj_unord((unsigned)s[8]); of[7] = obj_unord((unsigned)s[9]);
    }
  }
}

// ---- 7: the id map
__global__ __launch_bounds__(256) void obj_ids_kernel(ObjArgs a) {
  const long long n = (long long)a.h * a.w, e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const int p = a.P[e];
  int id = -1;
  if (p >= 0) id = a.S[(size_t)p * OBJ_SLOT + 5];
  a.ids[e] = id >= 0 ? (unsigned short)id : (unsigned short)0xFFFF;
}

// ---- the scratch: chunk rows, parents, slots; 16-byte aligned by the call itself
static inline long long obj_parent_bytes(long long n) { return (4 * n + 15) & ~15LL; }

extern "C" long long codd_objects_scratch(int h, int w, int max_objects) {
  if (h <= 0 || w <= 0 || (long long)h * w >= (1LL << 31) || max_objects < 1 || max_objects > 4096) return -1;
  const long long n = (long long)h * w;
  return 16 + 16LL * OBJ_NB + obj_parent_bytes(n) + 4LL * OBJ_SLOT * n;
}

extern "C" int codd_objects(const float* disp, int H, int W, int h, int w, float fx, float fy, float cx, float cy,
                            float calib, const unsigned char* labels, const double* ground_record, unsigned select,
                            float gap_px, float gap_rel, int min_pixels, float min_height, int max_objects, void* scratch,
                            long long scratch_bytes, int* count, int* obj_i, float* obj_f, unsigned short* ids,
                            void* stream) {
  if (!disp || !labels || !ground_record || !scratch || !count || !obj_i || !obj_f) return CODD_EINVAL;
  if (H <= 0 || W <= 0 || h <= 0 || w <= 0 || h > H || w > W || (long long)h * w >= (1LL << 31)) return CODD_EINVAL;
  if (max_objects < 1 || max_objects > 4096 || select == 0u || min_pixels < 1) return CODD_EINVAL;
  if (!(fx > 0.f && fx < INFINITY) || !(fy > 0.f && fy < INFINITY) || !(calib > 0.f && calib < INFINITY)) return CODD_EINVAL;
  if (!(fabsf(cx) < INFINITY) || !(fabsf(cy) < INFINITY)) return CODD_EINVAL;
  if (!(gap_px > 0.f && gap_px < INFINITY) || !(gap_rel >= 0.f) || min_height != min_height) return CODD_EINVAL;
  if (scratch_bytes < codd_objects_scratch(h, w, max_objects)) return CODD_EINVAL;
  const long long n = (long long)h * w;
  char* base = (char*)(((uintptr_t)scratch + 15) & ~(uintptr_t)15);
  ObjArgs a;
  a.disp = disp; a.labels = labels; a.rec = ground_record;
  a.part = (int*)base;
  a.P = (int*)(base + 16LL * OBJ_NB);
  a.S = (int*)(base + 16LL * OBJ_NB + obj_parent_bytes(n));  // 16-byte aligned: a slot's 64-bit word is 8-byte aligned
  a.count = count; a.obj_i = obj_i; a.obj_f = obj_f; a.ids = ids;
  a.select = select;
  a.W = W; a.h = h; a.w = w; a.min_pixels = min_pixels; a.max_objects = max_objects;
  const long long per = (n + OBJ_NB - 1) / OBJ_NB;
  a.chunk = (int)((per + 255) / 256 * 256);
  a.nchunk = (int)((n + a.chunk - 1) / a.chunk);
  a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.calib = calib;
  a.gap_px = gap_px; a.gap_rel = gap_rel; a.min_height = min_height;
  hipStream_t s = (hipStream_t)stream;
  const unsigned tiles = (unsigned)(((w + OBJ_TW - 1) / OBJ_TW) * (long long)((h + OBJ_TH - 1) / OBJ_TH));
  const unsigned px = (unsigned)((n + 255) / 256);
  const long long nb = (long long)((h - 1) / OBJ_TH) * w + (long long)((w - 1) / OBJ_TW) * h;
  obj_local_kernel<<<tiles, 256, 0, s>>>(a);
  CODD_LAUNCH_CHECK();
  if (nb > 0) {  // (a crop of one tile has no border; the shape decides, not the data)
    obj_border_kernel<<<(unsigned)((nb + 255) / 256), 256, 0, s>>>(a);
    CODD_LAUNCH_CHECK();
  }
  obj_flatten_kernel<<<px, 256, 0, s>>>(a);
  CODD_LAUNCH_CHECK();
  obj_stats_kernel<<<px, 256, 0, s>>>(a);
  CODD_LAUNCH_CHECK();
  obj_count_kernel<<<a.nchunk, 256, 0, s>>>(a);
  CODD_LAUNCH_CHECK();
  obj_number_kernel<<<a.nchunk, 256, 0, s>>>(a);
  CODD_LAUNCH_CHECK();
  if (ids) {
    obj_ids_kernel<<<px, 256, 0, s>>>(a);
    CODD_LAUNCH_CHECK();
  }
  return CODD_OK;
}
