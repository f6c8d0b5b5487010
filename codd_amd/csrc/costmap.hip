// codd_cost_map: where can I go?  (codd_amd/live.py, costmap=)  The last stage behind codd_local_map: per cell of the
// unrolled occupancy map the squared distance to the nearest occupied cell (truncated at R), an inflated cost in the
// convention of ROS costmap_2d, the cells the robot can reach from where it stands, and where the known space ends (the
// frontiers).  The reference has no such output; what this replaces is a download of the map every frame and a distance
// transform plus a flood fill on the host.  Integers only.  The contract is in include/codd_hip.h.
//
// Five launches on one stream (four for a grid of one tile), no allocation, no host synchronisation:
//   1 column   per cell its class and the row of the nearest occupied cell of its column within R rows (ties: the smaller
//              row); the counters of the scratch are zeroed;
//   2 tile     one 16 x 64 tile per workgroup: the column results of the tile's rows with a halo of R columns in LDS, per
//              cell the minimum over the 2R+1 columns of di^2 + g^2 (a global minimiser is its own column's nearest, and
//              the column pass kept the smallest row, so the key (d2, raster) keeps the tie rule), dist2, nearest, cost,
//              the traversable flag; then objects.hip's tile-local union-find of the traversable cells in LDS: a cell
//              starts out under the first cell of its horizontal run (one ballot per tile row), and two runs in
//              adjacent rows are united once per stretch in which they overlap;
//   3 border   the edges that cross a tile border, united in global memory, once per stretch of edges between the same
//              two tiles;
//   4 flatten  every traversable cell's parent becomes its root;
//   5 reach    reach, the frontiers, the counts, the nearest frontier by one 64-bit atomic minimum; the workgroup that
//              draws the last ticket writes the record (localmap.hip's fence, barrier, ticket order).
// Parents only ever decrease (atomicMin), so whatever a racing load returns is an ancestor and every chase ends; within
// launches 3 and 4 parents are read and written with relaxed agent-scope atomics (objects.hip's invariants).
// A single-workgroup path was built and measured, and is NOT in the library: one launch for grids of at most
// CM_ONE_MAX_CELLS cells, class, column result and 32-bit parents of the whole window in LDS (7 bytes per cell), the phases
// above separated by barriers instead of kernel boundaries.  At 128 x 128 it takes two to four times as long as the five
// launches (profiles/live_costmap.md): one CU with sixteen cells per thread waits for memory that 64 tiles on as many
// CUs fetch at once.  It is this file compiled with -DCOSTMAP_ONE_WORKGROUP (tools/live_costmap_bench.py builds and
// times it, and asserts equal bytes).
#include "common.h"

#define CM_TH 16           // tile rows
#define CM_TW 64           // tile columns: one wave reads one row of the tile
#define CM_MAX_R 128
#define CM_MAX_SIDE 4096   // codd_local_map's limits
#define CM_MAX_CELLS (1 << 22)
#define CM_ONE_THREADS 1024
#define CM_ONE_MAX_CELLS 16384  // the variant: the size threshold between the two paths
#define CM_ONE_LDS(n) (7 * (size_t)(n) + 80)  // parents int32, column rows int16, flags uint8; alignment and the counters
static_assert(CM_TW == 64 && CM_TH % 4 == 0, "cm_tile_kernel: 256 threads, a wave per tile row, four rows at a time");
static_assert(CM_ONE_LDS(CM_ONE_MAX_CELLS) <= 160 * 1024, "the single-workgroup path must fit gfx950's 160 KiB of LDS");
static_assert(CM_ONE_MAX_CELLS % 2 == 0, "the int16 plane behind the parents keeps the flags' offset even");
#define CM_RLX(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

enum { CM_FREE = 0, CM_OCC = 1, CM_UNKNOWN = 2, CM_CLASS = 3, CM_TRAV = 4 };  // a flags byte: class | CM_TRAV
// counters (int32 words): [0] OCC [1] inscribed or lethal [2] no information [3] reachable [4] frontiers [5] ticket
// [6] nearest at the start cell [7] unused [8:10] the nearest frontier's (d2 << 32) | raster, one 8-byte aligned word
enum { CN_OCC = 0, CN_INSCRIBED = 1, CN_NOINFO = 2, CN_REACH = 3, CN_FRONTIER = 4, CN_TICKET = 5, CN_NEAR0 = 6, CN_KEY = 8 };

struct CostArgs {
  const short* map;
  const unsigned char* age;
  const unsigned char* lut;
  short* G;            // scratch [gh][gw]: the row of the column's nearest OCC cell, -1 for none within R
  unsigned char* F;    // scratch [gh][gw]: flags
  int* P;              // scratch [gh][gw]: parents (raster indices), -1 for a cell that is not traversable
  int* cnt;            // scratch: the counters
  int* dist2;
  int* nearest;        // may be NULL
  unsigned char* cost;
  unsigned char* reach;
  double* record;
  int gh, gw, occ_level, free_level, R, start_i, start_j, seed_r2, through_unknown;
};

__device__ __forceinline__ int cm_class(const CostArgs& a, int k) {
  const int m = a.map[k];
  if (m >= a.occ_level) return CM_OCC;
  return (a.age[k] != 255 && m <= a.free_level) ? CM_FREE : CM_UNKNOWN;
}

// the cost of a cell and whether it is traversable, from its class and its squared distance (CODD_COST_FAR: none)
__device__ __forceinline__ int cm_cost(const CostArgs& a, int cls, int d2, int j, int i, bool* trav) {
  const int c = a.lut[d2 <= a.R * a.R ? d2 : a.R * a.R + 1];
  const long long di = i - a.start_i, dj = j - a.start_j;
  const bool seed = di * di + dj * dj <= (long long)a.seed_r2;
  *trav = seed ? cls != CM_OCC
               : c < CODD_COST_INSCRIBED && (cls == CM_FREE || (cls == CM_UNKNOWN && a.through_unknown != 0));
  return (cls == CM_UNKNOWN && c < CODD_COST_INSCRIBED) ? CODD_COST_NO_INFO : c;
}

// the row of the nearest OCC cell of column i within R rows of row j, the smaller row first; -1 for none.  occ(row)
template <class Occ>
__device__ __forceinline__ int cm_column(int j, int gh, int R, Occ occ) {
  for (int s = 0; s <= R; ++s) {
    if (j - s >= 0 && occ(j - s)) return j - s;
    if (j + s < gh && occ(j + s)) return j + s;
    if (j - s < 0 && j + s >= gh) break;
  }
  return -1;
}

// the smaller (d2 << 32) | raster over the columns i - R .. i + R of row j; g(column) is that column's row or -1
template <class Col>
__device__ __forceinline__ unsigned long long cm_row(int j, int i, int gw, int R, Col g) {
  unsigned long long best = ~0ull;
  const int lo = i - R < 0 ? 0 : i - R, hi = i + R >= gw ? gw - 1 : i + R;
  for (int c = lo; c <= hi; ++c) {
    const int r = g(c);
    if (r < 0) continue;
    const int dj = r - j, di = c - i;
    const unsigned long long key = ((unsigned long long)(unsigned)(di * di + dj * dj) << 32) | (unsigned)(r * gw + c);
    best = key < best ? key : best;
  }
  return best;
}

// unions in LDS (objects.hip's obj_lds_find / obj_lds_unite)
__device__ __forceinline__ int cm_lds_find(int* P, int i) {
  int p;  // (strictly decreasing: fewer steps than cells)
  while ((p = __hip_atomic_load(P + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != i) i = p;
  return i;
}

__device__ __forceinline__ void cm_lds_unite(int* P, int i, int j) {
  int a = cm_lds_find(P, i), b = cm_lds_find(P, j);
  while (a != b) {  // max(a, b) strictly decreases
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(P + a, b);
    if (old == a) break;
    a = old;
  }
}

// the record from the counters; d0: dist2 at the start cell
__device__ __forceinline__ void cm_record(double* r, int occ, int inscribed, int noinfo, int nreach, int nfront, bool ok,
                                          int d0, int near0, unsigned long long key) {
  r[0] = (double)occ; r[1] = (double)inscribed; r[2] = (double)noinfo; r[3] = (double)nreach; r[4] = (double)nfront;
  r[5] = ok ? 1.0 : 0.0;
  r[6] = d0 == CODD_COST_FAR ? -1.0 : (double)d0;
  r[7] = (double)near0;
  r[8] = key == ~0ull ? -1.0 : (double)(unsigned)(key & 0xffffffffull);
  r[9] = key == ~0ull ? -1.0 : (double)(unsigned)(key >> 32);
  for (int k = 10; k < 16; ++k) r[k] = 0.0;
}

// ---- 1: classes and columns
__global__ __launch_bounds__(256) void cm_column_kernel(CostArgs a) {
  if (blockIdx.x == 0 && threadIdx.x < 10) a.cnt[threadIdx.x] = threadIdx.x >= CN_KEY ? -1 : 0;
  const int cells = a.gh * a.gw, k = blockIdx.x * 256 + threadIdx.x;
  if (k >= cells) return;
  const int j = k / a.gw, i = k - j * a.gw;
  a.F[k] = (unsigned char)cm_class(a, k);
  a.G[k] = (short)cm_column(j, a.gh, a.R, [&](int r) { return a.map[r * a.gw + i] >= a.occ_level; });
}

// ---- 2: rows, cost, the tile's union-find
__global__ __launch_bounds__(256) void cm_tile_kernel(CostArgs a) {
  __shared__ short sG[CM_TH][CM_TW + 2 * CM_MAX_R];
  __shared__ int sP[CM_TH * CM_TW];
  __shared__ unsigned char sT[CM_TH * CM_TW];  // 1: traversable
  const int tid = threadIdx.x, lx = tid & 63, lr = tid >> 6, lane = lx;
  const int tiles_x = (a.gw + CM_TW - 1) / CM_TW;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int x0 = tx * CM_TW - a.R, span = CM_TW + 2 * a.R;  // the halo: R columns on either side
  for (int e = tid; e < CM_TH * span; e += 256) {
    const int ly = e / span, c = e - ly * span, y = ty * CM_TH + ly, x = x0 + c;
    sG[ly][c] = (y < a.gh && x >= 0 && x < a.gw) ? a.G[y * a.gw + x] : (short)-1;
  }
  __syncthreads();
  const int x = tx * CM_TW + lx;
  int n_occ = 0, n_ins = 0, n_no = 0;
#pragma unroll
  for (int k = 0; k < CM_TH / 4; ++k) {
    const int ly = lr + 4 * k, y = ty * CM_TH + ly, t = ly * CM_TW + lx;
    bool trav = false;
    if (x < a.gw && y < a.gh) {
      const int e = y * a.gw + x;
      const short* row = sG[ly];
      const unsigned long long key = cm_row(y, x, a.gw, a.R, [&](int c) { return (int)row[c - x0]; });
      const bool far = key == ~0ull || (int)(key >> 32) > a.R * a.R;
      const int d2 = far ? CODD_COST_FAR : (int)(key >> 32), near = far ? -1 : (int)(key & 0xffffffffull);
      const int cls = a.F[e] & CM_CLASS;
      const int c = cm_cost(a, cls, d2, y, x, &trav);
      a.dist2[e] = d2;
      if (a.nearest) a.nearest[e] = near;
      a.cost[e] = (unsigned char)c;
      a.F[e] = (unsigned char)(cls | (trav ? CM_TRAV : 0));
      if (x == a.start_i && y == a.start_j) a.cnt[CN_NEAR0] = near;
      n_occ += cls == CM_OCC;
      n_ins += c == CODD_COST_INSCRIBED || c == CODD_COST_LETHAL;
      n_no += c == CODD_COST_NO_INFO;
    }
    // a wave holds one tile row: a traversable cell starts out under the first cell of its horizontal run, so the row's
    // edges need no union at all
    const unsigned long long gaps = ~__ballot(trav) & ((1ull << lx) - 1ull);  // the cells left of lx that are not traversable
    sT[t] = trav ? 1 : 0;
    sP[t] = ly * CM_TW + (gaps ? 64 - __clzll((long long)gaps) : 0);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    n_occ += __shfl_xor(n_occ, o, 64); n_ins += __shfl_xor(n_ins, o, 64); n_no += __shfl_xor(n_no, o, 64);
  }
  if (lane == 0) {
    if (n_occ) atomicAdd(a.cnt + CN_OCC, n_occ);
    if (n_ins) atomicAdd(a.cnt + CN_INSCRIBED, n_ins);
    if (n_no) atomicAdd(a.cnt + CN_NOINFO, n_no);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < CM_TH / 4; ++k) {
    const int ly = lr + 4 * k, t = ly * CM_TW + lx;
    // a vertical edge, once per overlap of two runs: the edge to its left joins the same two runs
    if (ly > 0 && sT[t] && sT[t - CM_TW] && (lx == 0 || !sT[t - 1] || !sT[t - CM_TW - 1])) cm_lds_unite(sP, t, t - CM_TW);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < CM_TH / 4; ++k) {
    const int ly = lr + 4 * k, y = ty * CM_TH + ly, t = ly * CM_TW + lx;
    if (x < a.gw && y < a.gh) {
      int g = -1;
      if (sT[t]) {
        const int r = cm_lds_find(sP, t);  // the tile's raster order is the window's: the smallest index stays the smallest
        g = (ty * CM_TH + r / CM_TW) * a.gw + (tx * CM_TW + r % CM_TW);
      }
      a.P[y * a.gw + x] = g;
    }
  }
}

// ---- 3, 4: global memory (objects.hip's obj_find / obj_link / obj_flatten_kernel)
__device__ __forceinline__ int cm_find(int* P, int i) {
  int p;  // (strictly decreasing: fewer steps than cells)
  while ((p = CM_RLX(P + i)) != i) i = p;
  return i;
}

// unites the cells i and j of two tiles; (i - step, j - step) is the edge before this one along the border, and `first`
// says that it belongs to another pair of tiles (or lies outside): an edge whose predecessor joins the same two tiles
// and is an edge of traversable cells itself adds nothing, the tiles' own trees hold both its ends already
__device__ __forceinline__ void cm_link(const CostArgs& a, int i, int j, int step, bool first) {
  if (CM_RLX(a.P + i) < 0 || CM_RLX(a.P + j) < 0) return;  // (a cell that is not traversable stays -1)
  if (!first && CM_RLX(a.P + i - step) >= 0 && CM_RLX(a.P + j - step) >= 0) return;
  int p = cm_find(a.P, i), q = cm_find(a.P, j);
  while (p != q) {  // max(p, q) strictly decreases
    if (p < q) { const int t = p; p = q; q = t; }
    const int old = atomicMin(a.P + p, q);
    if (old == p) break;
    p = old;
  }
}

__global__ __launch_bounds__(256) void cm_border_kernel(CostArgs a) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int rows = (a.gh - 1) / CM_TH, cols = (a.gw - 1) / CM_TW;  // tile borders inside the window
  const int nh = rows * a.gw, n = nh + cols * a.gh;
  if (e >= n) return;
  if (e < nh) {
    const int y = (e / a.gw + 1) * CM_TH, x = e % a.gw;
    cm_link(a, y * a.gw + x, (y - 1) * a.gw + x, 1, x % CM_TW == 0);
  } else {
    const int v = e - nh;
    const int x = (v / a.gh + 1) * CM_TW, y = v % a.gh;
    cm_link(a, y * a.gw + x, y * a.gw + x - 1, a.gw, y % CM_TH == 0);
  }
}

__global__ __launch_bounds__(256) void cm_flatten_kernel(CostArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.gh * a.gw) return;
  if (CM_RLX(a.P + i) < 0) return;
  const int r = cm_find(a.P, i);
  __hip_atomic_store(a.P + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (an ancestor, whoever reads it)
}

// ---- 5: reach, frontiers, the record
// reach of cell (j, i) given whether a cell is reachable (reached(raster)) and its class (cls(raster))
template <class Reached, class Cls>
__device__ __forceinline__ int cm_reach(int j, int i, int gh, int gw, Reached reached, Cls cls) {
  const int k = j * gw + i;
  if (!reached(k)) return 0;
  bool front = false;
  if (i > 0) front |= cls(k - 1) == CM_UNKNOWN && !reached(k - 1);
  if (i + 1 < gw) front |= cls(k + 1) == CM_UNKNOWN && !reached(k + 1);
  if (j > 0) front |= cls(k - gw) == CM_UNKNOWN && !reached(k - gw);
  if (j + 1 < gh) front |= cls(k + gw) == CM_UNKNOWN && !reached(k + gw);
  return front ? 2 : 1;
}

__device__ __forceinline__ unsigned long long cm_front_key(const CostArgs& a, int j, int i) {
  const int di = i - a.start_i, dj = j - a.start_j;
  return ((unsigned long long)(unsigned)(di * di + dj * dj) << 32) | (unsigned)(j * a.gw + i);
}

__global__ __launch_bounds__(256) void cm_reach_kernel(CostArgs a) {
  const int cells = a.gh * a.gw, k = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  const int s = a.start_j * a.gw + a.start_i;
  const int rs = a.P[s];  // the start cell's root, or -1: nothing is reachable
  int v = 0;
  unsigned long long key = ~0ull;
  if (k < cells) {
    const int j = k / a.gw, i = k - j * a.gw;
    v = cm_reach(j, i, a.gh, a.gw, [&](int c) { return rs >= 0 && a.P[c] == rs; }, [&](int c) { return a.F[c] & CM_CLASS; });
    a.reach[k] = (unsigned char)v;
    if (v == 2) key = cm_front_key(a, j, i);
  }
  const int n_reach = __popcll(__ballot(v != 0)), n_front = __popcll(__ballot(v == 2));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(key, o, 64);
    key = other < key ? other : key;
  }
  if (lane == 0) {
    if (n_reach) atomicAdd(a.cnt + CN_REACH, n_reach);
    if (n_front) {
      atomicAdd(a.cnt + CN_FRONTIER, n_front);
      atomicMin((unsigned long long*)(a.cnt + CN_KEY), key);
    }
  }
  // the record: every thread's atomics are performed device-wide before it passes the barrier, thread 0 draws the ticket
  // behind it, and the workgroup that draws the last one reads the counters by device-scope atomics
  __threadfence();
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (atomicAdd(a.cnt + CN_TICKET, 1) != (int)gridDim.x - 1) return;
  __threadfence();
  cm_record(a.record, atomicAdd(a.cnt + CN_OCC, 0), atomicAdd(a.cnt + CN_INSCRIBED, 0), atomicAdd(a.cnt + CN_NOINFO, 0),
            atomicAdd(a.cnt + CN_REACH, 0), atomicAdd(a.cnt + CN_FRONTIER, 0), rs >= 0, a.dist2[s], a.cnt[CN_NEAR0],
            atomicAdd((unsigned long long*)(a.cnt + CN_KEY), 0ull));
}

#ifdef COSTMAP_ONE_WORKGROUP
// ---- the single-workgroup variant: the phases above with barriers in between, the whole window as one tile
__global__ __launch_bounds__(CM_ONE_THREADS) void cm_one_kernel(CostArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char cm_lds[];
  const int cells = a.gh * a.gw, tid = threadIdx.x, lane = tid & 63;
  const int even = (cells + 1) & ~1;
  int* sP = (int*)cm_lds;                                  // [cells]
  short* sG = (short*)(cm_lds + 4 * (size_t)even);         // [cells]
  unsigned char* sF = cm_lds + 6 * (size_t)even;           // [cells]
  int* sC = (int*)(cm_lds + ((7 * (size_t)even + 15) & ~(size_t)15));  // the counters and [10] dist2 at the start
  const int s = a.start_j * a.gw + a.start_i;
  if (tid < 10) sC[tid] = tid >= CN_KEY ? -1 : 0;
  for (int k = tid; k < cells; k += CM_ONE_THREADS) sF[k] = (unsigned char)cm_class(a, k);
  __syncthreads();
  for (int k = tid; k < cells; k += CM_ONE_THREADS) {
    const int j = k / a.gw, i = k - j * a.gw;
    sG[k] = (short)cm_column(j, a.gh, a.R, [&](int r) { return sF[r * a.gw + i] == CM_OCC; });
  }
  __syncthreads();
  for (int k0 = 0; k0 < cells; k0 += CM_ONE_THREADS) {  // (the trip count is the workgroup's: the ballots are whole)
    const int k = k0 + tid;
    int cls = -1, c = 0;
    if (k < cells) {
      const int j = k / a.gw, i = k - j * a.gw;
      const short* row = sG + j * a.gw;
      const unsigned long long key = cm_row(j, i, a.gw, a.R, [&](int col) { return (int)row[col]; });
      const bool far = key == ~0ull || (int)(key >> 32) > a.R * a.R;
      const int d2 = far ? CODD_COST_FAR : (int)(key >> 32), near = far ? -1 : (int)(key & 0xffffffffull);
      bool trav;
      cls = sF[k];
      c = cm_cost(a, cls, d2, j, i, &trav);
      a.dist2[k] = d2;
      if (a.nearest) a.nearest[k] = near;
      a.cost[k] = (unsigned char)c;
      sF[k] = (unsigned char)(cls | (trav ? CM_TRAV : 0));  // (only the own cell's flags are read in this phase)
      sP[k] = k;
      if (k == s) { sC[CN_NEAR0] = near; sC[10] = d2; }
    }
    const int n_occ = __popcll(__ballot(cls == CM_OCC));
    const int n_ins = __popcll(__ballot(cls >= 0 && (c == CODD_COST_INSCRIBED || c == CODD_COST_LETHAL)));
    const int n_no = __popcll(__ballot(cls >= 0 && c == CODD_COST_NO_INFO));
    if (lane == 0) {
      if (n_occ) atomicAdd(sC + CN_OCC, n_occ);
      if (n_ins) atomicAdd(sC + CN_INSCRIBED, n_ins);
      if (n_no) atomicAdd(sC + CN_NOINFO, n_no);
    }
  }
  __syncthreads();
  for (int k = tid; k < cells; k += CM_ONE_THREADS) {
    if (!(sF[k] & CM_TRAV)) continue;
    const int j = k / a.gw, i = k - j * a.gw;
    if (i > 0 && (sF[k - 1] & CM_TRAV)) cm_lds_unite(sP, k, k - 1);
    if (j > 0 && (sF[k - a.gw] & CM_TRAV) && (i == 0 || !(sF[k - 1] & CM_TRAV) || !(sF[k - a.gw - 1] & CM_TRAV)))
      cm_lds_unite(sP, k, k - a.gw);  // (once per overlap of two runs)
  }
  __syncthreads();
  for (int k = tid; k < cells; k += CM_ONE_THREADS) {
    if (!(sF[k] & CM_TRAV)) continue;
    const int r = cm_lds_find(sP, k);
    __hip_atomic_store(sP + k, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);  // (an ancestor, whoever reads it)
  }
  __syncthreads();
  const int rs = (sF[s] & CM_TRAV) ? sP[s] : -1;
  for (int k0 = 0; k0 < cells; k0 += CM_ONE_THREADS) {
    const int k = k0 + tid;
    int v = 0;
    unsigned long long key = ~0ull;
    if (k < cells) {
      const int j = k / a.gw, i = k - j * a.gw;
      v = cm_reach(j, i, a.gh, a.gw, [&](int c) { return rs >= 0 && (sF[c] & CM_TRAV) && sP[c] == rs; },
                   [&](int c) { return sF[c] & CM_CLASS; });
      a.reach[k] = (unsigned char)v;
      if (v == 2) key = cm_front_key(a, j, i);
    }
    const int n_reach = __popcll(__ballot(v != 0)), n_front = __popcll(__ballot(v == 2));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_xor(key, o, 64);
      key = other < key ? other : key;
    }
    if (lane == 0) {
      if (n_reach) atomicAdd(sC + CN_REACH, n_reach);
      if (n_front) {
        atomicAdd(sC + CN_FRONTIER, n_front);
        atomicMin((unsigned long long*)(sC + CN_KEY), key);
      }
    }
  }
  __syncthreads();
  if (tid == 0)
    cm_record(a.record, sC[CN_OCC], sC[CN_INSCRIBED], sC[CN_NOINFO], sC[CN_REACH], sC[CN_FRONTIER], rs >= 0, sC[10],
              sC[CN_NEAR0], *(unsigned long long*)(sC + CN_KEY));
}
#endif

// ---- the scratch: column rows, flags, parents, the counters; 16-byte aligned by the call itself
static inline bool cm_shape_ok(int gh, int gw) {
  return gh >= 1 && gh <= CM_MAX_SIDE && gw >= 1 && gw <= CM_MAX_SIDE && (long long)gh * gw <= CM_MAX_CELLS;
}
static inline long long cm_align(long long v) { return (v + 15) & ~15LL; }

extern "C" long long codd_cost_map_scratch(int gh, int gw, int R) {
  if (!cm_shape_ok(gh, gw) || R < 1 || R > CM_MAX_R) return -1;
  const long long n = (long long)gh * gw;
  return 16 + cm_align(4 * n) + cm_align(2 * n) + cm_align(n) + 64;
}

extern "C" int codd_cost_map(const short* map, const unsigned char* age, int gh, int gw, int occ_level, int free_level,
                             int R, const unsigned char* lut, int start_i, int start_j, int seed_r2, int through_unknown,
                             void* scratch, long long scratch_bytes, int* dist2, int* nearest, unsigned char* cost,
                             unsigned char* reach, double* record, void* stream) {
  if (!map || !age || !lut || !scratch || !dist2 || !cost || !reach || !record) return CODD_EINVAL;
  if (!cm_shape_ok(gh, gw) || R < 1 || R > CM_MAX_R || free_level >= occ_level) return CODD_EINVAL;
  if (start_i < 0 || start_i >= gw || start_j < 0 || start_j >= gh || seed_r2 < 0) return CODD_EINVAL;
  if (scratch_bytes < codd_cost_map_scratch(gh, gw, R)) return CODD_EINVAL;
  const long long n = (long long)gh * gw;
  char* base = (char*)(((uintptr_t)scratch + 15) & ~(uintptr_t)15);
  CostArgs a;
  a.map = map; a.age = age; a.lut = lut;
  a.P = (int*)base;
  a.G = (short*)(base + cm_align(4 * n));
  a.F = (unsigned char*)(base + cm_align(4 * n) + cm_align(2 * n));
  a.cnt = (int*)(base + cm_align(4 * n) + cm_align(2 * n) + cm_align(n));
  a.dist2 = dist2; a.nearest = nearest; a.cost = cost; a.reach = reach; a.record = record;
  a.gh = gh; a.gw = gw; a.occ_level = occ_level; a.free_level = free_level; a.R = R;
  a.start_i = start_i; a.start_j = start_j; a.seed_r2 = seed_r2; a.through_unknown = through_unknown;
  hipStream_t s = (hipStream_t)stream;
#ifdef COSTMAP_ONE_WORKGROUP
  if (n <= CM_ONE_MAX_CELLS) {
    const size_t lds = CM_ONE_LDS((n + 1) & ~1LL);
    if (lds > 64 * 1024) {
      hipError_t e = hipFuncSetAttribute((const void*)cm_one_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return (int)e;
    }
    cm_one_kernel<<<1, CM_ONE_THREADS, lds, s>>>(a);
    CODD_LAUNCH_CHECK();
    return CODD_OK;
  }
#endif
  const unsigned px = (unsigned)((n + 255) / 256);
  const unsigned tiles = (unsigned)(((gw + CM_TW - 1) / CM_TW) * ((gh + CM_TH - 1) / CM_TH));
  const long long nb = (long long)((gh - 1) / CM_TH) * gw + (long long)((gw - 1) / CM_TW) * gh;
  cm_column_kernel<<<px, 256, 0, s>>>(a);
  CODD_LAUNCH_CHECK();
  cm_tile_kernel<<<tiles, 256, 0, s>>>(a);
  CODD_LAUNCH_CHECK();
  if (nb > 0) {  // (a window of one tile has no border; the shape decides, not the data)
    cm_border_kernel<<<(unsigned)((nb + 255) / 256), 256, 0, s>>>(a);
    CODD_LAUNCH_CHECK();
  }
  cm_flatten_kernel<<<px, 256, 0, s>>>(a);
  CODD_LAUNCH_CHECK();
  cm_reach_kernel<<<px, 256, 0, s>>>(a);
  CODD_LAUNCH_CHECK();
  return CODD_OK;
}
