// codd_plan: which way do I go?  (codd_amd/live.py, plan=)  The stage behind codd_cost_map: the navigation function -- the
// least cost to reach a goal from every reachable cell of the window -- and the path from the robot's cell to the goal.  The
// goal is the nearest frontier, a cell, or a point of the map frame.  The reference has no such output; what this replaces is
// a download of cost and reach every frame and Dijkstra on the host.  Integers only.  The contract is in include/codd_hip.h.
//
// ONE workgroup of 1024 threads, one launch, no allocation, no host synchronisation.  The number of relaxation rounds depends
// on the map, the family's contract forbids a launch count that does, and a grid-wide barrier needs a co-resident grid; so
// the whole potential (uint32) and the weights (uint16, 0: not in D) of up to CODD_PLAN_MAX_CELLS cells live in the LDS of
// one CU, 6 bytes per cell, which gfx950's 160 KiB hold and 64 KiB would not.  Five phases between barriers:
//   1 goal    the goal cell (mode), the weights, P = 0 on the cells of D within goal_r2 of it; if there are none, the cell
//             of D nearest to it by one 64-bit LDS atomic minimum of (d2 << 32) | raster;
//   2 relax   rounds until no thread changed a value, at most gh gw + 1.  A thread takes 4 x 4 blocks of cells: it loads the
//             6 x 6 potentials and weights around a block into registers (36 LDS reads for 16 cells instead of 128), relaxes
//             the block in raster order and then in reverse raster order, each cell from the values as they stand
//             (Gauss-Seidel, the two passes of a chamfer transform), and writes back what changed.  Blocks read each other's
//             values while they change: every value ever stored is the cost of a real path and values only decrease, so any
//             order ends in the same fixed point, which is unique because every weight is at least 1.  A round in which
//             nothing was written read only final values, so it proves the fixed point.  -DPLAN_JACOBI keeps the register
//             block and relaxes every cell from the round's old values instead (tools/live_plan_bench.py times both);
//   3 output  potential, dir (the smallest k whose move is allowed and attains P), the counts;
//   4 path    wave 0 walks the LDS potential from the start cell: the eight moves in eight lanes, one ballot, the lowest
//             set bit is the smallest k;
//   5 record  and the -1 behind the path's last entry.
// No loop waits on memory another workgroup writes.  Inside the kernel a cell that P has not reached holds PL_INF = 2^30,
// above every real potential (7 x 1271 x 25600 < 2^28), so that P + len w never wraps.
#include <cmath>

#include "common.h"

#ifndef PLAN_THREADS
#define PLAN_THREADS 1024  // 128 VGPRs a thread: the two sweeps spill 57 of them, and are still faster than at 512 threads
#endif
#define PL_THREADS PLAN_THREADS
#define PL_INF 0x40000000u
#define PL_LDS(n) (((6 * (size_t)(n) + 15) & ~(size_t)15) + 64)
static_assert(PL_LDS(CODD_PLAN_MAX_CELLS) <= 160 * 1024, "the window must fit gfx950's 160 KiB of LDS");
static_assert(7ull * (255 + (1024 * 254) / 256) * CODD_PLAN_MAX_CELLS < PL_INF, "PL_INF lies above every potential");

// LDS words behind the 64-bit snap key: three "changed" flags, the cells of G, the cells with finite P, the largest finite
// P, the written path entries
enum { PI_FLAG = 0, PI_NG = 3, PI_FINITE = 4, PI_MAXP = 5, PI_WRITTEN = 6, PI_WORDS = 8 };

struct PlanArgs {
  const unsigned char* cost;
  const unsigned char* reach;
  const double* cost_record;
  const double* map_record;
  unsigned* potential;
  unsigned char* dir;  // may be NULL
  int* path;
  double* record;
  int* rounds;         // scratch: the rounds the relaxation took (for tools/live_plan_bench.py; no output reads it)
  double goal_x, goal_z;
  float cell;
  int gh, gw, start_i, start_j, mode, goal_i, goal_j, goal_r2, neutral, factor, unknown_cost, max_path;
};

__device__ __forceinline__ void pl_step(int k, int* di, int* dj) {
  if (k < 4) {
    *di = k == 0 ? 1 : k == 1 ? -1 : 0;
    *dj = k == 2 ? 1 : k == 3 ? -1 : 0;
  } else {
    *di = (k & 1) ? -1 : 1;
    *dj = (k & 2) ? -1 : 1;
  }
}

// whether move k from cell (j, i) of D is allowed, and its target's raster index
__device__ __forceinline__ bool pl_move(const unsigned short* sW, int gh, int gw, int j, int i, int k, int* q) {
  int di, dj;
  pl_step(k, &di, &dj);
  const int y = j + dj, x = i + di;
  if (y < 0 || y >= gh || x < 0 || x >= gw) return false;
  *q = y * gw + x;
  if (!sW[*q]) return false;
  return k < 4 || (sW[j * gw + x] && sW[y * gw + i]);  // no corner is cut
}

// one 4 x 4 block at (y0, x0): true iff a potential changed
__device__ __forceinline__ bool pl_block(unsigned* sP, const unsigned short* sW, int gh, int gw, int y0, int x0) {
  unsigned P[6][6], W[6][6];
  unsigned lowest = PL_INF, any = 0;
#pragma unroll
  for (int r = 0; r < 6; ++r) {
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      const int y = y0 - 1 + r, x = x0 - 1 + c;
      const bool in = y >= 0 && y < gh && x >= 0 && x < gw;
      P[r][c] = in ? sP[y * gw + x] : PL_INF;
      W[r][c] = in ? (unsigned)sW[y * gw + x] : 0u;
      lowest = P[r][c] < lowest ? P[r][c] : lowest;
      if (r >= 1 && r <= 4 && c >= 1 && c <= 4) any |= W[r][c];
    }
  }
  if (lowest >= PL_INF || !any) return false;  // nothing has arrived here yet, or no cell of D
  auto relaxed = [&](int r, int c) -> unsigned {
    unsigned v = P[r][c];
    auto take = [&](int rr, int cc, unsigned len, bool ok) {
      const unsigned cand = ok ? P[rr][cc] + len * W[rr][cc] : PL_INF;  // (a target outside D holds PL_INF)
      v = cand < v ? cand : v;
    };
    take(r, c + 1, 5u, true);
    take(r, c - 1, 5u, true);
    take(r + 1, c, 5u, true);
    take(r - 1, c, 5u, true);
    take(r + 1, c + 1, 7u, W[r][c + 1] && W[r + 1][c]);
    take(r + 1, c - 1, 7u, W[r][c - 1] && W[r + 1][c]);
    take(r - 1, c + 1, 7u, W[r][c + 1] && W[r - 1][c]);
    take(r - 1, c - 1, 7u, W[r][c - 1] && W[r - 1][c]);
    return W[r][c] ? v : P[r][c];
  };
  bool changed = false;
#ifdef PLAN_JACOBI
  unsigned N[4][4];
#pragma unroll
  for (int r = 1; r <= 4; ++r) {
#pragma unroll
    for (int c = 1; c <= 4; ++c) N[r - 1][c - 1] = relaxed(r, c);
  }
#pragma unroll
  for (int r = 1; r <= 4; ++r) {
#pragma unroll
    for (int c = 1; c <= 4; ++c) {
      if (N[r - 1][c - 1] != P[r][c]) {  // (only a cell of D inside the window changes)
        sP[(y0 - 1 + r) * gw + (x0 - 1 + c)] = N[r - 1][c - 1];
        changed = true;
      }
    }
  }
#else
  unsigned old[4][4];
#pragma unroll
  for (int r = 1; r <= 4; ++r) {
#pragma unroll
    for (int c = 1; c <= 4; ++c) {
      old[r - 1][c - 1] = P[r][c];
      P[r][c] = relaxed(r, c);
    }
  }
#pragma unroll
  for (int r = 4; r >= 1; --r) {
#pragma unroll
    for (int c = 4; c >= 1; --c) P[r][c] = relaxed(r, c);
  }
#pragma unroll
  for (int r = 1; r <= 4; ++r) {
#pragma unroll
    for (int c = 1; c <= 4; ++c) {
      if (P[r][c] != old[r - 1][c - 1]) {  // (only a cell of D inside the window changes)
        sP[(y0 - 1 + r) * gw + (x0 - 1 + c)] = P[r][c];
        changed = true;
      }
    }
  }
#endif
  return changed;
}

__global__ __launch_bounds__(PL_THREADS) void plan_kernel(PlanArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pl_lds[];
  const int cells = a.gh * a.gw, tid = threadIdx.x, lane = tid & 63, gw = a.gw, gh = a.gh;
  unsigned* sP = (unsigned*)pl_lds;                                  // [cells]
  unsigned short* sW = (unsigned short*)(pl_lds + 4 * (size_t)cells);  // [cells]: the weight, 0 outside D
  unsigned long long* sK = (unsigned long long*)(pl_lds + ((6 * (size_t)cells + 15) & ~(size_t)15));
  volatile int* sI = (volatile int*)(sK + 1);
  const int s = a.start_j * gw + a.start_i;

  // ---- 1: the goal cell, the weights, the goal set
  long long gi = 0, gj = 0;
  bool have = true;
  int clamped = 0;
  if (a.mode == CODD_PLAN_GOAL_CELL) {
    gi = a.goal_i; gj = a.goal_j;
  } else if (a.mode == CODD_PLAN_GOAL_WORLD) {
    gi = (long long)floor(a.goal_x / (double)a.cell) - (long long)a.map_record[8];
    gj = (long long)floor(a.goal_z / (double)a.cell) - (long long)a.map_record[9];
    const long long ci = gi < 0 ? 0 : gi >= gw ? gw - 1 : gi, cj = gj < 0 ? 0 : gj >= gh ? gh - 1 : gj;
    clamped = ci != gi || cj != gj;
    gi = ci; gj = cj;
  } else {
    const long long r = (long long)a.cost_record[8];
    have = r >= 0;
    if (have) { gj = r / gw; gi = r % gw; }
  }
  if (tid == 0) sK[0] = ~0ull;
  if (tid < PI_WORDS) sI[tid] = 0;
  __syncthreads();
  for (int k0 = 0; k0 < cells; k0 += PL_THREADS) {  // (the trip count is the workgroup's: the ballots are whole)
    const int k = k0 + tid;
    unsigned long long key = ~0ull;
    bool ing = false;
    if (k < cells) {
      const int j = k / gw, i = k - j * gw;
      const bool ind = a.reach[k] != 0;
      int c = a.cost[k];
      c = c == CODD_COST_NO_INFO ? a.unknown_cost : c;
      sW[k] = ind ? (unsigned short)(a.neutral + (a.factor * c) / 256) : (unsigned short)0;
      if (ind && have) {
        const long long di = i - gi, dj = j - gj;
        unsigned long long d2 = (unsigned long long)(di * di + dj * dj);
        ing = d2 <= (unsigned long long)a.goal_r2;
        d2 = d2 > 0xffffffffull ? 0xffffffffull : d2;
        key = (d2 << 32) | (unsigned)k;
      }
      sP[k] = ing ? 0u : PL_INF;
    }
    const int ng = __popcll(__ballot(ing));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_xor(key, o, 64);
      key = other < key ? other : key;
    }
    if (lane == 0) {
      if (ng) atomicAdd((int*)sI + PI_NG, ng);
      if (key != ~0ull) atomicMin(sK, key);
    }
  }
  __syncthreads();
  int n_goal = sI[PI_NG], snapped = 0;
  if (n_goal == 0 && have && sK[0] != ~0ull) {  // no cell of D within goal_r2: the nearest one
    snapped = 1;
    n_goal = 1;
    if (tid == 0) sP[(unsigned)(sK[0] & 0xffffffffull)] = 0u;
  }
  __syncthreads();

  // ---- 2: relax to the fixed point
  int rounds = 0;
  if (n_goal > 0) {
    const int bw = (gw + 3) >> 2, tasks = bw * ((gh + 3) >> 2);
    for (; rounds <= cells; ++rounds) {  // (Bellman-Ford needs fewer than `cells` rounds: the bound is never met)
      const int slot = rounds % 3;
      if (tid == 0) sI[PI_FLAG + (rounds + 1) % 3] = 0;  // the next round's flag: last read before the previous barrier
      bool changed = false;
      for (int t = tid; t < tasks; t += PL_THREADS) {
        const int by = t / bw;
        changed |= pl_block(sP, sW, gh, gw, by << 2, (t - by * bw) << 2);
      }
      if (changed) sI[PI_FLAG + slot] = 1;
      __syncthreads();
      if (!sI[PI_FLAG + slot]) break;
    }
  }
  if (tid == 0) a.rounds[0] = rounds;

  // ---- 3: potential, dir, the counts
  for (int k0 = 0; k0 < cells; k0 += PL_THREADS) {
    const int k = k0 + tid;
    bool fin = false;
    unsigned pmax = 0;
    if (k < cells) {
      const unsigned p = sP[k];
      fin = sW[k] != 0 && p < PL_INF;
      int d = 255;
      if (fin) {
        pmax = p;
        d = 8;
        if (p != 0) {
          const int j = k / gw, i = k - j * gw;
          d = 255;
          for (int m = 7; m >= 0; --m) {
            int q;
            if (pl_move(sW, gh, gw, j, i, m, &q) && sP[q] + (m < 4 ? 5u : 7u) * sW[q] == p) d = m;
          }
        }
      }
      a.potential[k] = fin ? p : CODD_PLAN_UNREACHED;
      if (a.dir) a.dir[k] = (unsigned char)d;
    }
    const int nf = __popcll(__ballot(fin));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned other = __shfl_xor(pmax, o, 64);
      pmax = other > pmax ? other : pmax;
    }
    if (lane == 0 && nf) {
      atomicAdd((int*)sI + PI_FINITE, nf);
      atomicMax((unsigned*)sI + PI_MAXP, pmax);
    }
  }
  __syncthreads();

  // ---- 4: the path, by wave 0 (every value below is the same in all its lanes)
  if (tid < 64) {
    const bool found = sW[s] != 0 && sP[s] < PL_INF;
    int n = 0, p = s, maxc = -1, len = 0;
    if (found) {
      const int m = lane & 7;
      while (true) {
        if (lane == 0 && n < a.max_path) a.path[n] = p;
        ++n;
        const int c = a.cost[p];
        if (c != CODD_COST_NO_INFO && c > maxc) maxc = c;
        const unsigned pp = sP[p];
        if (pp == 0 || n > cells) break;  // in G (P decreases strictly: fewer steps than cells)
        const int j = p / gw, i = p - j * gw;
        int q = 0;
        const bool hit = pl_move(sW, gh, gw, j, i, m, &q) && sP[q] + (m < 4 ? 5u : 7u) * sW[q] == pp;
        const unsigned best = (unsigned)(__ballot(hit) & 0xffull);
        if (!best) break;  // (never: P is a fixed point)
        const int k = __ffs(best) - 1;  // the smallest k that attains P
        p = __shfl(q, k, 64);
        len += k < 4 ? 5 : 7;
      }
    }
    if (lane == 0) {
      const int written = n < a.max_path ? n : a.max_path;
      sI[PI_WRITTEN] = written;
      double* r = a.record;
      r[0] = found ? 1.0 : 0.0;
      r[1] = found ? (double)sP[s] : -1.0;
      r[2] = (double)n;
      r[3] = (double)written;
      r[4] = have ? (double)(gj * gw + gi) : -1.0;
      r[5] = (double)clamped;
      r[6] = (double)snapped;
      r[7] = (double)n_goal;
      r[8] = found ? (double)p : -1.0;
      r[9] = (double)sI[PI_FINITE];
      r[10] = sI[PI_FINITE] ? (double)(unsigned)sI[PI_MAXP] : -1.0;
      r[11] = (double)maxc;
      r[12] = (double)len;
      r[13] = 0.0; r[14] = 0.0; r[15] = 0.0;
    }
  }
  __syncthreads();

  // ---- 5: -1 behind the path
  for (int k = sI[PI_WRITTEN] + tid; k < a.max_path; k += PL_THREADS) a.path[k] = -1;
}

static inline bool pl_shape_ok(int gh, int gw) {
  return gh >= 1 && gw >= 1 && (long long)gh * gw <= CODD_PLAN_MAX_CELLS;  // (a side may exceed codd_local_map's 4096: 1 x 25600)
}

extern "C" long long codd_plan_scratch(int gh, int gw) {
  return pl_shape_ok(gh, gw) ? 16 + 64 : -1;  // the alignment and the counters
}

extern "C" int codd_plan(const unsigned char* cost, const unsigned char* reach, const double* cost_record,
                         const double* map_record, int gh, int gw, int start_i, int start_j, int mode, int goal_i, int goal_j,
                         double goal_x, double goal_z, float cell, int goal_r2, int neutral, int factor, int unknown_cost,
                         int max_path, void* scratch, long long scratch_bytes, unsigned* potential, unsigned char* dir,
                         int* path, double* record, void* stream) {
  if (!cost || !reach || !potential || !path || !record || !scratch) return CODD_EINVAL;
  if (!pl_shape_ok(gh, gw) || start_i < 0 || start_i >= gw || start_j < 0 || start_j >= gh) return CODD_EINVAL;
  if (goal_r2 < 0 || max_path < 1 || neutral < 1 || neutral > 255 || factor < 0 || factor > 1024 || unknown_cost < 0 ||
      unknown_cost > 254)
    return CODD_EINVAL;
  if (mode == CODD_PLAN_GOAL_CELL) {
    if (goal_i < 0 || goal_i >= gw || goal_j < 0 || goal_j >= gh) return CODD_EINVAL;
  } else if (mode == CODD_PLAN_GOAL_WORLD) {
    if (!map_record || !(cell > 0.f) || !std::isfinite(cell) || !std::isfinite(goal_x) || !std::isfinite(goal_z)) return CODD_EINVAL;
    if (!(fabs(goal_x / (double)cell) < 1073741824.0) || !(fabs(goal_z / (double)cell) < 1073741824.0)) return CODD_EINVAL;
  } else if (mode == CODD_PLAN_GOAL_FRONTIER) {
    if (!cost_record) return CODD_EINVAL;
  } else {
    return CODD_EINVAL;
  }
  if (scratch_bytes < codd_plan_scratch(gh, gw)) return CODD_EINVAL;
  PlanArgs a;
  a.cost = cost; a.reach = reach; a.cost_record = cost_record; a.map_record = map_record;
  a.potential = potential; a.dir = dir; a.path = path; a.record = record;
  a.rounds = (int*)(((uintptr_t)scratch + 15) & ~(uintptr_t)15);
  a.goal_x = goal_x; a.goal_z = goal_z; a.cell = cell;
  a.gh = gh; a.gw = gw; a.start_i = start_i; a.start_j = start_j; a.mode = mode; a.goal_i = goal_i; a.goal_j = goal_j;
  a.goal_r2 = goal_r2; a.neutral = neutral; a.factor = factor; a.unknown_cost = unknown_cost; a.max_path = max_path;
  const size_t lds = PL_LDS((size_t)gh * gw);
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)plan_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  plan_kernel<<<1, PL_THREADS, lds, (hipStream_t)stream>>>(a);
  CODD_LAUNCH_CHECK();
  return CODD_OK;
}
