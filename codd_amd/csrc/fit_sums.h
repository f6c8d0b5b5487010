// Fixed-order sums and the small solve of the robust fits that run entirely on the device: codd_ego_motion (ego.hip, 6
// unknowns), codd_epipolar_check (epipolar.hip, 4) and codd_ground_plane (ground.hip, 3).  Each promises equal bytes for
// equal inputs, no host synchronisation and no float atomics, and keeps the promise with the pieces below.
//
// Every pass is one launch of FIT_NB workgroups of 256 threads that stride over the pixels.  Per-pixel terms are fp32,
// every sum over more than one pixel is fp64: lane -> wave butterfly -> LDS -> ONE partial row per workgroup
// (fit_reduce_store).  There is no finish launch between passes and no grid barrier: every workgroup of pass k first adds
// pass k-1's FIT_NB rows in index order (fit_sum_rows: a fixed order, so the same bits in every workgroup and in every
// run), solves the small system (fit_cholesky_solve) and moves the state itself.  Rows and state are double-buffered by
// the parity of k, so no workgroup reads what another one of the same launch writes.  The record needs sums of the last
// pass itself: its workgroups take a ticket and the one that draws the last adds the rows, again in index order
// (fit_last_workgroup).  The scratch block is rows, states, ticket (fit_scratch_bytes, fit_carve); what a stage keeps
// per pixel lies behind it.
//
// What differs per stage stays in its file: the per-pixel terms, where the first state comes from, the gates around the
// solve, what a good step does to the state, and the record.
#pragma once
#include "common.h"

#define FIT_NB 256        // workgroups of every pass (about one per CU of the MI355X), and the number of partial rows
#define FIT_PIVOT 1e-12   // a Cholesky pivot <= FIT_PIVOT * trace stops the fit

// s[0:NCOL] = columns [0, NCOL) of the FIT_NB partial rows (NS doubles each), added in index order: wave v takes columns
// v, v + 4, ..; lane l adds rows l, l + 64, l + 128, l + 192 in that order, then the butterfly.  The rows were written by
// another launch or behind fit_last_workgroup, on other XCDs: every load of a lane is requested before the first is
// used, so the wave waits for memory once, not once per column.  All 256 threads call; s is valid after a barrier.
template <int NS, int NCOL>
__device__ __forceinline__ void fit_sum_rows(const double* __restrict__ rows, double* s) {
  constexpr int NC = (NCOL + 3) / 4, NR = FIT_NB / 64;
  constexpr bool GUARD = NCOL % 4 != 0;  // the last round of columns is not full
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double r[NC][NR];
#pragma unroll
  for (int i = 0; i < NC; ++i)
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const int col = wave + 4 * i;
      r[i][j] = !GUARD || col < NCOL ? rows[(size_t)(lane + 64 * j) * NS + col] : 0.0;
    }
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    double v = 0.0;
#pragma unroll
    for (int j = 0; j < NR; ++j) v += r[i][j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0 && (!GUARD || wave + 4 * i < NCOL)) s[wave + 4 * i] = v;
  }
}

// The workgroup's NACC accumulators -> row[0:NACC]: butterfly, the four waves' sums through LDS, added in wave order.
template <int NACC>
__device__ __forceinline__ void fit_reduce_store(const double* acc, double (*red)[4], double* row) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int i = 0; i < NACC; ++i) {
    double v = acc[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) red[i][wave] = v;
  }
  __syncthreads();
  if (tid < NACC) row[tid] = red[tid][0] + red[tid][1] + red[tid][2] + red[tid][3];
}

// True in exactly one workgroup of the launch: the one that draws ticket FIT_NB - 1, which may then read everything the
// others wrote before they called.  All 256 threads call, after the workgroup's last global write; *ticket is 0 before
// the launch (an earlier launch of the same call clears it).
//   fence 1    every thread's own writes -- its element of the row and, in ground.hip, its labels, heights and grid
//              atomics -- are written back device-wide before the thread passes the barrier, so before the ticket;
//   ticket     a device-scope integer atomic, taken by thread 0 behind that barrier: drawing FIT_NB - 1 means every
//              other workgroup's fence 1 has completed;
//   fence 2    in the last workgroup only, behind the barrier that publishes the ticket: it drops what this CU's
//              vector cache holds, so the loads that follow (the rows; ground.hip's take-back writes follow them) see
//              the other workgroups' bytes, not a stale line.
__device__ __forceinline__ bool fit_last_workgroup(unsigned* ticket) {
  __shared__ unsigned last;
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) last = atomicAdd(ticket, 1u) == (unsigned)(FIT_NB - 1);
  __syncthreads();
  if (!last) return false;
  __threadfence();
  return true;
}

// Solves A x = b for a symmetric A given by its lower triangle in the N x N LDS array A: Cholesky in place, stopping at
// a pivot <= floor (false; A and b are then partly overwritten), then forward and back substitution into b (true).
// One thread runs this while the workgroup waits: the factorisation stays a loop over the columns (unrolled it costs
// registers that the pixel loop's occupancy pays for).
template <int N>
__device__ __forceinline__ bool fit_cholesky_solve(double (*A)[N], double* b, double floor) {
#pragma unroll 1
  for (int j = 0; j < N; ++j) {
    double d = A[j][j];
    for (int k = 0; k < j; ++k) d -= A[j][k] * A[j][k];
    if (!(d > floor)) return false;  // (NaN too)
    const double l = sqrt(d);
    A[j][j] = l;
    for (int i = j + 1; i < N; ++i) {
      double v = A[i][j];
      for (int k = 0; k < j; ++k) v -= A[i][k] * A[j][k];
      A[i][j] = v / l;
    }
  }
  for (int i = 0; i < N; ++i) {
    double v = b[i];
    for (int k = 0; k < i; ++k) v -= A[i][k] * b[k];
    b[i] = v / A[i][i];
  }
  for (int i = N - 1; i >= 0; --i) {
    double v = b[i];
    for (int k = i + 1; k < N; ++k) v -= A[k][i] * b[k];
    b[i] = v / A[i][i];
  }
  return true;
}

// a record entry: 0 for what is not finite
__device__ __forceinline__ double fit_clean(double v) { return fabs(v) < (double)INFINITY ? v : 0.0; }

// ---- the scratch block: [2][FIT_NB][ns] rows, [2][state] states, the ticket; 16-byte aligned by the call itself
struct FitScratch {
  double* partial;
  double* state;
  unsigned* ticket;
  char* rest;  // 16-byte aligned: the stage's per-pixel planes
};

static inline long long fit_block_bytes(int ns, int state) { return 8LL * (2 * FIT_NB * ns + 2 * state) + 16; }

// bytes a caller provides for the block: 16 of slack for the alignment in front of it
static inline long long fit_scratch_bytes(int ns, int state) { return 16 + fit_block_bytes(ns, state); }

static inline FitScratch fit_carve(void* scratch, int ns, int state) {
  char* base = (char*)(((uintptr_t)scratch + 15) & ~(uintptr_t)15);
  FitScratch f;
  f.partial = (double*)base;
  f.state = f.partial + 2 * FIT_NB * ns;
  f.ticket = (unsigned*)(f.state + 2 * state);
  f.rest = base + fit_block_bytes(ns, state);
  return f;
}
