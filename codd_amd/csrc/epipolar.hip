// codd_epipolar_check: is the rig still rectified?  (codd_amd/live.py, epipolar=)  Per measured pixel the row offset dy at
// which the right image really matches the left one -- L(x, y) ~ R(x - d, y + dy) with the frame's own disparity d -- and a
// robust four-parameter fit of that vertical-disparity map: a small rotation of the right view plus a focal ratio.  The
// reference has no such output; what this replaces is downloading the disparity and both images every frame and running
// a block matcher on the host.  The contract, fixed to the fp32 operation, is in include/codd_hip.h.
//
// 2 + iters launches on one stream, no allocation, no host synchronisation:
//   grey            both normalised [3,H,W] images -> two compact [h,w] grey planes in the caller's scratch (8 bytes per
//                   crop pixel); every tap of the matcher is then ONE load instead of three loads and five operations,
//                   and a tap is read by up to 27 (2V + 1) / step^2 measured pixels;
//   measure (k = 0) a lane owns one measured pixel: the 27 left taps in registers, then the 3 + 2V right rows one after
//                   the other, each interpolated ONCE (10 loads -> 9 values) and added to the candidates it belongs to, so
//                   C(v) gets its three row sums in the order j = -1, 0, 1; the lane writes dy and the NaN of the step x step
//                   block it stands for, and accumulates the L2 step's sums;
//   pass k < iters  reads disp and dy at the measured pixels, accumulates the Cauchy-weighted sums under c_k;
//   pass iters      the statistics under the final c, and the record.
// The planes are read from global memory, not staged in LDS: the right-image address is x - d, so a workgroup's strip of
// the right plane would have to span its pixels' whole disparity range (unknown before the disparity is read) over 3 + 2V
// rows, which bounds the supported width; the two planes of a 960 x 540 frame are 4 MB, each XCD's L2 holds 4 MiB and a
// wave's taps are 10 consecutive floats per row and lane, `step` floats apart between lanes, where the disparity is smooth
// -- the vector cache and the L2 serve the reuse, there is no width limit and no second code path.
//
// The sums of the measure and fit passes, the 4x4 solve and the ticket that picks the record's writer are fit_sums.h's
// scheme.
#include "fit_sums.h"

#define EPI_NS 16      // doubles per partial row: A (10), b (4), n, sum dy^2; the last pass uses 4
#define EPI_STATE 8    // doubles per state: c (4), alive, steps
#define EPI_RX 4
#define EPI_RY 1

struct EpiArgs {
  const float* disp;
  const float* left;
  const float* right;
  float* gl;        // [h,w]
  float* gr;        // [h,w]
  float* map;       // [h,w]: the caller's dy_map, or the scratch
  double* partial;  // [2][FIT_NB][EPI_NS]
  double* state;    // [2][EPI_STATE]
  unsigned* ticket;
  double* record;
  size_t N;  // H * W
  int W, h, w, step, k, iters, min_valid;
  float s0, s1, s2, fx, fy, cx, cy, tau27, curv27, delta;
};

__global__ __launch_bounds__(256) void epi_grey_kernel(EpiArgs a) {
#pragma clang fp contract(off)  // every operation of the contract rounds once
  const long long n = (long long)a.h * a.w;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
    const int y = (int)(e / a.w), x = (int)(e - (long long)y * a.w);
    const size_t p = (size_t)y * a.W + x;
    a.gl[e] = ((a.left[p] * a.s0 + a.left[a.N + p] * a.s1) + a.left[2 * a.N + p] * a.s2) * (1.f / 3.f);
    a.gr[e] = ((a.right[p] * a.s0 + a.right[a.N + p] * a.s1) + a.right[2 * a.N + p] * a.s2) * (1.f / 3.f);
  }
}

// dy of the measured pixel (x, y), NaN if it is not measurable
template <int V>
__device__ __forceinline__ float epi_measure(const EpiArgs& a, int x, int y) {
#pragma clang fp contract(off)
  constexpr int RX = EPI_RX, RY = EPI_RY, NV = 2 * V + 1;
  const float d = a.disp[(size_t)y * a.W + x];
  if (!(d > 0.f && d < INFINITY)) return NAN;  // (NaN compares false)
  if (x - RX < 0 || x + RX >= a.w || y - RY - V < 0 || y + RY + V >= a.h) return NAN;
  const float u = (float)x - d, uf = floorf(u);
  if (!(uf >= (float)RX)) return NAN;  // f - RX < 0
  const int f = (int)uf;               // RX <= f <= x < w
  if (f + RX + 1 >= a.w) return NAN;
  const float al = u - uf, be = 1.f - al;
  float L[2 * RY + 1][2 * RX + 1];
#pragma unroll
  for (int j = 0; j <= 2 * RY; ++j) {
    const float* __restrict__ lp = a.gl + (size_t)(y + j - RY) * a.w + (x - RX);
#pragma unroll
    for (int i = 0; i <= 2 * RX; ++i) L[j][i] = lp[i];
  }
  float C[NV];
#pragma unroll
  for (int r = -(RY + V); r <= RY + V; ++r) {
    const float* __restrict__ rp = a.gr + (size_t)(y + r) * a.w + (f - RX);
    float q[2 * RX + 2], R[2 * RX + 1];
#pragma unroll
    for (int i = 0; i <= 2 * RX + 1; ++i) q[i] = rp[i];
#pragma unroll
    for (int i = 0; i <= 2 * RX; ++i) R[i] = q[i] * be + q[i + 1] * al;
#pragma unroll
    for (int v = -V; v <= V; ++v) {
      const int j = r - v;  // this right row is row j of candidate v's window
      if (j < -RY || j > RY) continue;
      float s = fabsf(L[j + RY][0] - R[0]);
#pragma unroll
      for (int i = 1; i <= 2 * RX; ++i) s = s + fabsf(L[j + RY][i] - R[i]);
      C[v + V] = j == -RY ? s : C[v + V] + s;
    }
  }
  // arg-min; ties: the smaller |v|, then the smaller v
  int vb = 0;
  float best = C[V];
#pragma unroll
  for (int m = 1; m <= V; ++m) {
    if (C[V - m] < best) { best = C[V - m]; vb = -m; }
    if (C[V + m] < best) { best = C[V + m]; vb = m; }
  }
  if (vb == -V || vb == V) return NAN;
  float cm = 0.f, cp = 0.f;
#pragma unroll
  for (int v = -V + 1; v <= V - 1; ++v)
    if (v == vb) { cm = C[v + V - 1]; cp = C[v + V + 1]; }
  const float den = (cm - 2.f * best) + cp;
  if (!(den > a.curv27) || !(den > 0.f)) return NAN;
  if (!(best <= a.tau27)) return NAN;
  return (float)vb + (cm - cp) / (2.f * den);
}

struct EpiTerms { float p[4], e; };

__device__ __forceinline__ EpiTerms epi_terms(const EpiArgs& a, int x, int y, float d, float dy, const float* c) {
#pragma clang fp contract(off)
  EpiTerms t;
  const float u = (float)x - d;
  const float xr = (u - a.cx) / a.fx, yn = ((float)y - a.cy) / a.fy;
  t.p[0] = a.fy * (1.f + yn * yn);
  t.p[1] = a.fy * (xr * yn);
  t.p[2] = a.fy * xr;
  t.p[3] = a.fy * yn;
  t.e = dy - (((c[0] * t.p[0] + c[1] * t.p[1]) + c[2] * t.p[2]) + c[3] * t.p[3]);
  return t;
}

// the 16 sums of a Gauss-Newton pass: A's upper triangle row by row, b, n, sum dy^2
__device__ __forceinline__ void epi_accumulate(const EpiTerms& t, float wt, float dy, double* acc) {
#pragma clang fp contract(off)
  float q[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = wt * t.p[i];
  int n = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = i; j < 4; ++j) acc[n++] += (double)(q[i] * t.p[j]);
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[10 + i] += (double)(q[i] * dy);
  acc[14] += 1.0;
  acc[15] += (double)(dy * dy);
}

// One step from the 16 sums s of a pass under the state st (thread 0 only; A, b: LDS work arrays).
// st: [0:4] c, [4] alive, [5] steps taken.
__device__ void epi_step(const double* s, double* st, int min_valid, double (*A)[4], double* b) {
  if (st[4] == 0.0) return;  // stopped earlier: the last good iterate stays
  bool good = s[14] >= (double)min_valid;
  for (int i = 0; i < EPI_NS; ++i) good = good && fabs(s[i]) < (double)INFINITY;  // (false for NaN)
  if (good) {
    int n = 0;
    for (int i = 0; i < 4; ++i)
      for (int j = i; j < 4; ++j) A[j][i] = s[n++];  // the lower triangle
    for (int i = 0; i < 4; ++i) b[i] = s[10 + i];
    good = fit_cholesky_solve<4>(A, b, FIT_PIVOT * (A[0][0] + A[1][1] + A[2][2] + A[3][3]));
  }
  if (good) {
    for (int i = 0; i < 4; ++i) good = good && fabs(b[i]) < (double)INFINITY;
    if (good) {
      for (int i = 0; i < 4; ++i) st[i] = b[i];
      st[5] += 1.0;
    }
  }
  if (!good) st[4] = 0.0;
}

// V > 0: the measure pass (k = 0) with search range V; V = 0: a Cauchy-weighted pass; V = -1: the last pass
template <int V>
__global__ __launch_bounds__(256) void epi_pass_kernel(EpiArgs a) {
#pragma clang fp contract(off)
  constexpr int NACC = V == -1 ? 4 : EPI_NS;
  __shared__ double sS[EPI_NS], sF[4];
  __shared__ double sA[4][4], sB[4];
  __shared__ double sSt[EPI_STATE];
  __shared__ double sRed[NACC][4];
  const int tid = threadIdx.x;

  // ---- the coefficients of this pass: pass k-1's rows -> one step on top of pass k-1's state
  if (V <= 0) {
    double prev[EPI_STATE] = {0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};  // pass 1 starts from c = 0, alive
    if (tid == 0 && a.k > 1) {  // (requested before the rows: one wait for memory)
#pragma unroll
      for (int i = 0; i < EPI_STATE; ++i) prev[i] = a.state[((a.k - 1) & 1) * EPI_STATE + i];
    }
    fit_sum_rows<EPI_NS, EPI_NS>(a.partial + (size_t)((a.k - 1) & 1) * FIT_NB * EPI_NS, sS);
    __syncthreads();
    if (tid == 0) {
#pragma unroll
      for (int i = 0; i < EPI_STATE; ++i) sSt[i] = prev[i];
      epi_step(sS, sSt, a.min_valid, sA, sB);
      if (blockIdx.x == 0) {
        double* cur = a.state + (a.k & 1) * EPI_STATE;
        for (int i = 0; i < EPI_STATE; ++i) cur[i] = sSt[i];
      }
    }
    __syncthreads();
  } else if (tid == 0 && blockIdx.x == 0) {
    *a.ticket = 0u;  // (the last pass is a later launch)
  }
  float c[4] = {0.f, 0.f, 0.f, 0.f};
  if (V <= 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = (float)sSt[i];
  }

  double acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = 0.0;
  const int nx = (a.w + a.step - 1) / a.step, ny = (a.h + a.step - 1) / a.step;
  const long long n = (long long)nx * ny;
  const float d2 = a.delta * a.delta;
  for (long long e = (long long)blockIdx.x * 256 + tid; e < n; e += (long long)FIT_NB * 256) {
    const int gy = (int)(e / nx), gx = (int)(e - (long long)gy * nx);
    const int x = gx * a.step, y = gy * a.step;
    float dy;
    if constexpr (V > 0) {
      dy = epi_measure<V>(a, x, y);
      // the step x step block this pixel stands for: dy in its corner, NaN elsewhere
      for (int jj = 0; jj < a.step && y + jj < a.h; ++jj)
        for (int ii = 0; ii < a.step && x + ii < a.w; ++ii)
          a.map[(size_t)(y + jj) * a.w + (x + ii)] = (ii | jj) ? NAN : dy;
    } else {
      dy = a.map[(size_t)y * a.w + x];
    }
    if (!(dy == dy)) continue;  // not measurable
    const EpiTerms t = epi_terms(a, x, y, a.disp[(size_t)y * a.W + x], dy, c);
    if (V == -1) {
      acc[0] += 1.0;
      acc[1] += (double)(dy * dy);
      if (fabsf(t.e) <= a.delta) { acc[2] += 1.0; acc[3] += (double)(t.e * t.e); }
    } else {
      epi_accumulate(t, V > 0 ? 1.f : 1.f / (1.f + (t.e * t.e) / d2), dy, acc);
    }
  }
  fit_reduce_store<NACC>(acc, sRed, a.partial + ((size_t)(a.k & 1) * FIT_NB + blockIdx.x) * EPI_NS);
  if (V != -1) return;

  // ---- the record: the workgroup that draws the last ticket adds the last pass's rows
  if (!fit_last_workgroup(a.ticket)) return;
  fit_sum_rows<EPI_NS, 4>(a.partial + (size_t)(a.k & 1) * FIT_NB * EPI_NS, sF);
  __syncthreads();
  if (tid == 0) {
    double* rec = a.record;
    for (int i = 0; i < 4; ++i) rec[i] = sSt[i];
    rec[4] = sSt[4] != 0.0 ? 1.0 : 0.0;
    rec[5] = sF[0];
    rec[6] = sF[2];
    rec[7] = sF[0] > 0.0 ? fit_clean(sqrt(sF[1] / sF[0])) : 0.0;
    rec[8] = sF[2] > 0.0 ? fit_clean(sqrt(sF[3] / sF[2])) : 0.0;
    rec[9] = sSt[5];
    for (int i = 0; i < 14; ++i) rec[10 + i] = fit_clean(sS[i]);  // the last step's A (upper triangle) and b
    for (int i = 24; i < 32; ++i) rec[i] = 0.0;
  }
}

extern "C" long long codd_epipolar_scratch(int h, int w) {
  if (h <= 0 || w <= 0 || (long long)h * w >= (1LL << 31)) return -1;
  return fit_scratch_bytes(EPI_NS, EPI_STATE) + 12LL * h * w;  // two grey planes, the map
}

extern "C" int codd_epipolar_check(const float* disp, const float* left, const float* right, int H, int W, int h, int w,
                                   const float* stdv, float fx, float fy, float cx, float cy, int range_px, int step,
                                   float tau, float min_curv, int iters, float delta_px, int min_valid, void* scratch,
                                   long long scratch_bytes, double* record, float* dy_map, void* stream) {
  if (!disp || !left || !right || !stdv || !scratch || !record) return CODD_EINVAL;
  if (H <= 0 || W <= 0 || h <= 0 || w <= 0 || h > H || w > W || (long long)h * w >= (1LL << 31)) return CODD_EINVAL;
  if (range_px < 1 || range_px > 4 || step < 1 || step > 8 || iters < 1 || iters > 32) return CODD_EINVAL;
  if (!(fx > 0.f) || !(fy > 0.f) || !(delta_px > 0.f) || tau != tau || min_curv != min_curv) return CODD_EINVAL;
  if (scratch_bytes < codd_epipolar_scratch(h, w)) return CODD_EINVAL;
  const FitScratch f = fit_carve(scratch, EPI_NS, EPI_STATE);
  const size_t n = (size_t)h * w;
  EpiArgs a;
  a.disp = disp; a.left = left; a.right = right;
  a.partial = f.partial; a.state = f.state; a.ticket = f.ticket;
  a.gl = (float*)f.rest;
  a.gr = a.gl + n;
  a.map = dy_map ? dy_map : a.gr + n;
  a.record = record;
  a.N = (size_t)H * W;
  a.W = W; a.h = h; a.w = w; a.step = step; a.iters = iters; a.min_valid = min_valid;
  a.s0 = stdv[0]; a.s1 = stdv[1]; a.s2 = stdv[2];
  a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy;
  a.tau27 = 27.f * tau; a.curv27 = 27.f * min_curv; a.delta = delta_px;
  hipStream_t s = (hipStream_t)stream;
  a.k = 0;
  const long long gb = ((long long)n + 255) / 256;
  epi_grey_kernel<<<(unsigned)(gb < 2048 ? gb : 2048), 256, 0, s>>>(a);
  CODD_LAUNCH_CHECK();
  switch (range_px) {
    case 1: epi_pass_kernel<1><<<FIT_NB, 256, 0, s>>>(a); break;
    case 2: epi_pass_kernel<2><<<FIT_NB, 256, 0, s>>>(a); break;
    case 3: epi_pass_kernel<3><<<FIT_NB, 256, 0, s>>>(a); break;
    default: epi_pass_kernel<4><<<FIT_NB, 256, 0, s>>>(a); break;
  }
  CODD_LAUNCH_CHECK();
  for (int k = 1; k <= iters; ++k) {
    a.k = k;
    if (k < iters) epi_pass_kernel<0><<<FIT_NB, 256, 0, s>>>(a);
    else epi_pass_kernel<-1><<<FIT_NB, 256, 0, s>>>(a);
    CODD_LAUNCH_CHECK();
  }
  return CODD_OK;
}
