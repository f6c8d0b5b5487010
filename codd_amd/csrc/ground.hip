// codd_ground_plane: where is the floor?  (codd_amd/live.py, ground=)  A robust fit of ONE plane to the frame's disparity
// -- in disparity space a 3-D plane is a plane, d = c0 (x - cx) + c1 (y - cy) + c2, so the fit is a 3x3 problem whose noise
// is uniform in the measured quantity --, then per pixel the height above that plane (Hc e / d: one division), a label
// (floor, obstacle, overhead, below, invalid) and a scatter of the floor and obstacle pixels into a top-down grid on the
// plane.  The reference has no such output; what this replaces is downloading the depth map every frame and running a
// plane fit, a classification and a histogram on the host.  The contract, fixed to the fp32 operation, is in
// include/codd_hip.h.
//
// iters + 1 launches on one stream, no allocation, no host synchronisation:
//   pass k < iters  reads disp at the fit pixels, accumulates the weighted sums under c_k (c_0: the seed); pass 0 also clears
//                   the grid and the ticket, which the last pass -- a later launch -- uses;
//   pass iters      over the whole crop: statistics under the final c, labels, heights and the grid scatter; the record.
// The sums, the 3x3 solve and the ticket that picks the record's writer are fit_sums.h's scheme; on top of it every
// workgroup of the last pass derives the metric plane itself, and labels, heights and grid updates precede its ticket.
//
// The grid scatter: neighbouring pixels of a row mostly fall into the same cell (a near-field cell collects thousands of
// pixels), so a lane-per-pixel atomic serialises on a few addresses.  The cells of a 128 x 128 grid (192 KiB with both
// count planes and the heights) do not fit a workgroup's LDS, and a workgroup's pixels are a strip of rows whose cells are
// not bounded beforehand; so each wave first merges RUNS of equal cell indices among its 64 consecutive pixels -- a ballot
// gives the run length, a segmented shuffle maximum the run's height -- and only a run's first lane issues the atomics.
// Integer add and integer max do not depend on grouping or order: the bytes are those of one atomic per pixel.
#include "fit_sums.h"

#define GND_NS 10     // doubles per partial row: A (6), b (3), n; the last pass uses 3
#define GND_STATE 8   // doubles per state: c (3), alive, steps

struct GndArgs {
  const float* disp;
  double* partial;  // [2][FIT_NB][GND_NS]
  double* state;    // [2][GND_STATE]
  unsigned* ticket;
  double* record;
  unsigned char* labels;
  float* height;     // or NULL
  int* grid_count;   // [2][gh][gw] or NULL
  int* grid_height;  // [gh][gw], the bits of non-negative floats, or NULL
  double seed[3], up[3], max_tilt_deg;
  int W, h, w, step, k, iters, min_valid, seeded, gh, gw;
  float fx, fy, cx, cy, calib, s2_neg, s2_pos, delta, tol_px, ground_tol, clearance, cell;
};

struct GndPlane {
  double n[3], f[3], r[3], Hc, tilt;
  int ok;
};

// One step from the 10 sums s of a pass under the state st (thread 0 only; A, b: LDS work arrays).
// st: [0:3] c, [3] alive, [4] steps taken.
__device__ void gnd_step(const double* s, double* st, int min_valid, double (*A)[3], double* b) {
  if (st[3] == 0.0) return;  // stopped earlier: the last good iterate stays
  bool good = s[9] >= (double)min_valid;
  for (int i = 0; i < GND_NS; ++i) good = good && fabs(s[i]) < (double)INFINITY;  // (false for NaN)
  if (good) {
    int n = 0;
    for (int i = 0; i < 3; ++i)
      for (int j = i; j < 3; ++j) A[j][i] = s[n++];  // the lower triangle
    for (int i = 0; i < 3; ++i) b[i] = s[6 + i];
    good = fit_cholesky_solve<3>(A, b, FIT_PIVOT * (A[0][0] + A[1][1] + A[2][2]));
  }
  if (good) {
    for (int i = 0; i < 3; ++i) good = good && fabs(b[i]) < (double)INFINITY;
    if (good) {
      for (int i = 0; i < 3; ++i) st[i] = b[i];
      st[4] += 1.0;
    }
  }
  if (!good) {
    st[3] = 0.0;
    if (st[4] == 0.0) st[0] = st[1] = st[2] = 0.0;  // no good iterate: zeros, not the seed
  }
}

// the metric plane of the final c (thread 0 only), fp64: N.X = calib  <=>  d = c.p
__device__ void gnd_metric(const GndArgs& a, const double* st, GndPlane* m) {
  for (int i = 0; i < 3; ++i) m->n[i] = m->f[i] = m->r[i] = 0.0;
  m->Hc = m->tilt = 0.0;
  m->ok = 0;
  if (st[3] == 0.0) return;
  const double N[3] = {st[0] * (double)a.fx, st[1] * (double)a.fy, st[2]};
  const double nn = sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]);
  if (!(nn > 0.0) || !(nn < (double)INFINITY)) return;
  const double Hc = (double)a.calib / nn;
  if (!(Hc > 0.0) || !(Hc < (double)INFINITY)) return;
  m->Hc = Hc;
  for (int i = 0; i < 3; ++i) m->n[i] = -N[i] / nn;
  const double* n = m->n;
  double dot = (n[0] * a.up[0] + n[1] * a.up[1]) + n[2] * a.up[2];
  dot = dot > 1.0 ? 1.0 : dot < -1.0 ? -1.0 : dot;
  m->tilt = acos(dot) * (180.0 / 3.14159265358979323846);
  bool ok = m->tilt <= a.max_tilt_deg;
  const double g[3] = {-n[2] * n[0], -n[2] * n[1], 1.0 - n[2] * n[2]};  // z - (z.n) n
  const double gl = sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
  if (gl < 1e-3) {
    ok = false;  // the camera looks along the normal: no forward axis
  } else {
    double* f = m->f;
    for (int i = 0; i < 3; ++i) f[i] = g[i] / gl;
    m->r[0] = f[1] * n[2] - f[2] * n[1];  // r = f x n
    m->r[1] = f[2] * n[0] - f[0] * n[2];
    m->r[2] = f[0] * n[1] - f[1] * n[0];
  }
  m->ok = ok ? 1 : 0;
}

// LAST = false: a weighted pass k < iters over the fit pixels; LAST = true: pass iters over the whole crop
template <bool LAST>
__global__ __launch_bounds__(256) void gnd_pass_kernel(GndArgs a) {
#pragma clang fp contract(off)  // every operation of the contract rounds once
  constexpr int NACC = LAST ? 3 : GND_NS;
  __shared__ double sS[GND_NS], sF[4];
  __shared__ double sA[3][3], sB[3];
  __shared__ double sSt[GND_STATE];
  __shared__ double sRed[NACC][4];
  __shared__ GndPlane sM;
  const int tid = threadIdx.x, lane = tid & 63;

  // ---- the coefficients of this pass: pass k-1's rows -> one step on top of pass k-1's state
  if (a.k > 0) {
    double prev[GND_STATE];
    if (tid == 0) {  // (requested before the rows: one wait for memory)
#pragma unroll
      for (int i = 0; i < GND_STATE; ++i) prev[i] = a.state[((a.k - 1) & 1) * GND_STATE + i];
    }
    fit_sum_rows<GND_NS, GND_NS>(a.partial + (size_t)((a.k - 1) & 1) * FIT_NB * GND_NS, sS);
    __syncthreads();
    if (tid == 0) {
#pragma unroll
      for (int i = 0; i < GND_STATE; ++i) sSt[i] = prev[i];
      gnd_step(sS, sSt, a.min_valid, sA, sB);
    }
  } else if (tid == 0) {
    for (int i = 0; i < 3; ++i) sSt[i] = a.seeded ? a.seed[i] : 0.0;
    sSt[3] = 1.0;
    for (int i = 4; i < GND_STATE; ++i) sSt[i] = 0.0;
    if (blockIdx.x == 0) *a.ticket = 0u;  // (the last pass is a later launch)
  }
  if (tid == 0) {
    if (blockIdx.x == 0) {
      double* cur = a.state + (a.k & 1) * GND_STATE;
      for (int i = 0; i < GND_STATE; ++i) cur[i] = sSt[i];
    }
    if (LAST) gnd_metric(a, sSt, &sM);
  }
  __syncthreads();
  const float c0 = (float)sSt[0], c1 = (float)sSt[1], c2 = (float)sSt[2];

  double acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = 0.0;

  if constexpr (!LAST) {
    if (a.k == 0 && a.grid_count) {  // the entry clears the grid itself: nothing accumulates over calls
      const int cells = a.gh * a.gw;
      for (int i = blockIdx.x * 256 + tid; i < cells; i += FIT_NB * 256) {
        a.grid_count[i] = 0;
        a.grid_count[cells + i] = 0;
        a.grid_height[i] = 0;
      }
    }
    const int nx = (a.w + a.step - 1) / a.step, ny = (a.h + a.step - 1) / a.step;
    const long long n = (long long)nx * ny;
    const bool flat = a.k == 0 && !a.seeded;
    for (long long e = (long long)blockIdx.x * 256 + tid; e < n; e += (long long)FIT_NB * 256) {
      const int gy = (int)(e / nx), gx = (int)(e - (long long)gy * nx);
      const int x = gx * a.step, y = gy * a.step;
      const float d = a.disp[(size_t)y * a.W + x];
      if (!(d > 0.f && d < INFINITY)) continue;  // (NaN compares false)
      const float p0 = (float)x - a.cx, p1 = (float)y - a.cy;
      float wt;
      if (flat) {
        wt = (float)y >= a.cy ? 1.f : 0.f;
      } else {
        const float r = d - ((c0 * p0 + c1 * p1) + c2);
        wt = 1.f / (1.f + (r * r) / (r > 0.f ? a.s2_pos : a.s2_neg));
      }
      const float q0 = wt * p0, q1 = wt * p1;
      acc[0] += (double)(q0 * p0);
      acc[1] += (double)(q0 * p1);
      acc[2] += (double)q0;
      acc[3] += (double)(q1 * p1);
      acc[4] += (double)q1;
      acc[5] += (double)wt;
      acc[6] += (double)(q0 * d);
      acc[7] += (double)(q1 * d);
      acc[8] += (double)(wt * d);
      acc[9] += 1.0;
    }
  } else {
    const long long n = (long long)a.h * a.w;
    const int cells = a.gh * a.gw;
    const bool ok = sM.ok != 0;
    const float Hc = (float)sM.Hc;
    const float r0 = (float)sM.r[0], r1 = (float)sM.r[1], r2 = (float)sM.r[2];
    const float f0 = (float)sM.f[0], f1 = (float)sM.f[1], f2 = (float)sM.f[2];
    const float half = 0.5f * (float)a.gw;
    // (the trip count is the workgroup's: every lane takes part in the shuffles below)
    for (long long e0 = (long long)blockIdx.x * 256; e0 < n; e0 += (long long)FIT_NB * 256) {
      const long long e = e0 + tid;
      int key = -1, hb = 0;
      if (e < n) {
        const int y = (int)(e / a.w), x = (int)(e - (long long)y * a.w);
        const float d = a.disp[(size_t)y * a.W + x];
        const bool valid = d > 0.f && d < INFINITY;
        const float p0 = (float)x - a.cx, p1 = (float)y - a.cy;
        const float r = d - ((c0 * p0 + c1 * p1) + c2);
        if (valid && x % a.step == 0 && y % a.step == 0) {
          acc[0] += 1.0;
          if (fabsf(r) <= a.delta) { acc[1] += 1.0; acc[2] += (double)(r * r); }
        }
        unsigned char label = CODD_GROUND_INVALID;
        float hgt = NAN;
        if (ok && valid) {
          hgt = (Hc * r) / d;
          if (fabsf(r) <= a.tol_px || fabsf(hgt) <= a.ground_tol) label = CODD_GROUND_FLOOR;
          else if (hgt > a.clearance) label = CODD_GROUND_OVERHEAD;
          else if (hgt > 0.f) label = CODD_GROUND_OBSTACLE;
          else label = CODD_GROUND_BELOW;
          if (a.grid_count && label <= CODD_GROUND_OBSTACLE) {
            const float Z = a.calib / d;
            const float X0 = Z * (p0 / a.fx), X1 = Z * (p1 / a.fy);
            const float gx = (r0 * X0 + r1 * X1) + r2 * Z, gz = (f0 * X0 + f1 * X1) + f2 * Z;
            const float fi = floorf(gx / a.cell + half), fz = floorf(gz / a.cell);
            if (fi >= 0.f && fi < (float)a.gw && fz >= 0.f && fz < (float)a.gh) {  // (false for NaN)
              key = (int)label * cells + ((int)fz * a.gw + (int)fi);
              if (label == CODD_GROUND_OBSTACLE) hb = __float_as_int(hgt);  // hgt > 0: the bits order like the floats
            }
          }
        }
        a.labels[e] = label;
        if (a.height) a.height[e] = hgt;
      }
      if (a.grid_count) {
        // runs of equal keys among the wave's 64 consecutive pixels: the first lane of a run adds the run's length
        const int prev = __shfl_up(key, 1, 64);
        const bool first = lane == 0 || prev != key;
        const unsigned long long firsts = __ballot(first);
        const unsigned long long rest = lane == 63 ? 0ull : firsts >> (lane + 1);
        const int len = rest ? __ffsll((long long)rest) : 64 - lane;
        int v = hb;
        if (__ballot(hb != 0)) {  // segmented maximum towards the run's first lane
#pragma unroll
          for (int o = 1; o < 64; o <<= 1) {
            const int ov = __shfl_down(v, o, 64), ok_ = __shfl_down(key, o, 64);
            if (lane + o < 64 && ok_ == key && ov > v) v = ov;
          }
        }
        if (first && key >= 0) {
          atomicAdd(a.grid_count + key, len);
          if (key >= cells && v > 0) atomicMax(a.grid_height + (key - cells), v);
        }
      }
    }
  }

  fit_reduce_store<NACC>(acc, sRed, a.partial + ((size_t)(a.k & 1) * FIT_NB + blockIdx.x) * GND_NS);
  if (!LAST) return;

  // ---- the record: the workgroup that draws the last ticket adds the last pass's rows
  if (!fit_last_workgroup(a.ticket)) return;
  fit_sum_rows<GND_NS, 3>(a.partial + (size_t)(a.k & 1) * FIT_NB * GND_NS, sF);
  __syncthreads();
  const bool ok = sM.ok != 0 && sF[1] >= (double)a.min_valid;
  if (tid == 0) {
    double* rec = a.record;
    for (int i = 0; i < 3; ++i) rec[i] = fit_clean(sSt[i]);
    rec[3] = ok ? 1.0 : 0.0;
    rec[4] = sF[0];
    rec[5] = sF[1];
    rec[6] = sF[1] > 0.0 ? fit_clean(sqrt(sF[2] / sF[1])) : 0.0;
    rec[7] = sSt[4];
    for (int i = 0; i < 3; ++i) rec[8 + i] = fit_clean(sM.n[i]);
    rec[11] = fit_clean(sM.Hc);
    rec[12] = fit_clean(sM.tilt);
    for (int i = 0; i < 9; ++i) rec[13 + i] = fit_clean(sS[i]);  // the last step's A (upper triangle) and b
    for (int i = 0; i < 3; ++i) rec[22 + i] = fit_clean(sM.f[i]);
    for (int i = 25; i < 32; ++i) rec[i] = 0.0;
  }
  if (sM.ok != 0 && !ok) {
    // Too few inliers, known only now: every other workgroup's outputs are complete (their fences precede their
    // tickets), so this one takes them back.  The failing frame's cost; a frame that is ok never comes here.
    const long long n = (long long)a.h * a.w;
    for (long long e = tid; e < n; e += 256) {
      a.labels[e] = CODD_GROUND_INVALID;
      if (a.height) a.height[e] = NAN;
    }
    if (a.grid_count) {
      const int cells = a.gh * a.gw;
      for (int i = tid; i < cells; i += 256) {
        a.grid_count[i] = 0;
        a.grid_count[cells + i] = 0;
        a.grid_height[i] = 0;
      }
    }
  }
}

static inline bool gnd_grid_ok(int gh, int gw) {
  return (gh == 0 && gw == 0) || (gh > 0 && gw > 0 && (long long)gh * gw < (1LL << 30));
}

extern "C" long long codd_ground_scratch(int h, int w, int gh, int gw) {
  if (h <= 0 || w <= 0 || (long long)h * w >= (1LL << 31) || !gnd_grid_ok(gh, gw)) return -1;
  return fit_scratch_bytes(GND_NS, GND_STATE);
}

extern "C" int codd_ground_plane(const float* disp, int H, int W, int h, int w, float fx, float fy, float cx, float cy,
                                 float calib, const double* seed, const float* up, int step, int iters, float delta_px,
                                 float delta0_px, float asym, int min_valid, float max_tilt_deg, float tol_px,
                                 float ground_tol, float clearance, float cell, int gh, int gw, void* scratch,
                                 long long scratch_bytes, double* record, unsigned char* labels, float* height,
                                 int* grid_count, float* grid_height, void* stream) {
  if (!disp || !up || !scratch || !record || !labels) return CODD_EINVAL;
  if (H <= 0 || W <= 0 || h <= 0 || w <= 0 || h > H || w > W || (long long)h * w >= (1LL << 31)) return CODD_EINVAL;
  if ((grid_count != nullptr) != (grid_height != nullptr)) return CODD_EINVAL;
  if (gh < 0 || gw < 0 || !gnd_grid_ok(gh, gw)) return CODD_EINVAL;
  if (grid_count ? !(gh > 0 && gw > 0 && cell > 0.f && cell < INFINITY) : (gh != 0 || gw != 0)) return CODD_EINVAL;
  if (step < 1 || step > 8 || iters < 1 || iters > 32) return CODD_EINVAL;
  if (!(fx > 0.f && fx < INFINITY) || !(fy > 0.f && fy < INFINITY) || !(calib > 0.f && calib < INFINITY)) return CODD_EINVAL;
  if (!(fabsf(cx) < INFINITY) || !(fabsf(cy) < INFINITY)) return CODD_EINVAL;
  if (!(delta_px > 0.f && delta_px < INFINITY) || !(delta0_px > 0.f && delta0_px < INFINITY)) return CODD_EINVAL;
  if (!(asym >= 1.f && asym < INFINITY) || !((delta_px / asym) * (delta_px / asym) > 0.f)) return CODD_EINVAL;
  if (!(max_tilt_deg >= 0.f) || !(tol_px >= 0.f) || !(ground_tol >= 0.f) || !(clearance >= ground_tol)) return CODD_EINVAL;
  if (cell != cell) return CODD_EINVAL;
  double u[3] = {(double)up[0], (double)up[1], (double)up[2]};
  const double ul = sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
  if (!(ul > 0.0) || !(ul < (double)INFINITY)) return CODD_EINVAL;
  if (seed && !(fabs(seed[0]) < (double)INFINITY && fabs(seed[1]) < (double)INFINITY && fabs(seed[2]) < (double)INFINITY))
    return CODD_EINVAL;
  if (scratch_bytes < codd_ground_scratch(h, w, gh, gw)) return CODD_EINVAL;
  const FitScratch f = fit_carve(scratch, GND_NS, GND_STATE);
  GndArgs a;
  a.disp = disp;
  a.partial = f.partial; a.state = f.state; a.ticket = f.ticket;
  a.record = record; a.labels = labels; a.height = height;
  a.grid_count = grid_count; a.grid_height = (int*)grid_height;
  for (int i = 0; i < 3; ++i) { a.seed[i] = seed ? seed[i] : 0.0; a.up[i] = u[i] / ul; }
  a.max_tilt_deg = (double)max_tilt_deg;
  a.W = W; a.h = h; a.w = w; a.step = step; a.iters = iters; a.min_valid = min_valid; a.seeded = seed ? 1 : 0;
  a.gh = grid_count ? gh : 0; a.gw = grid_count ? gw : 0;
  a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.calib = calib;
  a.delta = delta_px; a.tol_px = tol_px; a.ground_tol = ground_tol; a.clearance = clearance; a.cell = cell;
  a.s2_neg = a.s2_pos = 1.f;
  hipStream_t s = (hipStream_t)stream;
  for (int k = 0; k <= iters; ++k) {
    a.k = k;
    if (k < iters) {
      // s_k = max(delta_px, delta0_px * 0.5^k) (the product is exact), s_k / asym for e > 0, their squares: fp32, once
      const float sk = fmaxf(delta_px, ldexpf(delta0_px, -k)), sp = sk / asym;
      a.s2_neg = sk * sk;
      a.s2_pos = sp * sp;
      gnd_pass_kernel<false><<<FIT_NB, 256, 0, s>>>(a);
    } else {
      gnd_pass_kernel<true><<<FIT_NB, 256, 0, s>>>(a);
    }
    CODD_LAUNCH_CHECK();
  }
  return CODD_OK;
}
