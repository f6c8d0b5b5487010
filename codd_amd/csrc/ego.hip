// Camera ego-motion and moving-pixel mask from the frame's dense SE3 field (codd_amd/live.py, egomotion=): a robust
// rigid fit G of the field over the cropped image -- Gauss-Newton / IRLS on a Cauchy likelihood from G = identity -- and
// the per-pixel residual flow against it.  The reference has no such output; what this replaces is the fit a user of
// outputs["Ts"] (raft3d.py:268-270) writes with torch: dozens of launches over every pixel and a host sync for the 6x6
// solve in every iteration.
//
// iters + 1 launches on one stream, no allocation, no host synchronisation:
//   pass 0          reads T (28 bytes / pixel) and depth_prev, writes X1 = T * X0 compactly (12 bytes / pixel) into the
//                   caller's scratch and accumulates the L2 step's sums;
//   pass k < iters  reads depth_prev and X1, accumulates the Cauchy-weighted sums under G_k;
//   pass iters      the mask pass: residual flow and mask under the final G, and the inlier statistics.
// The sums, the 6x6 solve and the ticket that picks the record's writer are fit_sums.h's scheme; a good step composes
// the pose in fp64 and rounds it to fp32, which is what the per-pixel arithmetic uses.
#include "fit_sums.h"
#include "se3.h"

#define EGO_NS 20      // doubles per partial row: 17 sums of a Gauss-Newton pass (3 of the mask pass), padded
#define EGO_STATE 16   // doubles per pose state: t, q, alive, steps

struct EgoArgs {
  const float* T;
  const float* depth;
  float* x1;
  double* partial;  // [2][FIT_NB][EGO_NS]
  double* state;    // [2][EGO_STATE]
  unsigned* ticket;
  float* record;
  unsigned char* moving;
  float* residual;
  int W, h, w, k, iters, min_valid;
  float fx, fy, cx, cy, scale, delta, tau;  // delta = delta_px / fx
};

// ---- fp64 SE3 pieces of the pose update (se3.h's expressions and branch thresholds, in double) -----------------------
struct D3 { double x, y, z; };
__device__ __forceinline__ D3 dcross(D3 a, D3 b) { return D3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

// G <- se3_exp(xi) * G, quaternion renormalised; g = [t(3), q_xyzw(4)]
__device__ void ego_apply(const double* xi, double* g) {
  const D3 tau{xi[0], xi[1], xi[2]}, phi{xi[3], xi[4], xi[5]};
  const double th2 = phi.x * phi.x + phi.y * phi.y + phi.z * phi.z, th = sqrt(th2), th4 = th2 * th2;
  const bool small = th2 < (double)SE3_EPS;
  const double imag = small ? 0.5 - th2 / 48.0 + th4 / 3840.0 : sin(0.5 * th) / th;
  const double real = small ? 1.0 - th2 / 8.0 + th4 / 384.0 : cos(0.5 * th);
  const double c1 = small ? 0.5 - th2 / 24.0 : (1.0 - cos(th)) / th2;
  const double c2 = small ? 1.0 / 6.0 - th2 / 120.0 : (th - sin(th)) / (th2 * th);
  const D3 pv = dcross(phi, tau), ppv = dcross(phi, pv);
  const D3 te{tau.x + c1 * pv.x + c2 * ppv.x, tau.y + c1 * pv.y + c2 * ppv.y, tau.z + c1 * pv.z + c2 * ppv.z};
  const D3 u{imag * phi.x, imag * phi.y, imag * phi.z};
  // t' = R(qe) t + te
  const D3 t{g[0], g[1], g[2]};
  D3 uv = dcross(u, t);
  uv = D3{2.0 * uv.x, 2.0 * uv.y, 2.0 * uv.z};
  const D3 uuv = dcross(u, uv);
  const double tx = t.x + real * uv.x + uuv.x + te.x, ty = t.y + real * uv.y + uuv.y + te.y, tz = t.z + real * uv.z + uuv.z + te.z;
  // q' = qe (x) q
  const D3 ub{g[3], g[4], g[5]};
  const double wb = g[6];
  const D3 c = dcross(u, ub);
  double qx = real * ub.x + wb * u.x + c.x, qy = real * ub.y + wb * u.y + c.y, qz = real * ub.z + wb * u.z + c.z;
  double qw = real * wb - (u.x * ub.x + u.y * ub.y + u.z * ub.z);
  const double n = sqrt(qx * qx + qy * qy + qz * qz + qw * qw);
  qx /= n; qy /= n; qz /= n; qw /= n;
  g[0] = tx; g[1] = ty; g[2] = tz; g[3] = qx; g[4] = qy; g[5] = qz; g[6] = qw;
}

// One Gauss-Newton step from the 17 sums s of a pass under the pose st (thread 0 only; A, b: LDS work arrays).
// st: [0:7] the pose, rounded to fp32 (what the per-pixel arithmetic uses); [7] alive; [8] steps taken.
__device__ void ego_step(const double* s, double* st, int min_valid, double (*A)[6], double* b) {
  if (st[7] == 0.0) return;  // stopped earlier: the last good iterate stays
  bool good = s[16] >= (double)min_valid;
  for (int i = 0; i < 17; ++i) good = good && fabs(s[i]) < (double)INFINITY;  // (false for NaN)
  if (good) {
    for (int i = 0; i < 6; ++i)
      for (int j = 0; j < 6; ++j) A[i][j] = 0.0;
    const double sw = s[0], ax = s[1], ay = s[2], az = s[3];
    const double tr = s[4] + s[7] + s[9];
    A[0][0] = A[1][1] = A[2][2] = sw;
    // -[a]x in the upper right block, its transpose below
    A[0][4] = az; A[0][5] = -ay; A[1][3] = -az; A[1][5] = ax; A[2][3] = ay; A[2][4] = -ax;
    A[4][0] = az; A[5][0] = -ay; A[3][1] = -az; A[5][1] = ax; A[3][2] = ay; A[4][2] = -ax;
    A[3][3] = tr - s[4]; A[3][4] = -s[5]; A[3][5] = -s[6];
    A[4][3] = -s[5]; A[4][4] = tr - s[7]; A[4][5] = -s[8];
    A[5][3] = -s[6]; A[5][4] = -s[8]; A[5][5] = tr - s[9];
    for (int i = 0; i < 6; ++i) b[i] = -s[10 + i];
    good = fit_cholesky_solve<6>(A, b, FIT_PIVOT * (3.0 * sw + 2.0 * tr));  // x trace(H)
  }
  if (good) {
    double g[7];
    for (int i = 0; i < 7; ++i) g[i] = st[i];
    ego_apply(b, g);
    for (int i = 0; i < 7; ++i) good = good && fabs(g[i]) < (double)INFINITY;
    if (good) {
      for (int i = 0; i < 7; ++i) st[i] = (double)(float)g[i];
      st[8] += 1.0;
    }
  }
  if (!good) st[7] = 0.0;
}

__device__ __forceinline__ bool ego_finite3(V3 a) {
  return fabsf(a.x) < INFINITY && fabsf(a.y) < INFINITY && fabsf(a.z) < INFINITY;  // (false for NaN)
}

// PASS 0: first pass (T -> X1, L2 weights); 1: a Cauchy-weighted pass; 2: the mask pass
template <int PASS>
__global__ __launch_bounds__(256) void ego_pass_kernel(EgoArgs a) {
  constexpr int NACC = PASS == 2 ? 3 : 17;
  __shared__ double sS[EGO_NS];
  __shared__ double sSt[EGO_STATE];
  __shared__ double sA[6][6], sB[6];
  __shared__ double sRed[NACC][4];
  const int tid = threadIdx.x;

  // ---- the pose of this pass: pass k-1's rows -> one Gauss-Newton step on top of pass k-1's pose
  if (PASS != 0) {
    fit_sum_rows<EGO_NS, 17>(a.partial + (size_t)((a.k - 1) & 1) * FIT_NB * EGO_NS, sS);
    __syncthreads();
    if (tid == 0) {
      if (a.k == 1) {
        for (int i = 0; i < EGO_STATE; ++i) sSt[i] = 0.0;
        sSt[6] = 1.0; sSt[7] = 1.0;  // identity, alive
      } else {
        const double* prev = a.state + ((a.k - 1) & 1) * EGO_STATE;
        for (int i = 0; i < EGO_STATE; ++i) sSt[i] = prev[i];
      }
      ego_step(sS, sSt, a.min_valid, sA, sB);
      if (blockIdx.x == 0) {
        double* cur = a.state + (a.k & 1) * EGO_STATE;
        for (int i = 0; i < EGO_STATE; ++i) cur[i] = sSt[i];
      }
    }
    __syncthreads();
  } else if (tid == 0 && blockIdx.x == 0) {
    *a.ticket = 0u;  // (the mask pass is a later launch)
  }
  SE3T G{V3{0.f, 0.f, 0.f}, Q4{0.f, 0.f, 0.f, 1.f}};
  bool alive = true;
  if (PASS != 0) {
    G = SE3T{V3{(float)sSt[0], (float)sSt[1], (float)sSt[2]}, Q4{(float)sSt[3], (float)sSt[4], (float)sSt[5], (float)sSt[6]}};
    alive = sSt[7] != 0.0;
  }

  double acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = 0.0;
  const long long n = (long long)a.h * a.w;
  const float d2 = a.delta * a.delta;
  // (a stopped fit needs no further sums; pass 0 and the mask pass always run)
  if (PASS != 1 || alive) {
    for (long long e = (long long)blockIdx.x * 256 + tid; e < n; e += (long long)FIT_NB * 256) {
      const int y = (int)(e / a.w), x = (int)(e - (long long)y * a.w);
      const size_t p = (size_t)y * a.W + x;
      const V3 X0 = inv_project(a.depth[p], x, y, a.fx, a.fy, a.cx, a.cy);
      V3 X1;
      if (PASS == 0) {
        X1 = se3_act(se3_load(a.T + p * 7), X0);
        float* o = a.x1 + (size_t)e * 3;
        o[0] = X1.x; o[1] = X1.y; o[2] = X1.z;
      } else {
        const float* o = a.x1 + (size_t)e * 3;
        X1 = V3{o[0], o[1], o[2]};
      }
      const bool valid = X0.z >= MIN_DEPTH && X1.z >= MIN_DEPTH && ego_finite3(X0) && ego_finite3(X1);
      const V3 Y = PASS == 0 ? X0 : se3_act(G, X0);
      const V3 r = V3{Y.x - X1.x, Y.y - X1.y, Y.z - X1.z};
      const float iz = 1.f / X0.z, w0 = iz * iz;
      const float e2 = dot3(r, r) * w0;
      if (PASS == 2) {
        float res = NAN;
        unsigned char mv = 255;
        if (valid) {
          const V3 pa = project(X1, a.fx, a.fy, a.cx, a.cy), pc = project(Y, a.fx, a.fy, a.cx, a.cy);
          const float fu = pa.x - pc.x, fv = pa.y - pc.y;
          res = sqrtf(fu * fu + fv * fv);
          mv = res > a.tau ? 1 : 0;
          acc[0] += 1.0;
          if (e2 <= d2) { acc[1] += 1.0; acc[2] += (double)e2; }
        }
        a.moving[e] = mv;
        if (a.residual) a.residual[e] = res;
      } else if (valid) {
        const float wt = PASS == 0 ? w0 : w0 / (1.f + e2 / d2);
        const V3 wY = scale3(wt, Y), wr = scale3(wt, r), wc = scale3(wt, cross3(Y, r));
        acc[0] += (double)wt;
        acc[1] += (double)wY.x; acc[2] += (double)wY.y; acc[3] += (double)wY.z;
        acc[4] += (double)(wY.x * Y.x); acc[5] += (double)(wY.x * Y.y); acc[6] += (double)(wY.x * Y.z);
        acc[7] += (double)(wY.y * Y.y); acc[8] += (double)(wY.y * Y.z); acc[9] += (double)(wY.z * Y.z);
        acc[10] += (double)wr.x; acc[11] += (double)wr.y; acc[12] += (double)wr.z;
        acc[13] += (double)wc.x; acc[14] += (double)wc.y; acc[15] += (double)wc.z;
        acc[16] += 1.0;
      }
    }
  }
  fit_reduce_store<NACC>(acc, sRed, a.partial + ((size_t)(a.k & 1) * FIT_NB + blockIdx.x) * EGO_NS);
  if (PASS != 2) return;

  // ---- the record: the workgroup that draws the last ticket adds the mask pass's rows
  if (!fit_last_workgroup(a.ticket)) return;
  fit_sum_rows<EGO_NS, 3>(a.partial + (size_t)(a.k & 1) * FIT_NB * EGO_NS, sS);
  __syncthreads();
  if (tid == 0) {
    float* rec = a.record;
    rec[0] = a.scale * (float)sSt[0]; rec[1] = a.scale * (float)sSt[1]; rec[2] = a.scale * (float)sSt[2];
    for (int i = 3; i < 7; ++i) rec[i] = (float)sSt[i];
    rec[7] = sSt[7] != 0.0 ? 1.f : 0.f;
    rec[8] = (float)sS[0];
    rec[9] = (float)sS[1];
    rec[10] = sS[1] > 0.0 ? (float)sqrt(sS[2] / sS[1]) * a.fx : 0.f;
    rec[11] = (float)sSt[8];
    for (int i = 12; i < 16; ++i) rec[i] = 0.f;
  }
}

extern "C" long long codd_ego_motion_scratch(int h, int w) {
  if (h <= 0 || w <= 0) return -1;
  return fit_scratch_bytes(EGO_NS, EGO_STATE) + 12LL * h * w;  // X1
}

extern "C" int codd_ego_motion(const float* T, const float* depth_prev, int H, int W, int h, int w, float fx, float fy,
                               float cx, float cy, float scale, int iters, float delta_px, float tau_px, int min_valid,
                               void* scratch, long long scratch_bytes, float* record, unsigned char* moving,
                               float* residual, void* stream) {
  if (!T || !depth_prev || !scratch || !record || !moving) return CODD_EINVAL;
  if (H <= 0 || W <= 0 || h <= 0 || w <= 0 || h > H || w > W) return CODD_EINVAL;
  if (iters < 1 || iters > 32) return CODD_EINVAL;
  if (!(fx > 0.f) || !(fy > 0.f) || !(delta_px > 0.f) || !(tau_px > 0.f)) return CODD_EINVAL;
  if (scratch_bytes < codd_ego_motion_scratch(h, w)) return CODD_EINVAL;
  const FitScratch f = fit_carve(scratch, EGO_NS, EGO_STATE);
  EgoArgs a;
  a.T = T; a.depth = depth_prev;
  a.partial = f.partial; a.state = f.state; a.ticket = f.ticket;
  a.x1 = (float*)f.rest;
  a.record = record; a.moving = moving; a.residual = residual;
  a.W = W; a.h = h; a.w = w; a.iters = iters; a.min_valid = min_valid;
  a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.scale = scale; a.delta = delta_px / fx; a.tau = tau_px;
  hipStream_t s = (hipStream_t)stream;
  for (int k = 0; k <= iters; ++k) {
    a.k = k;
    if (k == 0) ego_pass_kernel<0><<<FIT_NB, 256, 0, s>>>(a);
    else if (k < iters) ego_pass_kernel<1><<<FIT_NB, 256, 0, s>>>(a);
    else ego_pass_kernel<2><<<FIT_NB, 256, 0, s>>>(a);
    CODD_LAUNCH_CHECK();
  }
  return CODD_OK;
}
