// codd_export_confidence: which pixels of a live session's depth map to trust (codd_amd/live.py, confidence=).
// The reference has no such output (its evaluation masks come from ground truth): per crop pixel the flags
// OUT_OF_VIEW / OCCLUDED / MISMATCH / INVALID and a photometric residual, from the frame's fused disparity and the two
// normalised images the frame graph read.  The contract, fixed to the fp32 operation, is in include/codd_hip.h.
//
// A workgroup owns one row: the row's right-view z-buffer (the largest disparity that lands on each right column) must
// be complete before any pixel of the row is tested against it.  Three passes over the row, a barrier between them:
//   clear   zbuf[0, w) = 0 (the bits of +0.0f: below every valid disparity);
//   splat   every valid in-view pixel offers the bits of d to zbuf[f] and zbuf[f + 1] with an integer LDS atomic max:
//           positive floats order like their bit patterns and a maximum does not depend on arrival order, so equal
//           inputs give equal bits; the lane also parks d in LDS for the test pass;
//   test    occlusion against zbuf[r], the residual from two taps of the right row, the flag byte.
// Largest row: 8 bytes of LDS per pixel (z-buffer word + parked disparity) within the 64 KiB a workgroup may use
// without opting in to more: CODD_CONF_MAX_W = 8192.
//
// Lane-to-pixel mapping: lane t of pass k takes row element i = 256 k + t, which is pixel x = i - s, where s is the
// byte phase of the row's first flag inside its 32-bit word (s = (flags + y * w) & 3; rows of w bytes start at any
// phase).  So consecutive lanes read consecutive dwords of the disparity row and of the six image rows and write
// consecutive dwords of the residual row (one dword per lane, a wave covers 256 contiguous bytes per plane), and the four
// lanes 4j .. 4j+3 hold the four flag bytes of one ALIGNED 32-bit word: lane 4j collects them with three wave shuffles
// and stores the word.  Quads that hang over either end of the row store their (at most 3 + 3) bytes one by one.  The
// LDS traffic is one dword per lane at consecutive addresses (conflict-free) except the atomics and the z-buffer read,
// whose addresses are x - d: neighbouring lanes differ by about one column wherever the disparity is smooth.
#include "common.h"

#define CONF_THREADS 256

__device__ __forceinline__ float conf_residual(const float* __restrict__ lrow, const float* __restrict__ rrow, size_t N,
                                               int x, int f, int x1, float a, float s0, float s1, float s2) {
#pragma clang fp contract(off)  // every operation of the contract rounds once: no fused multiply-add
  const float b = 1.f - a;
  const float e0 = fabsf(lrow[x] - (rrow[f] * b + rrow[x1] * a)) * s0;
  const float e1 = fabsf(lrow[N + x] - (rrow[N + f] * b + rrow[N + x1] * a)) * s1;
  const float e2 = fabsf(lrow[2 * N + x] - (rrow[2 * N + f] * b + rrow[2 * N + x1] * a)) * s2;
  return ((e0 + e1) + e2) * (1.f / 3.f);
}

__global__ __launch_bounds__(CONF_THREADS) void export_confidence_kernel(
    const float* __restrict__ disp, const float* __restrict__ left, const float* __restrict__ right, size_t N, int W, int w,
    float s0, float s1, float s2, float occ_px, float tau, unsigned char* __restrict__ flags, float* __restrict__ residual) {
  extern __shared__ unsigned conf_lds[];
  unsigned* zbuf = conf_lds;               // [w]
  float* sd = (float*)(conf_lds + w);      // [w]
  const int y = blockIdx.x, t = threadIdx.x;
  const float* __restrict__ drow = disp + (size_t)y * W;
  unsigned char* __restrict__ frow = flags + (size_t)y * w;
  const int s = (int)((uintptr_t)frow & 3), n = w + s;

  for (int x = t; x < w; x += CONF_THREADS) zbuf[x] = 0u;
  __syncthreads();
  for (int i = t; i < n; i += CONF_THREADS) {
    const int x = i - s;
    if (x < 0) continue;
    const float d = drow[x];
    sd[x] = d;
    if (!(d > 0.f && d < INFINITY)) continue;  // (NaN compares false)
    const float u = (float)x - d;
    if (u < 0.f) continue;
    const int f = (int)floorf(u);  // 0 <= f <= x < w
    atomicMax(&zbuf[f], __float_as_uint(d));
    if (f + 1 < w) atomicMax(&zbuf[f + 1], __float_as_uint(d));
  }
  __syncthreads();
  for (int i0 = 0; i0 < n; i0 += CONF_THREADS) {  // (uniform trip count: every lane takes part in the shuffles)
    const int i = i0 + t, x = i - s;
    const bool in = x >= 0 && x < w;
    unsigned fl = 0u;
    float res = NAN;
    if (in) {
      const float d = sd[x];
      if (!(d > 0.f && d < INFINITY)) {
        fl = CODD_CONF_INVALID;
      } else {
        const float u = (float)x - d;
        if (u < 0.f) {
          fl = CODD_CONF_OUT_OF_VIEW;
        } else {
          const int f = (int)floorf(u), r = (int)floorf(u + 0.5f);  // r is f or f + 1 and <= x
          if (__uint_as_float(zbuf[r]) > d + occ_px) fl = CODD_CONF_OCCLUDED;
          if (left) {
            res = conf_residual(left + (size_t)y * W, right + (size_t)y * W, N, x, f, min(f + 1, w - 1), u - (float)f,
                                s0, s1, s2);
            if (res > tau) fl |= CODD_CONF_MISMATCH;
          }
        }
      }
      if (residual) residual[(size_t)y * w + x] = res;
    }
    // the four flag bytes of lanes 4j .. 4j+3 are one aligned 32-bit word of the output
    const unsigned word = fl | (__shfl_down(fl, 1) << 8) | (__shfl_down(fl, 2) << 16) | (__shfl_down(fl, 3) << 24);
    const int x0 = (i & ~3) - s;  // first pixel of this lane's quad
    if (x0 >= 0 && x0 + 3 < w) {
      if ((i & 3) == 0) *(unsigned*)(frow + x0) = word;
    } else if (in) {
      frow[x] = (unsigned char)fl;
    }
  }
}

extern "C" int codd_export_confidence(const float* disp, const float* left, const float* right, int H, int W, int h, int w,
                                      const float* stdv, float occ_px, float tau, unsigned char* flags, float* residual,
                                      void* stream) {
  if (!disp || !flags) return CODD_EINVAL;
  if ((left == nullptr) != (right == nullptr) || (left && !stdv) || (residual && !left)) return CODD_EINVAL;
  if (H <= 0 || W <= 0 || h <= 0 || w <= 0 || h > H || w > W) return CODD_EINVAL;
  if (!(occ_px >= 0.f) || tau != tau) return CODD_EINVAL;  // (a NaN occ_px compares false)
  if (w > CODD_CONF_MAX_W) return CODD_EUNSUPPORTED;
  const float s0 = left ? stdv[0] : 0.f, s1 = left ? stdv[1] : 0.f, s2 = left ? stdv[2] : 0.f;
  export_confidence_kernel<<<h, CONF_THREADS, (size_t)w * 8, (hipStream_t)stream>>>(
      disp, left, right, (size_t)H * W, W, w, s0, s1, s2, occ_px, tau, flags, residual);
  CODD_LAUNCH_CHECK();
  return CODD_OK;
}
