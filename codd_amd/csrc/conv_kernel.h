#pragma once
// Kernel template of the convolution family; instantiated in conv_inst_*.hip (one translation unit per
// group so that the instantiations compile in parallel) and launched from conv.hip.
#include "common.h"
#include <stdint.h>
#include <string.h>

// Convolution family: implicit GEMM on v_mfma_f32_16x16x4_f32 (exact fp32, k-ordered fma chain).
//
// GEMM view:  D[pixel, co] = sum_k X[pixel, k] * W[k, co],  k = (tap, ci).
//   MFMA A operand (16 x 4)  = im2col    : lane l holds X[pixel = l&15][ci = c4 + (l>>4)]
//   MFMA B operand (4 x 16)  = weights   : lane l holds W[ci = c4 + (l>>4)][co = l&15]
//   MFMA D (16 x 16)         : lane l holds D[pixel = 4*(l>>4) + r][co = l&15], r = 0..3
// (the A and B lane layouts are mirror images -- row or column l&15, k = l>>4 -- so the LDS images and reads are those
// of the weights-as-A order; only the accumulator is its transpose, the layout of conv_bf16_kernel.h).  A lane holds
// FOUR CONSECUTIVE output pixels of ONE channel: the operands and the output of the epilogue are one 16-byte access per
// block in NCHW where Wout % 4 == 0, and the four lanes l>>4 of a channel cover 64 contiguous bytes.
//
// Workgroup = NW waves (4 by default).  Output tile = TH x TW pixels, every wave owns NPB 16-pixel blocks and
// all MB 16-channel blocks of the workgroup's channel group.  The input halo tile of CK
// channels and the matching weight chunk are staged in LDS per chunk; channel stride of the
// LDS image is padded to 16 (mod 32) floats so that the two ci-groups of a 32-lane half hit
// disjoint banks.

struct ConvK {
  codd_conv_params p;
  int cin, nchunks, ntaps;
  int th, tw, thi, twi, chs;
  int wrow, wchunk;
  int tiles_x, tiles_y, ncog;
  int cout_eff;
  int twp;     // LDS row stride (floats, multiple of 4) of the input tile
  int xoff;    // column of the tile's first input pixel inside the 4-aligned LDS row
  int twp4;    // float4 units per LDS row
  int upc;     // float4 units per channel = thi * twp4
  int nunits;  // ck * upc
  int vec_ok;  // 16-byte global loads allowed (Win % 4 == 0 and 16-byte aligned bases)
  int evec;    // 16-byte epilogue accesses allowed (store_mode 0, Wout % 4 == 0, out and every present operand 16-byte aligned)
  int xcd;     // 1: workgroup b (which the dispatcher places on XCD b % 8) takes work item conv_xcd_item(b): every XCD
               // walks ONE contiguous range of tiles, so the halo rows neighbouring tiles share are re-read from that
               // XCD's own L2 instead of being fetched by up to 8 L2s
};

// work item of workgroup ``bid`` under the XCD-contiguous mapping: XCD x = bid % 8 owns items [start_x, start_x + n_x)
__device__ __forceinline__ int conv_xcd_item(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, x = bid & 7, idx = bid >> 3;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + idx;
}

__device__ __forceinline__ const float* view_ptr(const codd_view& v, int b, int c, int hw) {
  return v.ptr + ((size_t)b * v.ctot + v.coff + c) * (size_t)hw;
}

// Activation of N accumulator blocks (4 pixels of channel co[i] each) and the optional post operand.  p.act is uniform
// over the launch: the switch is taken once per batch and every arm is a straight-line loop over the batch (act_apply
// with a constant selector folds to its one expression, so every value keeps the bits of act_apply(v, act, co)).
// The post operand is ADDED to the activation's rounded result, never fused with a product inside it (mish is
// v * tanh(softplus v), leaky ReLU 0.2 v): the value-at-a-time epilogue added it to the result of the switch, and the
// recorded bits (tests/golden/conv_epilogue_bits.json, mish + post) are those of the separate multiply and add.
template <int N>
__device__ __forceinline__ void conv_epi_act(float (&v)[N][4], const float (&po)[N][4], bool post, int act,
                                             const int (&co)[N]) {
#pragma clang fp contract(off)
#define CONV_EPI_ARM(ACT)                                                 \
  case ACT:                                                               \
    _Pragma("unroll") for (int i = 0; i < N; ++i)                         \
    _Pragma("unroll") for (int r = 0; r < 4; ++r) {                       \
      float t = act_apply(v[i][r], ACT, co[i]);                           \
      if (post) t += po[i][r];                                            \
      v[i][r] = t;                                                        \
    }                                                                     \
    break;
  switch (act) {
    CONV_EPI_ARM(CODD_ACT_LRELU02)
    CONV_EPI_ARM(CODD_ACT_RELU)
    CONV_EPI_ARM(CODD_ACT_SIGMOID)
    CONV_EPI_ARM(CODD_ACT_TANH)
    CONV_EPI_ARM(CODD_ACT_MISH)
    CONV_EPI_ARM(CODD_ACT_RELU_CH0)
    default:
#pragma unroll
      for (int i = 0; i < N; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (post) v[i][r] += po[i][r];
  }
#undef CONV_EPI_ARM
}

// the same without a post operand, for N blocks of ONE channel (the transposed-convolution store)
template <int N>
__device__ __forceinline__ void conv_epi_act(float (&v)[N][4], int act, int co) {
  float none[N][4];
  int cos[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    cos[i] = co;
#pragma unroll
    for (int r = 0; r < 4; ++r) none[i][r] = 0.f;
  }
  conv_epi_act<N>(v, none, false, act, cos);
}

// Epilogue shared by conv_mfma_kernel and conv_quad_body: bias, res1, res2, activation, post, store -- in phases.  A
// value-at-a-time loop (load bias, load res1, ..., store, next value) costs one memory round trip per LOAD: the operand
// and output pointers are kernel arguments, so a store may alias the next load and the compiler keeps program order and
// drains vmcnt (which on gfx9 also counts the previous store) before every use.  Here a batch of accumulator blocks
//   (a) gets its predicates and pixel offsets,
//   (b) issues every bias / res1 / res2 / post load into registers -- before any store of the batch,
//   (c) waits once (at the first use),
//   (d) applies ((acc + bias) + res1) + res2 -> act_apply -> + post per value: the order of the value-at-a-time loop, so
//       every output element keeps its bits,
//   (e) stores.
// An accumulator block (a, m) of a lane is FOUR CONSECUTIVE PIXELS ox .. ox + 3 of row oy[a] in ONE channel
// co = (cog * MB + m) * 16 + j (layout at the top of this file): one channel predicate, one bias scalar, one constant
// channel for the activation per block.
//   k.evec (host: store_mode 0, Wout % 4 == 0, out and every present operand 16-byte aligned): ox is a multiple of 4 and
//     tiles are multiples of 16 wide, so a lane's quad is 16-byte aligned and entirely inside or outside the row -- res1,
//     res2 and post are one 16-byte load each and the block is one 16-byte store.
//   otherwise (30- and 15-wide maps, operands off a 16-byte boundary): the same registers filled by 4-byte accesses under
//     a per-pixel predicate.
// A load is issued only where co < cout_eff, oy < Hout, ox + r < Wout and the operand is present; no other address is
// formed.  Aliasing contract (include/codd_hip.h, codd_conv_params): an operand may be the output tensor itself element
// for element -- the lane that writes out[c][pixel] is the only one that reads operand[c][pixel], and it reads before
// it writes.
// A batch is BLK of the lane's NPB * MB accumulator blocks (block q = m * NPB + a: the pixel blocks of one channel block
// are neighbours, so its channel base addresses die early).  A block needs 13 operand registers (1 bias + 3 x 4): the
// whole lane (up to 4 blocks = 52) where the K loop's staging registers (DEAD of them, dead by now) cover those 52,
// 2 blocks (26) under the staging classes of 32 and 48 -- so that no instantiation needs more registers than its K loop
// (same occupancy, no scratch: profiles/conv_fp32_vec_epilogue_resources.txt).
template <int NPB, int MB, int DEAD>
__device__ __forceinline__ void conv_epilogue(const ConvK& k, const f32x4 (&acc)[NPB][MB], int b, int cog, int ty, int tx) {
  const codd_conv_params& p = k.p;
  // the lane's coordinates, formed from a thread index that is opaque to the optimiser: every predicate and address below
  // is formed HERE, behind the K loop, instead of being hoisted in front of it and kept in registers across it (the
  // compile-time table profiles/conv_fp32_vec_epilogue_resources.txt: eight instantiations need fewer registers than their
  // parent for it and none more waves' worth; its effect on time is not measured on its own)
  int t_ = threadIdx.x;
  asm volatile("" : "+v"(t_));
  const int wave = t_ >> 6, g = (t_ & 63) >> 4, j = t_ & 15;
  constexpr int XB = NPB >= 2 ? 2 : 1;
  constexpr int RPW = NPB / XB;
  constexpr int NBLK = NPB * MB;
  constexpr int BLK = NBLK <= 2 ? NBLK : (DEAD >= 52 ? 4 : 2);  // blocks per batch
  static_assert(NBLK % BLK == 0, "batch");
  const int hwout = p.Hout * p.Wout;
#ifdef CONV_NO_EPILOGUE
  {  // dev ablation: one store per lane keeps the accumulators alive
    float s_ = 0.f;
#pragma unroll
    for (int a = 0; a < NPB; ++a)
#pragma unroll
      for (int m = 0; m < MB; ++m) s_ += acc[a][m][0] + acc[a][m][1] + acc[a][m][2] + acc[a][m][3];
    const int oy = ty * k.th + wave * RPW, ox = tx * k.tw + 4 * g;
    const int co = cog * MB * 16 + j;
    if (oy < p.Hout && ox < p.Wout && co < k.cout_eff && p.store_mode == 0)
      p.out[((size_t)b * p.out_ctot + p.out_coff + co) * (size_t)hwout + oy * p.Wout + ox] = s_;
    return;
  }
#endif
  bool cok[MB];      // channel predicate of a block
  unsigned pm[NPB];  // pixel predicates of a block: bit r = pixel ox + r is inside the map
  int oy[NPB], ox[NPB];
#pragma unroll
  for (int m = 0; m < MB; ++m) cok[m] = (cog * MB + m) * 16 + j < k.cout_eff;
#pragma unroll
  for (int a = 0; a < NPB; ++a) {
    oy[a] = ty * k.th + wave * RPW + a / XB;
    ox[a] = tx * k.tw + (a % XB) * 16 + 4 * g;
    pm[a] = 0;
    if (oy[a] < p.Hout) {
#pragma unroll
      for (int r = 0; r < 4; ++r) pm[a] |= (ox[a] + r < p.Wout) ? (1u << r) : 0u;
    }
  }
  if (p.store_mode == 0) {
    int pix[NPB];
#pragma unroll
    for (int a = 0; a < NPB; ++a) pix[a] = oy[a] * p.Wout + ox[a];
#pragma unroll
    for (int q0 = 0; q0 < NBLK; q0 += BLK) {
      float bv[BLK], r1[BLK][4], r2[BLK][4], po[BLK][4];
      int co[BLK];
      bool ok[BLK];
#pragma unroll
      for (int i = 0; i < BLK; ++i) {
        const int a = (q0 + i) % NPB, m = (q0 + i) / NPB;
        co[i] = (cog * MB + m) * 16 + j;
        ok[i] = cok[m] && pm[a] != 0;
        bv[i] = 0.f;
        if (p.bias && ok[i]) bv[i] = p.bias[co[i]];
      }
#define CONV_EPI_LOAD(DST, VIEW, VEC)                                                    \
  _Pragma("unroll") for (int i = 0; i < BLK; ++i) {                                      \
    const int a = (q0 + i) % NPB;                                                        \
    _Pragma("unroll") for (int r = 0; r < 4; ++r) DST[i][r] = 0.f;                       \
    if (VIEW.ptr && ok[i]) {                                                             \
      const float* s_ = view_ptr(VIEW, b, co[i], hwout) + pix[a];                        \
      if (VEC) {                                                                         \
        const f32x4 q_ = *(const f32x4*)s_;                                              \
        DST[i][0] = q_[0]; DST[i][1] = q_[1]; DST[i][2] = q_[2]; DST[i][3] = q_[3];      \
      } else {                                                                           \
        _Pragma("unroll") for (int r = 0; r < 4; ++r)                                    \
          if (pm[a] & (1u << r)) DST[i][r] = s_[r];                                      \
      }                                                                                  \
    }                                                                                    \
  }
      if (k.evec) {
        CONV_EPI_LOAD(r1, p.res1, true)
        CONV_EPI_LOAD(r2, p.res2, true)
        CONV_EPI_LOAD(po, p.post, true)
      } else {
        CONV_EPI_LOAD(r1, p.res1, false)
        CONV_EPI_LOAD(r2, p.res2, false)
        CONV_EPI_LOAD(po, p.post, false)
      }
#undef CONV_EPI_LOAD
      float v[BLK][4];
#pragma unroll
      for (int i = 0; i < BLK; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int a = (q0 + i) % NPB, m = (q0 + i) / NPB;
          float t = acc[a][m][r];
          if (p.bias) t += bv[i];
          if (p.res1.ptr) t += r1[i][r];
          if (p.res2.ptr) t += r2[i][r];
          v[i][r] = t;
        }
      conv_epi_act<BLK>(v, po, p.post.ptr != nullptr, p.act, co);
#pragma unroll
      for (int i = 0; i < BLK; ++i) {
        const int a = (q0 + i) % NPB;
        if (!ok[i]) continue;
        float* d_ = p.out + ((size_t)b * p.out_ctot + p.out_coff + co[i]) * (size_t)hwout + pix[a];
        if (k.evec) {
          *(f32x4*)d_ = (f32x4){v[i][0], v[i][1], v[i][2], v[i][3]};  // (a native vector: one 16-byte store in the IR)
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (pm[a] & (1u << r)) d_[r] = v[i][r];
        }
      }
    }
  } else {  // ConvTranspose2d k=2 s=2: co = (a2*2+b2)*Cout + c; bias only.  One batch per channel block; the output
            // pixels of a lane are 2 apart, so the stores stay 4-byte.
    const int W2 = 2 * p.Wout;
    bool anyp = false;
#pragma unroll
    for (int a = 0; a < NPB; ++a) anyp |= pm[a] != 0;
#pragma unroll
    for (int m = 0; m < MB; ++m) {
      const int co = (cog * MB + m) * 16 + j;
      const int cq = co / p.Cout, cc = co - cq * p.Cout;
      float bv = 0.f;
      if (p.bias && anyp && cok[m]) bv = p.bias[cc];
      float v[NPB][4];
#pragma unroll
      for (int a = 0; a < NPB; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float t = acc[a][m][r];
          if (p.bias) t += bv;
          v[a][r] = t;
        }
      conv_epi_act<NPB>(v, p.act, cc);
      if (!cok[m]) continue;
      float* d_ = p.out + ((size_t)b * p.out_ctot + p.out_coff + cc) * (size_t)(4 * hwout) + (size_t)(cq >> 1) * W2 + (cq & 1);
#pragma unroll
      for (int a = 0; a < NPB; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (pm[a] & (1u << r)) d_[(size_t)(2 * oy[a]) * W2 + 2 * (ox[a] + r)] = v[a][r];
    }
  }
}

// Staging: a chunk (CK input channels of the halo tile + the matching packed weights) is fetched
// with 16-byte global loads into REGISTERS right before the MFMA phase of the previous chunk and
// written to LDS after it (issue early / write late), so that HBM/L2 latency overlaps the matrix
// pipe.  The (channel, row, float4-column) decomposition of a thread's units does not depend on
// the chunk and is computed once.
// Workgroups per CU the register allocator is held to (0: none).  <4,2,2,4,8> needs 126 VGPRs for its K loop and two more
// as spill lanes of scalar registers: without the bound the allocator takes 128 + 2 and the kernel drops from 4 to 3 waves
// per SIMD.  This depends on the register allocator of the compiler in use: under a bound it cannot meet, a compiler spills
// to scratch instead of failing.  When the compiler changes, regenerate profiles/conv_fp32_vec_epilogue_resources.txt (its
// header has the command) and check this kernel's scratch and VGPR-spill columns; tests/test_conv_resources_table.py holds
// the committed table to "no scratch, no VGPR spill, no occupancy below the parent's".
constexpr int conv_min_blocks(int nw, int npb, int mb, int wreg, int ireg) {
  return (nw == 4 && npb == 2 && mb == 2 && wreg == 4 && ireg == 8) ? 4 : 0;
}

template <int NW, int NPB, int MB, int WREG, int IREG>
__global__ __launch_bounds__(NW * 64, conv_min_blocks(NW, NPB, MB, WREG, IREG)) void conv_mfma_kernel(const ConvK k) {
  constexpr int NT = NW * 64;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* wl = smem;
  float* il = smem + k.wchunk;
  const codd_conv_params& p = k.p;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, j = lane & 15;
  constexpr int XB = NPB >= 2 ? 2 : 1;  // 16-pixel blocks along x in the tile
  constexpr int RPW = NPB / XB;         // tile rows per wave

  int bid = k.xcd ? conv_xcd_item(blockIdx.x, gridDim.x) : blockIdx.x;
  const int tx = bid % k.tiles_x; bid /= k.tiles_x;
  const int ty = bid % k.tiles_y; bid /= k.tiles_y;
  const int cog = bid % k.ncog;
  const int b = bid / k.ncog;

  const int hwin = p.Hin * p.Win;
  const int gy0 = ty * k.th * p.sy - p.pad_t;
  const int gxs = tx * k.tw * p.sx - p.pad_l - k.xoff;  // 4-aligned start column (may be negative)

  // ---- per-thread staging metadata ---------------------------------------------------------------
  int u_lds[IREG], u_g[IREG], u_c[IREG];
  unsigned u_m[IREG];
#pragma unroll
  for (int r = 0; r < IREG; ++r) {
    const int u = tid + r * NT;
    u_c[r] = -1; u_m[r] = 0; u_lds[r] = 0; u_g[r] = 0;
    if (u < k.nunits) {
      const int c = u / k.upc, rem = u - c * k.upc;
      const int y = rem / k.twp4, x4 = rem - y * k.twp4;
      const int gy = gy0 + y, gx = gxs + 4 * x4;
      unsigned m = 0;
      if ((unsigned)gy < (unsigned)p.Hin) {
#pragma unroll
        for (int q = 0; q < 4; ++q) m |= ((unsigned)(gx + q) < (unsigned)p.Win) ? (1u << q) : 0u;
      }
      u_c[r] = c; u_m[r] = m;
      u_lds[r] = c * k.chs + y * k.twp + 4 * x4;
      u_g[r] = gy * p.Win + gx;
    }
  }
  const int wchunk4 = k.wchunk >> 2;
  float4 wreg[WREG], ireg[IREG];

#define CONV_ISSUE(CH)                                                                                    \
  {                                                                                                       \
    const float4* src_ = (const float4*)(p.wpacked + ((size_t)(cog * k.nchunks + (CH))) * k.wchunk);      \
    _Pragma("unroll") for (int r = 0; r < WREG; ++r) {                                                    \
      const int e = tid + r * NT;                                                                         \
      wreg[r] = e < wchunk4 ? src_[e] : make_float4(0.f, 0.f, 0.f, 0.f);                                  \
    }                                                                                                     \
    const int c0_ = (CH) * p.ck;                                                                          \
    _Pragma("unroll") for (int r = 0; r < IREG; ++r) {                                                    \
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);                                                         \
      const int cg = c0_ + u_c[r];                                                                        \
      if (u_c[r] >= 0 && cg < k.cin && u_m[r]) {                                                          \
        const float* s_ =                                                                                 \
            (cg < p.C0 ? view_ptr(p.in0, b, cg, hwin) : view_ptr(p.in1, b, cg - p.C0, hwin)) + u_g[r];    \
        if (u_m[r] == 0xFu && k.vec_ok) {                                                                 \
          v = *(const float4*)s_;                                                                         \
        } else {                                                                                          \
          if (u_m[r] & 1u) v.x = s_[0];                                                                   \
          if (u_m[r] & 2u) v.y = s_[1];                                                                   \
          if (u_m[r] & 4u) v.z = s_[2];                                                                   \
          if (u_m[r] & 8u) v.w = s_[3];                                                                   \
        }                                                                                                 \
      }                                                                                                   \
      ireg[r] = v;                                                                                        \
    }                                                                                                     \
  }
#define CONV_COMMIT()                                                                                     \
  {                                                                                                       \
    float4* dst_ = (float4*)wl;                                                                           \
    _Pragma("unroll") for (int r = 0; r < WREG; ++r) {                                                    \
      const int e = tid + r * NT;                                                                         \
      if (e < wchunk4) dst_[e] = wreg[r];                                                                 \
    }                                                                                                     \
    _Pragma("unroll") for (int r = 0; r < IREG; ++r) if (u_c[r] >= 0) *(float4*)(il + u_lds[r]) = ireg[r]; \
  }

  f32x4 acc[NPB][MB];
#pragma unroll
  for (int a = 0; a < NPB; ++a)
#pragma unroll
    for (int m = 0; m < MB; ++m) acc[a][m] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // per pixel-block LDS base offset (row / col part that does not depend on the tap)
  int pbase[NPB];
#pragma unroll
  for (int a = 0; a < NPB; ++a) {
    const int prow = wave * RPW + a / XB, pcol = (a % XB) * 16 + j;
    pbase[a] = prow * p.sy * k.twp + pcol * p.sx + k.xoff;
  }

  CONV_ISSUE(0);
  for (int ch = 0; ch < k.nchunks; ++ch) {
    __syncthreads();  // every wave is done reading the previous chunk
    CONV_COMMIT();
    __syncthreads();
    if (ch + 1 < k.nchunks) CONV_ISSUE(ch + 1);
    for (int ky = 0; ky < p.kh; ++ky) {
      for (int kx = 0; kx < p.kw; ++kx) {
        const float* wp = wl + (ky * p.kw + kx) * p.ck * k.wrow + j + g * k.wrow;
        const float* ip = il + ky * p.dil_y * k.twp + kx * p.dil_x + g * k.chs;
        const int wstep = 4 * k.wrow, istep = 4 * k.chs;
        // 4 k-steps per trip: the 4*(MB+NPB) LDS reads are issued ahead of the 4*MB*NPB MFMAs
#pragma unroll 4
        for (int c4 = 0; c4 < p.ck; c4 += 4) {
          float av[MB], bv[NPB];
#pragma unroll
          for (int m = 0; m < MB; ++m) av[m] = wp[m * 16];
#pragma unroll
          for (int a = 0; a < NPB; ++a) bv[a] = ip[pbase[a]];
          wp += wstep;
          ip += istep;
#pragma unroll
          for (int a = 0; a < NPB; ++a)
#pragma unroll
            for (int m = 0; m < MB; ++m)
              acc[a][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(bv[a], av[m], acc[a][m], 0, 0, 0);
        }
      }
    }
  }

  conv_epilogue<NPB, MB, 4 * WREG + 4 * IREG>(k, acc, b, cog, ty, tx);
}

// ---- instantiation lists (X(NW, NPB, MB, WREG, IREG)) -----------------------------------------------
#define CONV_REGS_NW4(X, NPB, MB) X(4, NPB, MB, 4, 4) X(4, NPB, MB, 4, 8) X(4, NPB, MB, 12, 4) X(4, NPB, MB, 12, 8) X(4, NPB, MB, 16, 8)
#define CONV_REGS_NWX(X, NW, MB) X(NW, 1, MB, 8, 4) X(NW, 1, MB, 16, 4)
#define CONV_GROUP_0(X) CONV_REGS_NW4(X, 1, 1)
#define CONV_GROUP_1(X) CONV_REGS_NW4(X, 1, 2)
#define CONV_GROUP_2(X) CONV_REGS_NW4(X, 1, 4)
#define CONV_GROUP_3(X) CONV_REGS_NW4(X, 2, 1) CONV_REGS_NW4(X, 2, 2)
#define CONV_GROUP_4(X) CONV_REGS_NW4(X, 2, 4) CONV_REGS_NW4(X, 4, 1)
#define CONV_GROUP_5(X) CONV_REGS_NW4(X, 4, 2)
#define CONV_GROUP_6(X) CONV_REGS_NW4(X, 4, 4)
#define CONV_GROUP_7(X) CONV_REGS_NWX(X, 9, 1) CONV_REGS_NWX(X, 9, 2) CONV_REGS_NWX(X, 9, 4)
#define CONV_GROUP_8(X) CONV_REGS_NWX(X, 2, 1) CONV_REGS_NWX(X, 2, 2) CONV_REGS_NWX(X, 2, 4)
#define CONV_GROUP_9(X) CONV_REGS_NWX(X, 8, 1) CONV_REGS_NWX(X, 8, 2) CONV_REGS_NWX(X, 8, 4)
#define CONV_ALL_GROUPS(X) CONV_GROUP_0(X) CONV_GROUP_1(X) CONV_GROUP_2(X) CONV_GROUP_3(X) CONV_GROUP_4(X) CONV_GROUP_5(X) CONV_GROUP_6(X) CONV_GROUP_7(X) CONV_GROUP_8(X) CONV_GROUP_9(X)
#define CONV_DECLARE(NW, NPB, MB, WREG, IREG) extern template __global__ void conv_mfma_kernel<NW, NPB, MB, WREG, IREG>(const ConvK);
#define CONV_DEFINE(NW, NPB, MB, WREG, IREG) template __global__ void conv_mfma_kernel<NW, NPB, MB, WREG, IREG>(const ConvK);
