/*
 * codd_hip.h -- C ABI of libcodd_hip.so, the MI355X (gfx950) kernel library behind CODD's
 * per-frame stereo -> motion -> fusion forward path.
 *
 * The reference (facebookresearch/CODD) has no FFI of its own: it is pure Python on torch ops
 * plus three un-vendored CUDA dependencies (lietorch / lietorch_extras, pytorch3d, mmseg).  Each
 * entry point below therefore replaces a *call site* of the reference (cited file:line, paths
 * relative to the reference root) and is what a ctypes / pybind stub in the reference's plug-in
 * classes would bind.
 *
 * Conventions
 *   - all tensors are fp32, NCHW-contiguous device memory owned by the caller (PyTorch-ROCm);
 *   - a "view" (ptr, ctot, coff) addresses channels [coff, coff+C) of a buffer that physically
 *     holds `ctot` channels per batch item -- producers write straight into concatenated
 *     buffers instead of torch.cat;
 *   - every function enqueues on `stream` (hipStream_t as void*) and returns immediately:
 *     0 on success, a negative CODD_E* code on bad arguments, a positive hipError_t otherwise;
 *   - no allocation, no host synchronisation, nothing read from the process environment: safe under hipGraph
 *     capture and callable concurrently on distinct streams.  The ONLY process-wide state is the small option table
 *     behind codd_set_option() below; every option defaults to the shipped configuration and the host library sets
 *     one only where a test asks for it.
 */
#ifndef CODD_HIP_H
#define CODD_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define CODD_ABI_VERSION 13

#define CODD_OK 0
#define CODD_EINVAL (-1)
#define CODD_EUNSUPPORTED (-2)

/* Options (ABI v12; they replace the CODD_* environment switches the library used to read -- VERDICT r5 item 7).
 *   CODD_OPT_GN_Q4       neighbours per workgroup of the Gauss-Newton builder (default 192, >= 16): the grouping of its
 *                        partial sums, i.e. another fp32 summation order of the same normal equations; the parity tests
 *                        use 256 as a re-association probe.  Changes codd_se3_gn_scratch(): set it before sizing scratch.
 *   CODD_OPT_GN_BUILDER  5 (default): the pixel's own embedding in LDS (125 VGPRs); 3: in registers (157 VGPRs) -- the
 *                        bit-identity reference of the shipped builder.
 * codd_set_option returns the previous value, or CODD_EINVAL for an unknown key / out-of-range value; not thread-safe
 * against concurrent launches (set options before launching). */
enum { CODD_OPT_GN_Q4 = 0, CODD_OPT_GN_BUILDER = 1, CODD_OPT_COUNT = 2 };
int codd_set_option(int key, int value);
int codd_get_option(int key);

/* activation codes for the conv epilogue */
enum { CODD_ACT_NONE = 0, CODD_ACT_LRELU02 = 1, CODD_ACT_RELU = 2, CODD_ACT_SIGMOID = 3,
       CODD_ACT_TANH = 4, CODD_ACT_MISH = 5, CODD_ACT_RELU_CH0 = 6 };

typedef struct {
  const float* ptr;
  int ctot; /* channels physically present per batch item */
  int coff; /* first channel of the view */
} codd_view;

/* A split-bf16 activation tensor (codd_split_bf16 layout: [b][plane hi|lo][octet][hp][wp][8 bf16], image pixel
 * (y, x) at (y + bt, x + bl), planes = 2 for terms 3 / 1 for terms 1) as the DESTINATION of a producer kernel: the
 * producer writes the image interior of channels [8*o8, ...) only; border and padding channels stay as they are
 * (zero in a persistent buffer). */
/* `terms` of a record tensor / a layout-2 convolution: the operand format of the MFMA convolution family.
 *   CODD_TERMS_BF16  (1)   one plane of bf16 records, v_mfma_f32_16x16x32_bf16
 *   CODD_TERMS_SPLIT (3)   two planes (hi | lo) of bf16 records, three MFMAs per product: the fp32-grade default
 *   CODD_TERMS_F16   (16)  one plane of IEEE fp16 records, v_mfma_f32_16x16x32_f16 (ABI v10): 11 mantissa bits instead of
 *                          bf16's 8 at the same MFMA rate -- the reference's own reduced-precision hook is fp16
 *                          (auto_fp16, model/codd.py:37,128, enabled by inference.py:120-122).  Range: |x| > 65504
 *                          saturates to +-inf as in the reference's .half() path; the host policy uses it only for
 *                          RAFT3D's feature encoder and update block (O(1) activations). */
#define CODD_TERMS_BF16 1
#define CODD_TERMS_SPLIT 3
#define CODD_TERMS_F16 16
/*   CODD_TERMS_SPLIT_F16 (48)  two planes (hi | lo) of IEEE-fp16 records, three v_mfma_f32_16x16x32_f16 per product (ABI v11):
 *                          x = hi + lo to 22 significant bits, products to ~2^-22 -- the split scheme at fp32's own grade
 *                          (bf16 split: 16 bits, 2^-17), same MFMA rate.  fp16's RANGE applies: |x| > 65504 becomes +-inf and
 *                          lo parts below 6e-8 vanish (absolute error <= 3e-8 per operand); the host keeps it to stages with
 *                          O(1)-O(1e3) activations and the parity tests watch for non-finite values. */
#define CODD_TERMS_SPLIT_F16 48
#define CODD_TERMS_OK(t) ((t) == 1 || (t) == 3 || (t) == 16 || (t) == 48)
#define CODD_TERMS_PLANES(t) (((t) == 3 || (t) == 48) ? 2 : 1)
#define CODD_TERMS_IS_F16(t) ((t) == 16 || (t) == 48)
typedef struct codd_xs_view {
  void* ptr;
  int c8, hp, wp, bt, bl, o8, terms;
} codd_xs_view;

/* ---------------------------------------------------------------------------------------------
 * Convolution family (MFMA implicit GEMM).  Three kernel families behind one entry point, selected by `layout`:
 *   0 / 1  v_mfma_f32_16x16x4_f32 (exact fp32 k-ordered fma chain);
 *   2      v_mfma_f32_16x16x32_bf16 on split-bf16 operands: terms = 3 evaluates every product as
 *          a_hi b_hi + a_hi b_lo + a_lo b_hi (fp32 accumulate, ~16 mantissa bits per product: the fp32-grade
 *          default), terms = 1 is plain bf16 operands / fp32 accumulate (reference auto_fp16 hook,
 *          model/codd.py:37,128; BASELINE.json configs[4]).
 * Replaces every nn.Conv2d / nn.ConvTranspose2d call of the hot path: HITUNet (backbone.py:8-88),
 * TileInitialization convs (initialization.py:60-156,186-190), TileUpdate* / PostTileUpdate /
 * FinalTileUpdate (propagation.py:89-333), BasicEncoder (blocks/extractor.py:119-199),
 * BasicUpdateBlock + ConvGRU (raft3d.py:44-106, blocks/gru.py:9-35), HRNet + ResizeConcatConv
 * (raft3d.py:109-160), Fusion heads (fusion.py:74-138).
 *
 *   v   = sum_{ci,ky,kx} W[co,ci,ky,kx] * in[ci, oy*sy - pad_t + ky*dil_y, ox*sx - pad_l + kx*dil_x]
 *   v  += bias[co] + res1 + res2          (each optional)
 *   v   = act(v)
 *   out = v + post                        (optional)
 * The input is the channel concatenation of in0 (C0 channels) and in1 (C1 channels, may be 0).
 * `wpacked` is the weight tensor re-laid-out by codd_conv2d_pack_weights for (mb, ck).
 * store_mode 1 = ConvTranspose2d(k=2, s=2) expressed as a 1x1 conv with 4*Cout outputs
 * (co' = (a*2+b)*Cout + co is scattered to out[co][2y+a][2x+b]).
 *
 * Aliasing contract of the epilogue operands: res1, res2 or post MAY be the output tensor itself, element for
 * element (same buffer, same ctot and coff as out / out_ctot / out_coff; the ConvGRU's gate 3 runs with out = post):
 * the lane that writes out[b][co][y][x] is the only one that reads operand[b][co][y][x], and it reads before it writes.
 * The kernels issue ALL operand loads of a batch of output elements before that batch's first store (conv_kernel.h
 * conv_epilogue), so nothing else is allowed: an operand whose elements overlap those of `out` at any OTHER offset (a shifted view, an
 * overlapping channel range under another coff, a different batch stride), or an input (in0 / in1 / xs) that overlaps `out`,
 * gives undefined results.  `bias` and `wpacked` never alias `out`.
 * Alignment: res1, res2, post and out need no alignment beyond 4 bytes; where `out` and every operand present are 16-byte
 * aligned and Wout % 4 == 0, the exact-fp32 kernels (layouts 0 and 1) take their vector path: one 16-byte access per
 * operand and per store for four consecutive pixels of a channel -- the same bits as the 4-byte path.
 * --------------------------------------------------------------------------------------------- */
typedef struct {
  codd_view in0, in1;
  int C0, C1;
  int B, Hin, Win;
  const float* wpacked;
  const float* bias; /* [Cout] or NULL */
  codd_view res1, res2, post; /* ptr == NULL when absent */
  float* out;
  int out_ctot, out_coff;
  int Cout, Hout, Wout;
  int kh, kw, sy, sx, pad_t, pad_l, dil_y, dil_x;
  int act;
  int store_mode;
  int mb;  /* 16-channel output blocks per workgroup (1, 2 or 4) */
  int npb; /* 16-pixel blocks per wave (1, 2 or 4) */
  int nw;  /* waves (= 16-pixel tile rows) per workgroup: 0 or 4 (default), or 2 / 8 / 9 (npb 1 only) */
  int ck;  /* input channels staged per LDS chunk (multiple of 4) */
  int layout; /* 0: weights packed by codd_conv2d_pack_weights; 1: quad layout (codd_conv2d_pack_weights_quad;
                 ck 16 or 32, x-stride <= 2, 16-byte aligned rows); 2: split-bf16 kernel (weights packed by
                 codd_conv2d_pack_weights_bf16 for (mb, ck, terms); here nw = tile rows, npb = 16-pixel units per
                 tile row (1 | 2), ck a multiple of 8) */
  int terms;  /* layout 2: 1 = bf16 operands, 3 = split-bf16 (hi/lo) operands, 16 = fp16 operands, 48 = split-fp16 (CODD_TERMS_*) */
  int pgw, cgw; /* layout 2: wave grid of a workgroup (pixel-unit groups x channel-block groups), mb % cgw == 0 */
  /* layout 2: the input (channel concatenation of C0 + C1 channels; in0 / in1 are not read) re-laid-out by
   * codd_split_bf16 with borders (pad_t, pad_l): [B][plane][xs_c8 octets][xs_hp][xs_wp][8] bf16 */
  const void* xs;
  int xs_c8, xs_hp, xs_wp;
  int xs_bt, xs_bl; /* borders the split tensor was made with (>= pad_t, pad_l: one split input can serve several
                       convolutions of the same activation, e.g. a 3x3 and a dilated 3x3) */
  int xs_o8;        /* first channel octet of this conv's input inside the split tensor (channel-slice views) */
  /* layout 2, optional: write the result as split-bf16 records straight into the NEXT convolution's input tensor
   * (same layout as xs, borders (xso_bt, xso_bl), first octet xso_o8, xso_terms = the consumer's terms, which must equal `terms`) instead of
   * fp32 NCHW `out` (then unused; plain convolutions only: no residual / post operand, no deconv).  The border and
   * the octets past the output channels are NOT written: the caller keeps the tensor zero there. */
  void* xso;
  int xso_c8, xso_hp, xso_wp, xso_bt, xso_bl, xso_o8, xso_terms;
  /* layout 2: 0 | 1 = every accumulator tile is owned by one consumer wave; 2 = by a PAIR of waves on the same SIMD
   * that take alternate k-steps of every chunk and add their partial sums through LDS before the epilogue (two
   * independent MFMA streams per SIMD: one wave's LDS / barrier stalls are filled by the other) */
  int ksplit;
  /* layout 2: TWO tap sets over one input tile (the ConvGRU's conv*1 + conv*2 pairs, blocks/gru.py:12-33: a 3x3 and a
   * dilated 3x3 convolution of the same tensor whose results are only ever used summed).  dil2 > 0: kh = 2 * kh0 weight
   * rows; rows [0, kh0) are the taps of a kh0 x kw convolution with dilation dil2 (both axes), rows [kh0, kh) those of
   * one with dilation (dil_y, dil_x) >= dil2; both are centred on the same pixel and (pad_t, pad_l) belongs to the
   * larger one.  One launch, one read of the input tile, one accumulator.  0: plain convolution. */
  int dil2;
  /* layout 2: ConvGRU gate epilogues on channel-quad fp32 tensors ("c4": [B][C/4][H*W][4], private to the update
   * block).  Views name c4 tensors here (ctot = their channel count, coff a multiple of 4); `act` is ignored.
   *   0  none
   *   1  out_c4[co] = acc + bias                                                      (no xso)
   *   2  Cout = 3G:  s = acc + bias + res1_c4[co]
   *        co in [0, G):   out_c4[co]     = sigmoid(s + res2_c4[co])                                 (z)
   *        co in [G, 2G):  xso[co - G]    = sigmoid(s + res2_c4[co]) * post_c4[co - G]   (records)   (r * h)
   *        co in [2G, 3G): out_c4[co - G] = s                                                        (q's input stream)
   *   3  Cout = G:   q = tanh(acc + bias + res1_c4[G + co]),  z = res1_c4[co],  h = post_c4[co]:
   *        h' = (1 - z) h + z q  ->  out_c4[co] (may be the post tensor: in place) and xso[co] (records)
   * (reference blocks/gru.py:17-34 with the gate inputs summed by the producer, raft3d.py:92-106).
   * Aliasing: the contract above holds for the gate operands too.  res1 / res2 / post may be the c4 tensor `out` itself
   * element for element (same buffer, ctot and coff: gate 3 with out = post) and nothing else: the kernel requests the
   * operand quads of several tiles before it stores the first of them (conv_bf16_kernel.h), a lane reads exactly the
   * quads it writes, and a lane outside the map may read -- and drop -- a quad another lane is writing. */
  int gate;
} codd_conv_params;

int codd_conv2d(const codd_conv_params* p, void* stream);
/* n <= 4 INDEPENDENT convolutions as one launch (exact-fp32 quad layout, layout = 1, npb = 1, nw = 4, one common mb of
 * 1 | 2): the resolution branches of an mmseg HRModule (configs/models/codd.py:44-74) are launch-bound ~10 us layers
 * that do not depend on each other.  CODD_EUNSUPPORTED when a job does not fit that class (launch them one by one). */
int codd_conv2d_multi(const codd_conv_params* p, int n, void* stream);
/* Dry runs (ABI v13 for layouts 0 and 1): they launch nothing and read no pointer field -- the pointer checks of
 * codd_conv2d are skipped and its alignment-dependent choices see null pointers, i.e. aligned operands -- so callers probe
 * candidate configurations before packing weights for them.
 *   codd_conv2d_lds_bytes  the dynamic LDS bytes of the launch codd_conv2d would make with this configuration (tile,
 *                          chunk depth, wave grid), or the negative CODD_E* code with which it would refuse it (LDS and
 *                          register-staging limits of the instantiated kernels)
 *   codd_conv2d_check      CODD_OK where that is >= 0, else that code */
long long codd_conv2d_lds_bytes(const codd_conv_params* p);
int codd_conv2d_check(const codd_conv_params* p);
/* The layout-2 kernels this build instantiates: writes up to `cap` quintuples (pgw, cgw, A, B, ksplit) -- A = pixel units
 * per wave row group (nw * npb = pgw * A), B = mb / cgw -- in dispatch order and returns their number. */
int codd_conv2d_bf16_instantiations(int* out, int cap);

/* quad layout (layout = 1): four input channels innermost, [cog][chunk][tap][c/4][co][4] */
long long codd_conv2d_packed_size_quad(int Cout, int Cin, int kh, int kw, int mb, int ck);
int codd_conv2d_pack_weights_quad(const float* w, float* wpacked, int Cout, int Cin, int kh, int kw, int mb,
                                  int ck, void* stream);

/* Activation re-layout for layout 2: fp32 NCHW views (in0 | in1 concatenated) -> split-bf16 records
 * xs[b][plane hi|lo][octet][yp][xp][8 bf16]; pixel (y, x) sits at (y + bt, x + bl); the border and the channels past
 * C0 + C1 are zero, so that every halo tile of the convolution is in-bounds row segments of 16-byte records (the
 * kernel's LDS-DMA copies them verbatim).  A conv needs bt >= pad_t, bl >= pad_l, 8 * (c8 - xs_o8) >= ceil(Cin / ck) * ck
 * and hp >= max(bt + H, bt - pad_t + (tiles_y * th - 1) * sy + (kh - 1) * dil_y + 1), wp likewise (th x 16*npb = its tile).
 * terms = 1: hi plane only; terms = 16: one plane of fp16 records. */
long long codd_split_bf16_bytes(int B, int c8, int hp, int wp, int terms);
int codd_split_bf16(codd_view in0, int C0, codd_view in1, int C1, int B, int H, int W, int bt, int bl,
                    int c8, int hp, int wp, int terms, void* xs, void* stream);

/* split-bf16 layout (layout = 2): [cog][chunk][plane hi|lo][k-step][g][co][8 bf16]; element (co, ci, tap) is read
 * from w[co*co_stride + ci*ci_stride + tap] and scaled (as codd_conv2d_pack_weights_ex). */
long long codd_conv2d_packed_bytes_bf16(int Cout, int Cin, int kh, int kw, int mb, int ck, int terms);
int codd_conv2d_pack_weights_bf16(const float* w, void* wpacked, int Cout, int Cin, int kh, int kw, int mb, int ck,
                                  int terms, long long co_stride, long long ci_stride, float scale, void* stream);

/* number of floats of the packed weight buffer for (Cout, Cin, kh, kw, mb, ck) */
long long codd_conv2d_packed_size(int Cout, int Cin, int kh, int kw, int mb, int ck);
/* w: [Cout][Cin][kh][kw] device pointer -> wpacked (device).  Runs on `stream`. */
int codd_conv2d_pack_weights(const float* w, float* wpacked, int Cout, int Cin, int kh, int kw,
                             int mb, int ck, void* stream);
/* generalised: element (co, ci, tap) is read from w[co*co_stride + ci*ci_stride + tap] and scaled. */
int codd_conv2d_pack_weights_ex(const float* w, float* wpacked, int Cout, int Cin, int kh, int kw,
                                int mb, int ck, long long co_stride, long long ci_stride, float scale,
                                void* stream);

/* ---------------------------------------------------------------------------------------------
 * ROLLING-WINDOW convolutions (exact fp32, v_mfma_f32_16x16x4_f32) for HITNet's large-map, few-channel stride-1
 * layers (round 4): one launch runs
 *   mode 0   y = actA(conv3x3_A(x) + bA)
 *   mode 1   y = actB(conv3x3_B(actA(conv3x3_A(x) + bA)) + bB [+ x])      BasicBlock (reference
 *            model/stereo/hitnet/propagation.py:103-121 incl. the enclosing LeakyReLU, :119-121) and the two trailing
 *            3x3 layers of a U-Net merge (backbone.py:31-39)
 *   mode 2   y = actB(conv3x3_B(actA(conv1x1_A(cat[in0, in1]) + bA)) + bB)  head of a merge / PostTileUpdate
 *            (backbone.py:24-30, propagation.py:255-258)
 * with C = 16 | 32 channels out of every stage, "same" zero padding per stage, x = cat[in0, in1] (C0 + C1 = C for
 * modes 0 / 1, <= 64 for mode 2).  A workgroup walks a 64-column strip down `rh` rows; weights stay in registers, the
 * intermediate of a pair stays in LDS (csrc/conv_roll.hip).  Weights are packed per stage by codd_roll_pack_weights
 * (w: [Cout][Cin][k][k] fp32, Cout <= C, output channels past Cout are zero; codd_roll_packed_size floats).
 * Only channels [0, cout_store) of the last stage are written.
 * --------------------------------------------------------------------------------------------- */
typedef struct {
  codd_view in0, in1;
  int C0, C1;
  int B, H, W;
  int C;                 /* 16 | 32 */
  int mode;              /* 0 | 1 | 2 */
  const float* wA;       /* packed weights of stage A (16-byte aligned) */
  const float* bA;       /* bias of stage A or NULL */
  const float* wB;       /* stage B (modes 1, 2) */
  const float* bB;
  int actA, actB;        /* CODD_ACT_* */
  int residual;          /* mode 1: add the chain input before actB */
  float* out;            /* NCHW, channels [out_coff, out_coff + cout_store) of a buffer with out_ctot channels */
  int out_ctot, out_coff, cout_store;
  int rh;                /* output rows per workgroup (launch granularity; any value >= 1 gives the same result) */
} codd_roll_params;
long long codd_roll_packed_size(int C, int k, int Cin);
int codd_roll_pack_weights(const float* w, float* packed, int C, int Cout, int Cin, int k, void* stream);
int codd_conv_roll(const codd_roll_params* p, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Stereo (HITNetMF)
 * --------------------------------------------------------------------------------------------- */
/* Tile cost volume + first arg-min, fused (never materialises cv):
 *   cost[y,x] = min_d sum_c |L[c,y,x] - R~[c,y,4x-d]|, d in [0,D), R~ = 0 outside [0,Wr)
 * replaces calc_init_disp + torch.min (initialization.py:18-45, 167-183).
 * L [B,C,Ht,Wt], R [B,C,Ht,Wr]; cost -> view channel 0 of `cost` buffer, disparity (as float)
 * -> channel 0 of `disp` buffer; dx, dy (channels 1,2 of the hypothesis) are zeroed when
 * zero_dxdy != 0 (initialization.py:192-208). */
int codd_tile_costvol_argmin(const float* L, const float* R, int B, int C, int Ht, int Wt, int Wr, int D,
                             float* cost, int cost_ctot, int cost_coff,
                             float* disp, int disp_ctot, int disp_coff, int zero_dxdy, void* stream);

/* Local slanted-plane correlation (TileWarping.forward, propagation.py:61-86) fused with the
 * ||fea_l||_1 unshuffle (propagation.py:157,207).  For each of `nhyp` (1 or 2) plane sets
 * (d,dx,dy = channels 0..2 of hyp{0,1}) writes 64 channels [fea(16) | cv(k=-1,0,1)(48)] into
 * out{0,1}.  fl, fr: [B,C,4Ht,4Wt]. */
int codd_tile_warp_cost(const float* fl, const float* fr, int B, int C, int Ht, int Wt,
                        codd_view hyp0, codd_view hyp1, int nhyp,
                        float* out0, float* out1, void* stream);

/* Plane up-sampling of a 16-channel hypothesis (propagation.py:10-32): channel 0 =
 * (d + (j-(s-1)/2) dx + (i-(s-1)/2) dy) * scale on an s-times finer grid (s = 2), channels
 * 1..15 nearest.  in [B,16,h,w] view -> out view [B,16,2h,2w]. */
int codd_hyp_upsample(codd_view in, int B, int h, int w, float scale,
                      float* out, int out_ctot, int out_coff, void* stream);

/* Hypothesis selection of TileUpdate (propagation.py:225-240): upd [B,34,h,w] = lastconv output;
 * cur / prev: 16-channel views; out [B,16,h,w] view. */
int codd_hyp_select(const float* upd, codd_view cur, codd_view prev, int B, int h, int w,
                    float* out, int out_ctot, int out_coff, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Motion (Motion + RAFT3D)
 * --------------------------------------------------------------------------------------------- */
/* InstanceNorm2d (affine=False, eps=1e-5) + optional residual + optional ReLU
 * (blocks/extractor.py:9-58,119-199):  y = relu?( (x - mean_c)/sqrt(var_c + eps) [+ res] ).
 * stats: 8-byte aligned scratch of 128*B*C floats (fp64 partial moments, <= 32 parts per plane). */
int codd_instnorm(const float* x, int B, int C, int HW, float* stats, const float* res, int relu,
                  float* y, void* stream);
/* ... with the result written as split-bf16 records (the next convolution's input form, codd_xs_view: image interior
 * only) and, when y != NULL, as fp32 too:  v = norm(x); relu ? max(v,0); res ? (v += res; relu_after_res ? max(v,0)).
 * The second ReLU is the residual block's (blocks/extractor.py:52-58): InstanceNorm -> ReLU -> + x -> ReLU -> re-layout
 * in one launch.  C must be a multiple of 8. */
int codd_instnorm_xs(const float* x, int B, int C, int H, int W, float* stats, const float* res, int relu,
                     int relu_after_res, float* y, codd_xs_view xs, void* stream);

/* All-pairs correlation pyramid (CorrBlock.__init__/corr, blocks/corr.py:28-45,56-62):
 * lvl0[n1,n2] = <f1[:,n1], f2[:,n2]> / 16, lvl_{i+1} = avg_pool2d(lvl_i, 2) over (y2,x2), computed by
 * linearity as <f1, avg_pool^i(f2)> / 16 so the 300 MB level-0 volume is never re-read.
 * f1,f2 [B,D,h,w]; lvl_i [B,h*w,(h>>i)*(w>>i)]. */
int codd_allpairs_corr(const float* f1, const float* f2, int B, int D, int h, int w,
                       float* lvl0, float* lvl1, float* lvl2, float* lvl3, float* scratch, void* stream);
/* floats of `scratch` codd_allpairs_corr needs (packed f1 + pooled f2 levels) */
long long codd_allpairs_corr_scratch(int B, int D, int h, int w);
/* avg_pool2d(kernel 2, stride 2, floor): in [BC,h,w] -> out [BC,h/2,w/2] */
int codd_avgpool2(const float* in, int BC, int h, int w, float* out, void* stream);

/* Pyramid lookup (lietorch_extras.corr_index_forward, call site blocks/corr.py:10-18,47-54):
 * out[b, l*49 + i*7 + j, y, x] = bilinear(lvl_l[b,y,x,:,:], (cx/2^l - 3 + i, cy/2^l - 3 + j)), zero
 * outside.  coords [B,h,w,3] (x,y,*) with stride `cstride` floats per pixel. */
int codd_corr_lookup(const float* lvl0, const float* lvl1, const float* lvl2, const float* lvl3,
                     const float* coords, int cstride, int B, int h, int w, float* out, void* stream);

/* Per-iteration geometry (raft3d.py:225-240; projective_ops.py:11-52; sampler_ops.py:9-28;
 * SE3.log): from T [B,h,w,7], depth1/depth2 [B,h,w] at 1/8 res and K8 = (fx,fy,cx,cy)/8:
 *   xyz    [B,h,w,3] = project(T * inv_project(depth1))
 *   minfo  [B,9,h,w] = clamp([xy - grid, 10*log(T), 10*(bilinear(1/depth2, xy) - xyz.z)], +-50)
 */
int codd_raft_geometry(const float* T, const float* depth1, const float* depth2, int B, int h, int w,
                       float fx, float fy, float cx, float cy, float* xyz, float* minfo, void* stream);

/* Dense SE3 Gauss-Newton step (se3_field.step_inplace, se3_field.py:150-170 =
 * lietorch_extras.se3_build_inplace + damping + cholesky6x6_forward + SE3.exp(dx) * Ts).
 * ae [B,32,h,w] (raw head output; /8 applied inside), delta/weight [B,3,h,w]; target = xyz + delta.
 * T is updated in place.  Hb: scratch of codd_se3_gn_scratch(B,h,w,radius) floats, 16-byte aligned, three regions and
 * nothing else: the per-workgroup partial normal equations (combined in a fixed order -> deterministic), the packed
 * 176-byte neighbour records, and the pair builder's second image of the per-neighbour scalars.  Every float of it is
 * written before it is read, and nothing past it is touched. */
long long codd_se3_gn_scratch(int B, int h, int w, int radius);
int codd_se3_gn_step(float* T, const float* ae, int ae_c, const float* xyz, const float* delta,
                     const float* weight, const float* depth1, int B, int h, int w,
                     float fx, float fy, float cx, float cy, int radius, float lm, float ep,
                     float* Hb, void* stream);

/* The same step with the three 1x1 heads of the update block folded into the record packing (raft3d.py:59-61,
 * 100-104: ae = conv1x1(256->32), delta = conv1x1(256->3), weight = sigmoid(conv1x1(256->3))).
 * hidden: the 768 post-ReLU hidden channels [ae | delta | weight groups of 256] in split-bf16 form (written by the
 * fused 3x3 head convolution).  head_w: the 38 x 256 head weights as MFMA A operands,
 *   [32 blocks][plane hi|lo][lane 0..63][8 bf16]  (64 KB, 16-byte aligned): block t*8+s (t = 0, 1; s = 0..7) holds ae
 *   rows 16t + lane%16, channels 32s + 8*(lane/16) .. +8; block 16+s (s = 0..15) holds row lane%16 of
 *   [delta0..2 | weight0..2 | zeros] at hidden channel 256 + 32s + 8*(lane/16) .. +8 (zero where the row's head does
 *   not read that channel group); hi = bf16_rne(w), lo = bf16_rne(w - hi).  head_b [38] fp32 (ae, delta, weight).
 * weight_out [B,3,h,w] receives the confidence weights (up-sampled by the caller after the last update). */
int codd_se3_gn_step_heads(float* T, codd_xs_view hidden, const void* head_w, const float* head_b,
                           const float* xyz, const float* depth1, int B, int h, int w, float fx, float fy,
                           float cx, float cy, int radius, float lm, float ep, float* weight_out, float* Hb,
                           void* stream);

/* Convex 8x up-sampling (se3_field.cvx_upsample, se3_field.py:173-186) of `dim` channels.
 * mode 0: data [B,h,w,dim] -> out [B,8h,8w,dim]             (generic)
 * mode 1: data = SE3 field [B,h,w,7]: out = exp(cvx(log(T)))  (upsample_se3, :189-192)
 * mode 2: data [B,dim,h,w] -> out [B,dim,8h,8w]              (weight, raft3d.py:271-273) */
int codd_cvx_upsample(const float* data, const float* mask, int B, int h, int w, int dim, int mode,
                      float* out, void* stream);
/* upsample_se3 (mode 1) of T [B,h,w,7] and the convex up-sampling (mode 2) of weight [B,3,h,w] with the same mask in one
 * pass (raft3d.py:267-273): T_out [B,8h,8w,7], weight_out [B,3,8h,8w]. */
int codd_cvx_upsample_se3_weight(const float* T, const float* weight, const float* mask, int B, int h, int w,
                                 float* T_out, float* weight_out, void* stream);

/* disparity -> depth (motion.py:154-165): depth = clip(bf / (disp + 1e-5), 0, 210). */
int codd_disp_to_depth(const float* disp, long long n, float bf, float* depth, void* stream);
/* out[b][y][x] = in[b][oy + step*y][ox + step*x], out is [B][ceil((H-oy)/step)][ceil((W-ox)/step)]: RAFT3D's
 * 1/8-resolution depth samples `depth[:, 3::8, 3::8]` (reference model/motion/raft3d/raft3d.py:213-216). */
int codd_subsample(const float* in, int B, int H, int W, int oy, int ox, int step, float* out, void* stream);

/* Forward splat of the previous state into the current frame (Motion.transform_and_project,
 * motion.py:82-130 = pytorch3d PointsRasterizer(K=8) + AlphaCompositor) fused with
 * induced_flow (projective_ops.py:55-68) for the full-resolution call.
 *   T [B,Hs,Ws,7] sampled at (oy + ds*y, ox + ds*x) of a [B,HT,WT,7] field, depth likewise;
 *   feat channels = concat(featA [CA], flow(3, computed when with_flow), featB [CB]);
 *   out [B,C,H,W], zout [B,1,H,W] (nearest z, 0 when empty) or disparity when bf > 0:
 *   disp = bf/(z+1e-5), > W -> 0 (motion.py:190-193).
 * scratch: 16-byte aligned, codd_splat_scratch(B, H, W, radius) ints (per-pixel counters / list offsets, EXACT-SIZE
 * candidate lists -- a point covers at most (2 ceil(R) + 1)^2 pixel centres, R = radius min(H,W) / (2H) px, which
 * bounds them: no candidate is ever dropped -- and one float4 (u, v, z, valid) per source point).
 * CODD_EINVAL: a NULL T / depth / out / scratch, a missing feature pointer, a scratch that is not 16-byte aligned,
 * radius not > 0, B, H, W, HT, WT or ds < 1, oy or ox < 0, a sample outside the field (oy + ds (H - 1) >= HT,
 * ox + ds (W - 1) >= WT); nothing is launched then.  codd_splat_scratch returns -1 for sizes < 1 or radius not > 0.
 *
 * Scratch layout, in ints, once the launches have completed; n = B H W, bound = (2 ceil(R) + 1)^2, R evaluated in
 * fp32, nhead = (3 n + 4 + 3) & ~3, nlist = (n bound + 3) & ~3, codd_splat_scratch = nhead + nlist + 4 n:
 *   [0, n)                  cnt:  candidates of output pixel (b, y, x) at (b H + y) W + x: the valid points of item b
 *                                 with d^2 < R^2 to the pixel's centre (x + 0.5, y + 0.5);
 *   [n, 2 n)                off:  where the pixel's list starts in `list` (any value where cnt is 0);
 *   [2 n, 3 n)              cur:  entries the fill pass wrote into the pixel's list: equal to cnt;
 *   [3 n]                   cursor: entries in `list` = the sum of cnt; [3 n + 1, 3 n + 4) are 0; the rest of the
 *                                 head up to nhead is not written;
 *   [nhead, nhead + nlist)  list: the ranges [off, off + cnt) of the pixels with cnt > 0 are disjoint and tile
 *                                 [0, cursor) (in no particular order); an entry is the index y W + x of a source point
 *                                 of the pixel's own item, each point at most once per list, in no particular order;
 *                                 entries from cursor on are not written;
 *   [nhead + nlist, + 4 n)  uvz:  per source point (b H + y) W + x four floats: the projected u, v, z = (T X0).z and
 *                                 valid = 1.f (z > 0, |u| < 1e7, |v| < 1e7) or 0.f (u, v then meaningless).
 * The count and the fill pass decide coverage with the same fp32 expression on the same stored (u, v); the gather
 * pass reads exactly these lists. */
long long codd_splat_scratch(int B, int H, int W, float radius);
int codd_splat(const float* T, const float* depth, int HT, int WT, int oy, int ox, int ds,
               const float* featA, int CA, const float* featB, int CB, int with_flow,
               int B, int H, int W, float fx, float fy, float cx, float cy, float radius,
               float bf, float* out, float* zout, int* scratch, void* stream);

/* induced_flow (projective_ops.py:55-68): out [B,H,W,3] = project(T*X0) - project(X0). */
int codd_induced_flow(const float* T, const float* depth, int B, int H, int W,
                      float fx, float fy, float cx, float cy, float* out, void* stream);

/* context split (raft3d.py:183-186): net = tanh(x[:, :128]), inp = relu(x[:, 128:512]). */
int codd_context_split(const float* x, int B, int hw, float* net, float* inp, void* stream);

/* SE3.Identity field (raft3d.py:173): T [npix, 7] = (0,0,0, 0,0,0,1). */
int codd_se3_identity(float* T, long long npix, void* stream);

/* bilinear resize (HRNet fuse layers, align_corners = 0; ResizeConcatConv, align_corners = 1):
 * out view += / = resize(in).  accumulate: 0 overwrite, 1 add; relu applied after. */
int codd_resize_bilinear(const float* in, int B, int C, int Hi, int Wi, int Ho, int Wo, int align_corners,
                         float* out, int out_ctot, int out_coff, int accumulate, int relu, void* stream);
/* as codd_resize_bilinear, plus `extra` (contiguous [B, C, Ho, Wo], out_ctot == C, out_coff == 0 expected by the index):
 * out = relu?((out + extra) + blend) when accumulate, (extra + blend) otherwise -- the "+ x_i" term of an mmseg HRModule
 * fuse layer (configs/models/codd.py:44-74) folded into the neighbouring up-sampling term, with the roundings of the two
 * separate launches. */
int codd_resize_bilinear_add(const float* in, int B, int C, int Hi, int Wi, int Ho, int Wo, int align_corners,
                             float* out, int out_ctot, int out_coff, int accumulate, int relu, const float* extra,
                             void* stream);

/* y = relu?(a + b) elementwise (HRNet fuse sums), n floats. */
int codd_add_relu(const float* a, const float* b, long long n, int relu, float* y, void* stream);
/* dst[k][0..n[k]) = src[k][0..n[k]) for k < count <= 8 in ONE launch (the recurrent-state write-back at the end of a
 * captured frame); every n[k] a multiple of 4, every pointer 16-byte aligned. */
int codd_copy_many(const float* const* src, float* const* dst, const long long* n, int count, void* stream);
/* dst[0..n) = src[0..n) bit for bit, 32-bit words at any 4-byte alignment, any n >= 0 (the pairs of ops.copy_many that
 * miss the 16-byte rules of codd_copy_many; a kernel node under graph capture). */
int codd_copy(const float* src, float* dst, long long n, void* stream);

/* Diagnostics: *slot = the device's constant-rate wall clock (100 MHz ticks) when this one-thread launch runs -- a
 * marker inside a captured frame that does not perturb the replay the way a profiler does (tools/frame_marks.py). */
int codd_timestamp(long long* slot, void* stream);

/* ConvGRU gate fusions (blocks/gru.py:17-34).  t1, t2: the two gate convolutions of a gate pair
 * (3x3 and dilated 3x3, bias included); inp / cor / mot [B,384,hw]: the three input streams.
 *   zr [B,256,hw] = sigmoid(t1 + t2 + (inp+cor+mot)[:, :256]);  rh [B,128,hw] = r * h
 *   hout [B,128,hw] = (1 - z) h + z tanh(t1 + t2 + (inp+cor+mot)[:, 256:]) */
int codd_gru_gate_zr(const float* t1, const float* t2, const float* inp, const float* cor,
                     const float* mot, const float* h, int B, int hw, float* zr, float* rh, void* stream);
int codd_gru_gate_q(const float* t1, const float* t2, const float* inp, const float* cor,
                    const float* mot, const float* zr, const float* h, int B, int hw, float* hout,
                    void* stream);


/* The same gates, writing what the following convolutions read directly in their input form (no fp32 tensor, no
 * re-layout pass between gate and convolution):
 *   zr_xs: z [B,128,hw] fp32 (only z is read again) and r*h as split records into rh_xs (128 channels);
 *   q_xs:  z as written by zr_xs; the new hidden state as fp32 hout AND as split records into h_xs. */
int codd_gru_gate_zr_xs(const float* t1, const float* t2, const float* inp, const float* cor, const float* mot,
                        const float* h, int B, int H, int W, float* z, codd_xs_view rh_xs, void* stream);
int codd_gru_gate_q_xs(const float* t1, const float* t2, const float* inp, const float* cor, const float* mot,
                       const float* z, const float* h, int B, int H, int W, float* hout, codd_xs_view h_xs,
                       void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fusion
 * --------------------------------------------------------------------------------------------- */
/* 1/ds-resolution cues (fusion.py:200-241, 168-198, 243-318), patch = corr_cfg.patch_size (3 or 5; P2 = patch^2),
 * ds = Fusion.ds_scale (even): corr_feat [B, 3 P2 + 4, H/ds, W/ds] =
 * [feat cross (P2) | feat self curr (P2-1) | feat self warp (P2-1) | cost_curr (3) | cost_warp (3)]  (31 at patch 3)
 * and the sub-sampled disparities pc, pw (fuse(), fusion.py:331-342) written to channels
 * (dsub_coff, dsub_coff+1) of dsub. */
int codd_fusion_cues_lr(const float* pred_curr, const float* pred_warp, const float* feat_curr,
                        const float* feat_warp, const float* fea_l, const float* fea_r,
                        int B, int H, int W, int patch, int ds, int CF, int CS, float* corr_feat,
                        float* dsub, int dsub_ctot, int dsub_coff, void* stream);

/* Full-resolution cues (fusion.py:243-318): corr_feat_fr [B, 3 P2 + 5, H, W] = [|disp cross| (P2) |
 * |disp self curr| (P2-1) | |disp self warp| (P2-1) | flow_warp (3) | pred_warp>0 (1) | conf_warp (3)]  (32 at patch 3). */
int codd_fusion_cues_fr(const float* pred_curr, const float* pred_warp, const float* flow_warp,
                        const float* conf_warp, int B, int H, int W, int patch, float* out, void* stream);

/* The full-resolution forget branch in one launch (fusion.py:123-132, 243-318): the cue map of codd_fusion_cues_fr fed
 * through forget_head = Conv1x1(nc->16), Conv3x3(16->8, pad 1), Conv1x1(8->1), Sigmoid without materialising the cue
 * tensor or the 16- / 8-channel maps.  The head is linear up to the sigmoid, so the caller passes it MERGED:
 *   weff = [ W_eff[9][nc] | beta[9] | c0 ],  W_eff[k] = w2.W1[:,:,k].W0,  beta_k = w2.W1[:,:,k].b0,  c0 = w2.b1 + b2
 * (nc = 3 patch^2 + 5; tap k = ky*3 + kx of the 3x3).  A tap contributes W_eff[k].cues(p+k) + beta_k only where p+k lies
 * inside the image (the 3x3's zero padding acts on the biased 16-channel map).  wr [B,1,H,W] = sigmoid(...). */
int codd_fusion_forget(const float* pred_curr, const float* pred_warp, const float* flow_warp,
                       const float* conf_warp, int B, int H, int W, int patch, const float* weff, float* wr,
                       void* stream);

/* Blend (fusion.py:383-394): wf = up4(wf_lr) * (pw>0); wr *= (pw>0);
 * fused = pc*(1-wf*wr) + pw*wf*wr. */
int codd_fusion_blend(const float* pred_curr, const float* pred_warp, const float* wf_lr,
                      const float* wr_logit_sig, int B, int H, int W, int ds,
                      float* fused, float* wf_out, float* wr_out, void* stream);

/* The three metric entry points below share two rules.
 * Batch: the B items of a call are B FRAMES, added to ``meters`` in index order -- one call at B equals B calls at
 * B = 1 on the items in turn (bit for bit for codd_disp_metrics / codd_tepe_metrics, whose meters receive one mean per
 * item; up to the fp64 rounding of the sums for codd_sceneflow_metrics).  An item whose mask is empty moves neither its
 * means nor its count.  This is NOT the joint mean over a batch that a torch restatement fed B > 1 forms.
 * Nearest warp (codd_tepe_metrics, codd_gt_motion): the source pixel of (x, y) under the flow (fx, fy) is
 * (rint((float)x + fx), rint((float)y + fy)) -- the fp32 sum rounded half to even -- and it is inside the map when the
 * ROUNDED value lies in [0, w - 1] x [0, h - 1] (so x + fx = -0.5 rounds to 0 and is inside, (w - 1) + 0.5 is inside when
 * w - 1 is even).  grid_sample's normalise / un-normalise arithmetic picks a neighbouring pixel at some exact
 * half-integer coordinates ("Pointwise kernels"); this rule is the exact one and is kept.
 * All three return CODD_EINVAL for h < 1, w < 1, h > H or w > W.
 *
 * On-device disparity metrics (model/codd.py:456-471; utils/metric.py:9-17,40-54): over the mask
 * lo < gt < hi of the crop [0,h) x [0,w) of [B,1,H,W] maps, adds the frame's EPE, its > thr rate and
 * 1 to meters[0..2] (fp64, AverageMeter semantics) when the mask is non-empty.  No host sync.
 * scratch: 3*128*B doubles. */
int codd_disp_metrics(const float* pred, const float* gt, int B, int H, int W, int h, int w,
                      float lo, float hi, float thr, double* scratch, double* meters, void* stream);

/* Temporal metrics (model/codd.py:473-521; utils/metric.py:19-37; utils/warp.py:69-92): pulls the current
 * (gt, pred, mask) back with the previous frame's GT flow [B,2,H,W] (nearest, zeros) and adds the
 * frame's mean TEPE, (TEPE>3) rate, relative TEPE, (rel>1) rate and 1 to meters[0..4] (when the joint mask
 * is non-empty), mean |flow| and 1 to meters[5..6].  scratch: 6*128*B doubles.  No host sync.  gt_mask (or NULL = gt): the map the current frame's validity mask is computed from -- the reference substitutes a
 * constant in-range map for frames without any disparity ground truth (model/codd.py:478-486); gt2_prev (or NULL):
 * ground-truth second-frame disparity in the previous frame's coordinates, used instead of the flow-warped gt and
 * requiring gt2_prev > 0 (:497-499). */
int codd_tepe_metrics(const float* pred, const float* gt, const float* pred_prev, const float* gt_prev,
                      const float* flow_prev, const float* gt_mask, const float* gt2_prev, int B, int H, int W,
                      int h, int w, float lo, float hi, float bf, double* scratch, double* meters, void* stream);

/* Scene-flow metric columns (model/codd.py:519-575; utils/misc.py:12-36, 62-77): over the crop [0,h) x [0,w) of
 * [B,*,H,W] maps and the mask lo < gt_disp_prev < hi & |gt_flow_prev| < bf & |gt_disp_change| < bf (& gt_flow_occ == 0
 * when given), with est = induced_flow(Ts, clip(bf / pred_prev, 0, bf), K) and est.z * bf (inverse depth ->
 * disparity): meters[0..4] += count, sum of 3-D end-point errors, sum of 2-D ones, #(3-D < 1 px), #(2-D < 1 px) -- the
 * reference's count / epe2d_scene_flow / epe2d_optical_flow / 1px_scene_flow / 1px_optical_flow accumulators.
 * Ts [B,H,W,7]; gt_flow_prev [B,2,H,W]; gt_flow_occ: bytes [B,1,H,W] or NULL.  scratch: 5*128*B doubles. */
int codd_sceneflow_metrics(const float* Ts, const float* pred_prev, const float* gt_disp_prev,
                           const float* gt_flow_prev, const float* gt_disp_change, const unsigned char* gt_flow_occ,
                           int B, int H, int W, int h, int w, float lo, float hi, float bf, float fx, float fy,
                           float cx, float cy, double* scratch, double* meters, void* stream);

/* Input pre-processing (datasets/transforms.py:147-161,373-427; formating.py:65-85): uint8 HWC image
 * (device) -> fp32 CHW RGB, (x - mean)/std, reflect-padded bottom/right to [3,H,W].  mean/stdv: host
 * pointers to 3 floats in RGB order. */
int codd_preprocess(const unsigned char* img, int h, int w, int bgr, const float* mean, const float* stdv,
                    int H, int W, float* out, void* stream);

/* Live-session ingest (codd_amd/live.py): BOTH views of one frame in one launch.  Replaces, per camera frame, the two
 * Pad + Normalize + format passes of the reference's test pipeline (datasets/transforms.py:147-161, 373-427;
 * datasets/formating.py:65-85, run on img and r_img by datasets/custom_stereo_mf.py) and the host cv2.remap a user
 * of the reference runs in front of them on an unrectified rig.
 *   left, right   uint8 [h,w,3] HWC (device); out_left, out_right fp32 [3,H,W] (device, caller-owned: no allocation);
 *   mean / stdv   host pointers to 3 floats in RGB order; bgr != 0: the source is BGR.
 * Without maps (all four NULL) each output is bit-identical to codd_preprocess() of that view.
 * With maps (map_x, map_y: fp32 [h,w] per view, device, the layout cv2.initUndistortRectifyMap produces; a view's two
 * maps are given together or not at all, each view independently), pixel (y,x) of the rectified h x w image is the
 * bilinear sample of the source at (sx, sy) = (map_x[y,x], map_y[y,x]):
 *   x0 = floor(sx), y0 = floor(sy); weights ax = sx - x0, ay = sy - y0 computed in fp32;
 *   a tap outside the source contributes 0 in raw uint8 units; a non-finite map entry gives 0;
 *   v = (v00*(1-ax) + v01*ax)*(1-ay) + (v10*(1-ax) + v11*ax)*ay in fp32, NOT rounded back to uint8; then (v - mean)/std.
 * THE BLEND.  The fp32 operation order of v, per channel, in every ingest entry and for every source format (fma = one
 * fused multiply-add, every other operation rounded to nearest on its own; v00, v01 the taps of row y0 at x0, x0 + 1 and
 * v10, v11 those of row y0 + 1, as floats):
 *   w0 = 1 - ax;  w1 = 1 - ay
 *   top = fma(v00, w0, v01 * ax);  bot = fma(v10, w0, v11 * ax)
 *   v   = fma(top, w1, bot * ay)
 * On maps whose entries are multiples of 1/64 pixel (and on the identity map) no operation rounds at all.
 * The padded border is the BORDER_REFLECT_101 reflection of the RECTIFIED image.  An identity map gives the bits of the
 * map-free path.  Same size rules as codd_preprocess: h <= H < 2h, w <= W < 2w. */
int codd_ingest_pair(const unsigned char* left, const unsigned char* right, int h, int w, int bgr, const float* mean,
                     const float* stdv, const float* lmap_x, const float* lmap_y, const float* rmap_x,
                     const float* rmap_y, int H, int W, float* out_left, float* out_right, void* stream);

/* Live-session ingest of raw camera formats: codd_ingest_pair on frames as a camera, an ISP or a hardware decoder hands
 * them out, decoded inside the same pass.  The contract is "decode, then ingest": for every format F a decoder
 * D_F(frame) -> uint8 [h,w,3] RGB is defined below in integer arithmetic, and the outputs are, bit for bit, what
 *   codd_ingest_pair(D_F(left), D_F(right), h, w, bgr = 0, mean, stdv, maps..., H, W, ...)
 * writes: the (c - mean)/std expression, the BORDER_REFLECT_101 padding of the DECODED, RECTIFIED image and, with maps,
 * the bilinear blend of codd_ingest_pair, each of whose four taps is D_F at the integer source pixel (0 outside).  The
 * decoded image is never written to memory.
 * A format is named by its bytes in memory; pitch is the bytes per source row, 0 = tight (the row's own bytes):
 *   CODD_FMT_MONO8        [h][pitch], 1 byte per pixel, R = G = B = the byte;                          h, w >= 1
 *   CODD_FMT_YUYV         [h][pitch], per pixel pair Y0 U Y1 V (row bytes 2w);                         w even
 *   CODD_FMT_UYVY         [h][pitch], per pixel pair U Y0 V Y1 (row bytes 2w);                         w even
 *   CODD_FMT_NV12         Y plane [h][pitch], then at byte pitch*h the interleaved U V plane [h/2][pitch]; w, h even
 *   CODD_FMT_BAYER_RGGB, _GRBG, _GBRG, _BGGR   [h][pitch], 1 byte per pixel; the name spells the colours of pixels
 *                         (0,0), (0,1), (1,0), (1,1);                                                  h, w >= 2
 * codd_frame_bytes: the bytes of one view, pitch * rows with rows = h (3h/2 for NV12); -1 for an unknown format, a
 * violated size rule, or a pitch that is neither 0 nor >= the row's bytes.  No byte outside [0, codd_frame_bytes) of
 * either view is read.
 * YUV -> RGB.  Chroma is nearest, never interpolated: pixel (y,x) takes U, V of its pair x>>1 (NV12: of its block
 * (y>>1, x>>1)).  int32 arithmetic, >> arithmetic:
 *   yy = max(Y - yoff, 0) * CY;                         sat8(v) = min(max(v, 0), 255)
 *   R = sat8((yy + (1<<19) + CVR*(V-128)) >> 20)
 *   G = sat8((yy + (1<<19) - CUG*(U-128) - CVG*(V-128)) >> 20)
 *   B = sat8((yy + (1<<19) + CUB*(U-128)) >> 20)
 * each coefficient the integer nearest to c * 2^20, c from the row that `yuv` selects (ignored for mono and Bayer):
 *   yuv  name                        yoff  CY     CVR    CUG    CVG    CUB
 *   0    bt601, video range          16    1.164  1.596  0.391  0.813  2.018   (1220542, 1673527, 409993, 852492,
 *   1    bt709, video range          16    1.164  1.793  0.213  0.533  2.112    2116026: the integers OpenCV uses)
 *   2    jpeg, BT.601 full range     0     1.000  1.402  0.344  0.714  1.772
 * (every accumulator stays below 5.8e8 in magnitude).
 * Bayer: bilinear demosaic on the 3x3 window of the mosaic extended by reflect-101 (index -1 -> 1, n -> n-2, which
 * keeps the colour parity; with n = 2 both neighbours are the same pixel).  At an R or B site: own colour = the byte,
 * G = (N+S+W+E+2)>>2, the opposite colour = (NW+NE+SW+SE+2)>>2.  At a G site: G = the byte, the colour of its row
 * neighbours = (W+E+1)>>1, the colour of its column neighbours = (N+S+1)>>1.  The mosaic of a flat colour decodes to
 * exactly that colour at every pixel.
 * left, right: device, codd_frame_bytes each, ANY alignment; maps, mean / stdv, outputs and the h <= H < 2h, w <= W < 2w
 * rules as codd_ingest_pair (outputs: float alignment; 16-byte stores only when W % 4 == 0 and the output is 16-byte
 * aligned).
 * CODD_EINVAL, before any launch: a NULL image, mean, stdv or output; an unknown fmt; for a YUV format a yuv outside
 * 0..2; a violated size rule; pitch neither 0 nor >= the row's bytes; one map of a view without the other; a violated
 * H, W rule. */
#define CODD_FMT_MONO8 1
#define CODD_FMT_YUYV 2
#define CODD_FMT_UYVY 3
#define CODD_FMT_NV12 4
#define CODD_FMT_BAYER_RGGB 5
#define CODD_FMT_BAYER_GRBG 6
#define CODD_FMT_BAYER_GBRG 7
#define CODD_FMT_BAYER_BGGR 8
#define CODD_YUV_BT601 0
#define CODD_YUV_BT709 1
#define CODD_YUV_JPEG 2
int codd_ingest_frames(const unsigned char* left, const unsigned char* right, int fmt, int yuv, int h, int w,
                       long long pitch, const float* mean, const float* stdv, const float* lmap_x, const float* lmap_y,
                       const float* rmap_x, const float* rmap_y, int H, int W, float* out_left, float* out_right,
                       void* stream);
long long codd_frame_bytes(int fmt, int h, int w, long long pitch);

/* Rectification from a stereo calibration (codd_amd/calibration.py, LiveSession(calibration=)): the rectifying map as a
 * closed-form function of one view's calibration, written out as map arrays (codd_rectify_maps) or evaluated in
 * registers inside the ingest launch (codd_ingest_calibrated).
 * One view is described by a codd_calib_view, all doubles: R, the rectifying rotation R_rect (row-major, X_rect = R_rect
 * X_cam); f, cx, cy, the rectified pinhole camera (f' = fx' = fy', cx', cy'); K = (fx, fy, cx, cy) and dist, the source
 * camera; model, CODD_CALIB_BROWN (dist = k1 k2 p1 p2 k3 k4 k5 k6, OpenCV's rational model) or CODD_CALIB_FISHEYE
 * (dist = k1 k2 k3 k4 of Kannala-Brandt as cv2.fisheye, dist[4..7] ignored).
 * THE MAP FUNCTION.  Rectified pixel (u, v) of a view maps to the source position (sx, sy):
 *   xr = (u - cx') / f',  yr = (v - cy') / f'
 *   (X, Y, W) = R_rect^T (xr, yr, 1);   W <= 0 or non-finite  ->  (sx, sy) = NaN   (the pixel reads 0)
 *   x = X / W, y = Y / W, r2 = x^2 + y^2
 *   brown:   kr = (1 + k1 r2 + k2 r2^2 + k3 r2^3) / (1 + k4 r2 + k5 r2^2 + k6 r2^3)
 *            xd = x kr + 2 p1 x y + p2 (r2 + 2 x^2),   yd = y kr + p1 (r2 + 2 y^2) + 2 p2 x y
 *   fisheye: r = sqrt(r2), t = atan(r), td = t (1 + k1 t^2 + k2 t^4 + k3 t^6 + k4 t^8), s = r > 1e-8 ? td / r : 1,
 *            xd = x s, yd = y s
 *   sx = fx xd + cx,  sy = fy yd + cy
 * The constants.  The entry computes them on the host in fp64 and rounds each ONCE to fp32: the nine entries of
 * M = R_rect^T K'^-1, so that (X, Y, W) = M (u, v, 1):
 *   m[3i] = R[0][i] / f',  m[3i+1] = R[1][i] / f',  m[3i+2] = R[2][i] - (R[0][i] cx' + R[1][i] cy') / f'     (i = 0, 1, 2)
 * and fx, fy, cx, cy, dist[0..7].
 * The fp32 operation order of the kernels (fma = one fused multiply-add, every other operation rounded to nearest on
 * its own; u, v the pixel's integer coordinates as floats; division and sqrt correctly rounded; atan is atanf):
 *   X = fma(m0, u, fma(m1, v, m2));  Y = fma(m3, u, fma(m4, v, m5));  W = fma(m6, u, fma(m7, v, m8))
 *   !(0 < W < +inf)  ->  sx = sy = NaN
 *   iw = 1 / W;  x = X * iw;  y = Y * iw;  xx = x * x;  yy = y * y;  r2 = fma(y, y, xx)
 *   brown:   num = fma(fma(fma(k3, r2, k2), r2, k1), r2, 1);  den = fma(fma(fma(k6, r2, k5), r2, k4), r2, 1)
 *            kr = num / den;  xy2 = (x + x) * y
 *            xd = fma(x, kr, fma(p1, xy2, p2 * fma(2, xx, r2)));  yd = fma(y, kr, fma(p2, xy2, p1 * fma(2, yy, r2)))
 *   fisheye: r = sqrt(r2);  t = atanf(r);  t2 = t * t
 *            td = t * fma(fma(fma(fma(k4, t2, k3), t2, k2), t2, k1), t2, 1);  s = r > 1e-8f ? td / r : 1
 *            xd = x * s;  yd = y * s
 *   sx = fma(fx, xd, cx);  sy = fma(fy, yd, cy)
 * A value that overflows on the way (a pixel near the W = 0 horizon) ends as inf or NaN and reads 0 like any
 * non-finite map entry.
 *
 * codd_rectify_maps writes map_x, map_y (fp32 [h,w], device) of each view whose struct is not NULL -- exactly the maps
 * codd_ingest_pair / codd_ingest_frames take, and what cv2.remap takes.  CODD_EINVAL before any launch: both structs
 * NULL; h or w <= 0; a map pointer NULL for a view that has a struct; an unknown model; a non-finite entry in a struct;
 * f', fx or fy not positive.
 *
 * codd_ingest_calibrated is codd_ingest_pair (fmt = CODD_FMT_RGB8: packed [hs][pitch] rows of 3-byte pixels, row bytes
 * 3 ws, with bgr) and codd_ingest_frames (the eight raw formats; bgr ignored) in one entry whose source frame has a
 * size of its own: the source is hs x ws (the format size rules, pitch and codd_frame_bytes apply to hs, ws), the
 * rectified image h x w, the padded output H x W.  Each tap position comes from the map function above, evaluated in
 * registers.  THE CONTRACT: each output is, bit for bit, the bilinear blend of codd_ingest_pair / codd_ingest_frames
 * taken at the (sx, sy) codd_rectify_maps writes for the same struct: a tap outside the hs x ws source contributes 0, the
 * blend is fp32 and unrounded, then (c - mean) / std, and the border is the BORDER_REFLECT_101 padding of the RECTIFIED
 * image.  A view whose struct is NULL takes the map-free path (then hs, ws must equal h, w).
 * CODD_EINVAL before any launch: a NULL image, output, mean or stdv; both structs NULL; an unknown fmt, for a YUV format
 * a yuv outside 0..2, an unknown model; a violated format size rule on hs, ws; pitch neither 0 nor >= the row's bytes;
 * h or w <= 0 or a violated h <= H < 2h, w <= W < 2w; a struct with a non-finite entry or with f', fx or fy not
 * positive; a NULL struct with (hs, ws) != (h, w). */
enum { CODD_FMT_RGB8 = 0 }; /* this entry only: not one of the raw formats codd_ingest_frames / codd_frame_bytes take */
#define CODD_CALIB_BROWN 0
#define CODD_CALIB_FISHEYE 1
typedef struct codd_calib_view {
  double R[9];
  double f, cx, cy;
  double K[4];
  double dist[8];
  int model;
} codd_calib_view;
int codd_rectify_maps(const codd_calib_view* left, const codd_calib_view* right, int h, int w, float* lmap_x,
                      float* lmap_y, float* rmap_x, float* rmap_y, void* stream);
int codd_ingest_calibrated(const unsigned char* left, const unsigned char* right, int fmt, int bgr, int yuv, int hs,
                           int ws, long long pitch, const codd_calib_view* lcal, const codd_calib_view* rcal, int h,
                           int w, const float* mean, const float* stdv, int H, int W, float* out_left,
                           float* out_right, void* stream);

/* Live-session export: the frame's padded disparity [1,1,H,W] -> the cropped h x w result, contiguous, in a
 * caller-owned device staging buffer (model/codd.py:370-377: `calib / pred_disp` under reciprocal, then the
 * [:img_h, :img_w] crop).  mode:
 *   CODD_EXPORT_DISP      fp32 disparity (crop only);
 *   CODD_EXPORT_DEPTH     fp32 depth calib * (1 / disp): torch evaluates `calib / disp` with a Python scalar on top as
 *                         disp.reciprocal() * calib, so these are the bits inference(reciprocal=True) returns;
 *   CODD_EXPORT_DISP_U16  uint16 round-to-nearest-even(disp * 256) clamped to [0, 65535], non-finite -> 0 (the KITTI
 *                         devkit's PNG convention). */
#define CODD_EXPORT_DISP 0
#define CODD_EXPORT_DEPTH 1
#define CODD_EXPORT_DISP_U16 2
int codd_export_depth(const float* disp, int H, int W, int h, int w, int mode, float calib, void* out, void* stream);

/* Live-session motion export: the frame's up-sampled SE3 field T [H,W,7] (outputs["Ts"], batch 1; raft3d.py:268-270)
 * -> per-pixel motion of the cropped h x w image, contiguous fp32 [h,w,C], in a caller-owned device staging buffer;
 * and, in the same launch, the roll of the session's previous-frame depth map.  With X0 = inv_project(depth_prev, x, y,
 * K), X1 = T * X0, a = project(X1), c = project(X0) (projective_ops.py:55-68 induced_flow; PEPS and MIN_DEPTH as there),
 * mode:
 *   CODD_MOTION_FLOW2D     C = 2: (a.x - c.x, a.y - c.y), optical flow in pixels;
 *   CODD_MOTION_FLOW_DD    C = 3: the two above and bf * (a.z - c.z), the disparity change in pixels (the `est.z * bf`
 *                          of the scene-flow metrics, model/codd.py:519-575);
 *   CODD_MOTION_SCENEFLOW  C = 3: scale * (X1 - X0), the 3-D displacement; depth is in RAFT3D's normalised units
 *                          (bf / disp), so scale = calib / bf gives the unit of calib = fx * baseline.
 * The vectors live on the PREVIOUS frame's pixel grid and point to the current frame.  A pixel is valid iff
 * X0.z >= MIN_DEPTH && X1.z >= MIN_DEPTH (false for NaN); an invalid pixel gets NaN in every channel.
 * Roll: after reading depth_prev[y,x] ([H,W], read inside the crop only) the same lane overwrites it with
 * clip(bf / (disp_cur[y,x] + 1e-5), 0, 210), the bits of codd_disp_to_depth (motion.py:154-165): the next frame finds this
 * frame's depth there.  Elements outside the crop are neither read nor written.
 * T == NULL: the frame has no field (first frame of a sequence): only the roll runs and out may be NULL.
 * K = (fx, fy, cx, cy) at full resolution.  No pointer needs more than float alignment: spans that do not start or end
 * on a 16-byte boundary take scalar heads and tails and give the same bits.
 * CODD_EINVAL: disp_cur or depth_prev NULL; T without out; h > H or w > W; a non-positive size; an unknown mode; bf not
 * > 0. */
#define CODD_MOTION_FLOW2D 0
#define CODD_MOTION_FLOW_DD 1
#define CODD_MOTION_SCENEFLOW 2
int codd_export_motion(const float* T, const float* disp_cur, float* depth_prev, int H, int W, int h, int w, int mode,
                       float fx, float fy, float cx, float cy, float bf, float scale, float* out, void* stream);

/* Live-session ego-motion: the camera's rigid motion G between the previous and the current frame, fitted to the
 * frame's up-sampled SE3 field T [H,W,7] (outputs["Ts"], batch 1; raft3d.py:268-270) over the cropped h x w image, and
 * the pixels that moved on their own.  The reference has no such output; this replaces the robust rigid fit a user of
 * that field writes with torch (dozens of launches over every pixel and a host sync for the 6x6 solve per iteration).
 * Per crop pixel X0 = inv_project(depth_prev, x, y, K), X1 = T * X0 (projective_ops.py:25-41, :55-68; PEPS and MIN_DEPTH
 * as there); it is valid iff X0.z >= MIN_DEPTH && X1.z >= MIN_DEPTH and all six coordinates are finite.
 * G maps static points from the previous camera frame to the current one (G^-1 is the camera's own motion).  It is found
 * by `iters` Gauss-Newton / IRLS steps from identity over the valid pixels: Y = G_k X0, r = Y - X1, e^2 = |r|^2 / Z0^2,
 * delta = delta_px / fx; weight 1 / Z0^2 in step 0 and 1 / (Z0^2 (1 + e^2 / delta^2)) (Cauchy) afterwards;
 * H = sum w J^T J, g = sum w J^T r with J = [I | -[Y]x] in se3_exp's (tau, phi) order; xi = -H^-1 g by Cholesky;
 * G_{k+1} = se3_exp(xi) * G_k, quaternion renormalised, rounded to fp32.  Per-pixel terms are fp32, sums and the solve
 * fp64, every sum in a fixed order: equal inputs give equal bits.  The fit stops with ok = 0 at the last good iterate
 * (identity if none) when fewer than min_valid pixels are valid, a Cholesky pivot (the diagonal entry before its square
 * root) is <= 1e-12 * trace(H), or a sum is not finite.
 * Outputs, all caller-owned: record, 16 fp32: [0:3] scale * t, [3:7] q_xyzw, [7] ok, [8] valid pixels, [9] inliers
 * (e <= delta under the final G), [10] sqrt(mean e^2 over the inliers) * fx (pixels; 0 without inliers), [11] steps taken,
 * [12:16] zero -- never NaN; moving [h,w] bytes: 0 static, 1 where the residual flow |project(X1).xy - project(G X0).xy|
 * exceeds tau_px, 255 invalid; residual [h,w] fp32 (may be NULL): that magnitude in pixels, NaN where invalid.
 * depth_prev [H,W] is read inside the crop only and not written (codd_export_motion rolls it; call this first).
 * scratch: codd_ego_motion_scratch(h, w) bytes (-1 for a non-positive size), contents irrelevant, any alignment.
 * No pointer needs more than float alignment (moving: none).  iters + 1 launches, no host synchronisation.
 * CODD_EINVAL, before any launch: T, depth_prev, scratch, record or moving NULL; a non-positive size, h > H or w > W;
 * iters outside [1, 32]; fx, fy, delta_px or tau_px not > 0; scratch_bytes below the size function's answer. */
long long codd_ego_motion_scratch(int h, int w);
int codd_ego_motion(const float* T, const float* depth_prev, int H, int W, int h, int w, float fx, float fy, float cx,
                    float cy, float scale, int iters, float delta_px, float tau_px, int min_valid, void* scratch,
                    long long scratch_bytes, float* record, unsigned char* moving, float* residual, void* stream);

/* Live-session stereo confidence: which pixels of the frame's disparity to trust.  The reference has no such output (its
 * evaluation masks come from ground truth); this replaces the scatter-max per row, the gathers and the dozen element-wise
 * launches a user writes with torch.  One launch, no allocation, no host synchronisation.
 * disp [H,W]: the frame's padded disparity; left / right fp32 [3,H,W]: the normalised images exactly as codd_ingest_pair /
 * codd_preprocess wrote them, given together or not at all; stdv: HOST pointer to the 3 stds of that normalisation (RGB
 * order), required iff the images are given.  All are read inside the h x w crop only.  Outputs, caller-owned: flags
 * [h,w] bytes, contiguous, any alignment; residual fp32 [h,w], float alignment, may be NULL and must be NULL without
 * images.  Nothing outside the crop is read or written.
 * Per crop pixel (y, x), d = disp[y,x], every operation below one fp32 operation:
 *   INVALID (128)     d is not finite or not > 0: flags = 128, residual NaN, the pixel takes no further part;
 *   OUT_OF_VIEW (1)   u = (float)x - d is < 0: flags = 1, residual NaN, the pixel is not splatted;
 *   splat             f = (int)floorf(u); the pixel offers d to columns f and f + 1 (each only if < w) of its row's
 *                     right-view z-buffer; zbuf[c] is the largest d offered to column c;
 *   OCCLUDED (2)      r = (int)floorf(u + 0.5f) (f or f + 1, never w); set iff zbuf[r] > d + occ_px (a pixel never
 *                     occludes itself: zbuf[r] >= d);
 *   residual          with images, for every pixel neither invalid nor out of view (occluded ones too): a = u - (float)f,
 *                     x1 = min(f + 1, w - 1), per channel c: Rv = right[c,y,f] * (1 - a) + right[c,y,x1] * a,
 *                     e_c = |left[c,y,x] - Rv| * stdv[c]; residual = ((e_0 + e_1) + e_2) * (1/3): grey levels of the 8-bit
 *                     source; no operation is fused;
 *   MISMATCH (4)      residual > tau (false for NaN; never set without images).
 * The flags OR together (6: occluded and mismatched).  Equal inputs give equal bytes: the z-buffer is an integer
 * maximum over the floats' bits, which does not depend on arrival order.
 * A workgroup owns a row and keeps its z-buffer and disparities in LDS, 8 bytes per pixel: w <= CODD_CONF_MAX_W = 8192
 * (64 KiB), CODD_EUNSUPPORTED beyond it.
 * CODD_EINVAL, before any launch: disp or flags NULL; one image without the other; images without stdv; residual
 * without images; a non-positive size, h > H or w > W; occ_px negative or NaN; tau NaN. */
#define CODD_CONF_OUT_OF_VIEW 1
#define CODD_CONF_OCCLUDED 2
#define CODD_CONF_MISMATCH 4
#define CODD_CONF_INVALID 128
#define CODD_CONF_MAX_W 8192
int codd_export_confidence(const float* disp, const float* left, const float* right, int H, int W, int h, int w,
                           const float* stdv, float occ_px, float tau, unsigned char* flags, float* residual,
                           void* stream);

/* Live-session rectification health check (codd_amd/live.py, epipolar=): the row offset at which the right image really
 * matches the left one, per measured pixel, and a robust fit of that vertical-disparity map by a small rotation of the
 * right view plus a focal ratio.  The reference has no such output; this replaces downloading the disparity and both
 * images every frame and block matching on the host.  2 + iters launches (grey planes, measure, iters - 1 weighted passes,
 * the statistics pass), no allocation, no host synchronisation.
 * disp, left, right, stdv: as for codd_export_confidence (images and stdv required), read inside the h x w crop only.
 * K = (fx, fy, cx, cy) of the rectified camera.  Every operation below is one fp32 operation rounded on its own (no
 * fused multiply-add; division correctly rounded) unless it says fp64; x, y are the pixel's integer coordinates as floats.
 *   grey     gL[y,x] = ((l0 * s0 + l1 * s1) + l2 * s2) * (1.f / 3.f), l_c = left[c,y,x], s_c = stdv[c]; gR likewise: grey
 *            levels of the 8-bit source up to a constant that cancels in every difference.
 *   measure  a pixel is measured iff x % step == 0 && y % step == 0 (step in 1 .. 8).  RX = 4, RY = 1, V = range_px in
 *            1 .. 4.  d = disp[y,x]; u = x - d; f = floorf(u); a = u - f; b = 1.f - a.  The pixel is NOT MEASURABLE when d is
 *            not finite or not > 0, or a tap leaves the crop: x - RX < 0, x + RX >= w, f - RX < 0, f + RX + 1 >= w,
 *            y - RY - V < 0 or y + RY + V >= h.  Otherwise, for v = -V .. V,
 *              R(r,i) = gR[y+r, f+i] * b + gR[y+r, f+i+1] * a                           (r = -RY-V .. RY+V, i = -RX .. RX)
 *              row(v,j) = (..((|gL[y+j,x-RX] - R(j+v,-RX)| + |gL[y+j,x-RX+1] - R(j+v,-RX+1)|) + ..) + |gL[y+j,x+RX] - R(j+v,RX)|
 *              C(v) = (row(v,-1) + row(v,0)) + row(v,1)
 *            v* = the arg-min of C, ties to the smaller |v|, then to the smaller v (a C(v) that is NaN is never chosen
 *            against C(0));  cm = C(v*-1), c0 = C(v*), cp = C(v*+1);  den = (cm - 2.f * c0) + cp.  Also NOT MEASURABLE: |v*| == V;
 *            !(den > 27.f * min_curv) or !(den > 0) (no vertical texture);  !(c0 <= 27.f * tau) (a wrong match).
 *            dy = (float)v* + (cm - cp) / (2.f * den):  L(x, y) ~ R(x - d, y + dy).
 *   dy_map   fp32 [h,w], float alignment, may be NULL (the map then lives in the scratch): dy at measurable pixels, NaN at
 *            every other pixel of the crop, measured or not.
 *   model    xr = (u - cx) / fx;  yn = (y - cy) / fy;  p0 = fy * (1.f + yn * yn);  p1 = fy * (xr * yn);  p2 = fy * xr;
 *            p3 = fy * yn;  e = dy - (((c0 * p0 + c1 * p1) + c2 * p2) + c3 * p3) with the fp64 coefficients rounded to fp32:
 *            dy_model = fy (c0 (1 + yn^2) + c1 xr yn + c2 xr + c3 yn) is, to first order, a rotation of the right view by
 *            (wx, wy, wz) = (-c0, c1, c2) radians, and c3 the relative focal error of the right view.
 *   fit      c = 0; `iters` (1 .. 32) steps, each over the measurable pixels: wt = 1 in step 0 and 1.f / (1.f + (e * e) /
 *            (delta_px * delta_px)) afterwards (Cauchy), e under the previous c;  q_i = wt * p_i;  A_ij = sum (double)(q_i *
 *            p_j) (i <= j), b_i = sum (double)(q_i * dy), n = the number of measurable pixels: sums fp64 in a fixed order,
 *            the products fp32;  c = A^-1 b by a 4x4 Cholesky in fp64.  Equal inputs give equal bits.  The fit stops with ok =
 *            0 at the last good iterate (zeros if none) when n < min_valid, a Cholesky pivot (the diagonal entry before its
 *            square root) is <= 1e-12 * trace(A), or a sum or a coefficient is not finite.
 *   record   32 doubles, never NaN or infinite: [0:4] c, [4] ok, [5] n, [6] inliers (|e| <= delta_px under the final c),
 *            [7] sqrt(sum (double)(dy * dy) / n) (0 for n = 0), [8] sqrt(sum (double)(e * e) over the inliers / inliers) (0
 *            without inliers), [9] steps taken, [10:20] A of the last step (the sums the final c was solved from, or would
 *            have been had the fit not stopped), upper triangle row by row, [20:24] its b -- an entry that is not finite is
 *            written as 0 --, [24:32] zero.
 * scratch: codd_epipolar_scratch(h, w) bytes (-1 for a non-positive size or h w >= 2^31), contents irrelevant, any
 * alignment: the partial sums, both grey planes and the map (12 bytes per crop pixel).  The planes are read from global
 * memory through the caches: no limit on w.
 * CODD_EINVAL, before any launch: disp, left, right, stdv, scratch or record NULL; a non-positive size, h > H, w > W or
 * h w >= 2^31; range_px outside [1, 4], step outside [1, 8], iters outside [1, 32]; fx, fy or delta_px not > 0; tau or
 * min_curv NaN; scratch_bytes below the size function's answer. */
long long codd_epipolar_scratch(int h, int w);
int codd_epipolar_check(const float* disp, const float* left, const float* right, int H, int W, int h, int w,
                        const float* stdv, float fx, float fy, float cx, float cy, int range_px, int step, float tau,
                        float min_curv, int iters, float delta_px, int min_valid, void* scratch, long long scratch_bytes,
                        double* record, float* dy_map, void* stream);

/* Live-session depth on another camera's grid (codd_amd/live.py, align_to=): the frame's disparity, which lives on the
 * rectified virtual left camera, forward-warped into a calibrated target camera -- a physical camera of the rig or a
 * separate colour camera -- with occlusions resolved to the nearest surface.  The reference has no such output; this
 * replaces the z-buffered forward warp a user writes on the host.  Two launches (a fill and the splat), no allocation,
 * no host synchronisation.
 * disp [H,W]: the frame's padded disparity, read inside [0,h) x [0,w) only; f, cx, cy: the rectified camera (f' = fx' =
 * fy'); calib = f' * baseline.  depth_out fp32 [ht,wt] and uv_out fp32 [h,w,2] (may be NULL) are caller-owned and
 * contiguous; neither needs more than float alignment.
 * The target is a codd_align_view, all doubles except model: R (row-major) and T, X_t = R X_rect + T with T in the unit
 * of calib / f'; K = (fx, fy, cx, cy), dist and model, the target camera, with the meaning they have in codd_calib_view;
 * r2_max: a point whose normalised radius^2 in the target exceeds it is not projected (a Brown polynomial folds back
 * outside its field of view and would land far-off points inside the image).  The entry rounds R, T, K, dist and r2_max
 * ONCE to fp32.
 * Per source pixel (u, v), in this fp32 operation order (fma = one fused multiply-add, every other operation rounded to
 * nearest on its own; u, v the pixel's integer coordinates as floats; division and sqrt correctly rounded):
 *   d = disp[v,u];  !(0 < d < +inf)  ->  skipped                                            (false for NaN)
 *   Z = (1 / d) * calib                                         (the bits codd_export_depth's CODD_EXPORT_DEPTH gives)
 *   X = ((u - cx) / f) * Z;  Y = ((v - cy) / f) * Z
 *   Xt = fma(R0, X, fma(R1, Y, fma(R2, Z, T0)));  Yt = fma(R3, X, fma(R4, Y, fma(R5, Z, T1)))
 *   Zt = fma(R6, X, fma(R7, Y, fma(R8, Z, T2)));  !(0 < Zt < +inf)  ->  skipped
 *   x = Xt / Zt;  y = Yt / Zt;  r2 = fma(y, y, x * x);  !(r2 <= r2_max)  ->  skipped
 *   (sx, sy): THE MAP FUNCTION above from its line `xx = x * x` on (the target's lens and K);  sx or sy not finite -> skipped
 * uv_out[v,u] = (sx, sy), or NaN in both for a skipped pixel -- written whether or not the position lies inside the target.
 * footprint k in 1 .. CODD_ALIGN_MAX_FOOTPRINT: a pixel that was not skipped offers Zt to the k target columns nearest
 * to sx, odd k: rint(sx) - (k-1)/2 .. rint(sx) + (k-1)/2 (rint: ties to even), even k: floor(sx) - (k/2 - 1) .. floor(sx) +
 * k/2, and likewise to the k rows nearest to sy; those inside [0,ht) x [0,wt) take min(current, Zt).  A target pixel that
 * nothing reached holds +inf (what CODD_EXPORT_DEPTH gives for zero disparity).  k = 1 leaves lines of holes where the map
 * magnifies; k > 1 closes them and widens every foreground edge by up to k - 1 pixels.
 * Equal inputs give equal bytes: the minimum is a 32-bit integer atomic minimum over the bits of Zt (positive floats
 * order like their bit patterns, +inf above them all), which does not depend on arrival order.
 * CODD_EINVAL, before any launch: disp, view or depth_out NULL; a non-positive size, h > H or w > W; h w or ht wt >= 2^31;
 * f or calib not positive and finite, cx or cy not finite; an unknown model; a non-finite entry in the struct; fx, fy or
 * r2_max not > 0 (as doubles or once rounded to fp32); footprint outside 1 .. CODD_ALIGN_MAX_FOOTPRINT. */
#define CODD_ALIGN_MAX_FOOTPRINT 4
typedef struct codd_align_view {
  double R[9];
  double T[3];
  double K[4];
  double dist[8];
  double r2_max;
  int model;
} codd_align_view;
int codd_align_depth(const float* disp, int H, int W, int h, int w, float f, float cx, float cy, float calib,
                     const codd_align_view* view, int ht, int wt, int footprint, float* depth_out, float* uv_out,
                     void* stream);

/* Live-session ground plane (codd_amd/live.py, ground=): a robust fit of ONE plane to the frame's disparity, per pixel the
 * height above it and a label, and a top-down grid of the floor and obstacle pixels in a frame that lies on the plane.  The
 * reference has no such output; this replaces downloading the depth map every frame and a plane fit, a classification and
 * a histogram on the host.  iters + 1 launches (iters weighted passes over the fit pixels -- the first also clears the grid
 * -- and one pass over the whole crop), no allocation, no host synchronisation, no float atomics.
 * disp [H,W]: the frame's padded disparity, read inside [0,h) x [0,w) only.  K = (fx, fy, cx, cy) of the rectified camera,
 * calib = fx * baseline.  A pixel is VALID iff d = disp[y,x] is finite and > 0.
 * The plane.  A 3-D plane N.X = calib, with X = Z ((x - cx) / fx, (y - cy) / fy, 1) and Z = calib / d, is  d = N.X d / calib =
 * c0 (x - cx) + c1 (y - cy) + c2  with  N = (c0 fx, c1 fy, c2): in disparity space it is a plane too, and the noise of the fit
 * is that of the measured quantity.  The camera sits at X = 0, at the distance Hc = calib / |N| from the plane; n = -N / |N|
 * is the unit normal from the floor towards the camera; a point's height above the plane is n.X + Hc = Hc (1 - c.p / d) =
 * Hc e / d with e the pixel's disparity residual.  An obstacle standing on the floor is nearer than the floor behind it:
 * e > 0, and the floor is the LOWER envelope of the disparities.
 * Every operation below is one fp32 operation rounded on its own (no fused multiply-add; division correctly rounded)
 * unless it says fp64; x, y are the pixel's integer coordinates as floats.
 *   terms    p0 = x - cx;  p1 = y - cy;  (p2 = 1);  e = d - ((c0 * p0 + c1 * p1) + c2) with the fp64 coefficients rounded to
 *            fp32.
 *   fit      over the FIT PIXELS: valid, x % step == 0 && y % step == 0 (step in 1 .. 8).  `iters` (1 .. 32) steps k = 0 ..
 *            iters - 1, each under the previous c.  The scale anneals: s_k = max(delta_px, delta0_px * 0.5^k) (the product is
 *            exact); s = e > 0 ? s_k / asym : s_k;  wt = 1.f / (1.f + (e * e) / (s * s)): an asymmetric Cauchy weight, asym >= 1
 *            (1: symmetric).  Step 0 takes e under `seed` (HOST, 3 doubles) when it is given; with seed NULL step 0 uses
 *            wt = 1 for y >= cy and wt = 0 above (the lower half of the image), and every later step is as above.
 *            q0 = wt * p0, q1 = wt * p1;  A = sum of (double) of (q0 * p0, q0 * p1, q0, q1 * p1, q1, wt) (upper triangle row by
 *            row), b = sum of (double) of (q0 * d, q1 * d, wt * d), n = the number of fit pixels (whatever their weight):
 *            sums fp64 in a fixed order, the products fp32;  c = A^-1 b by a 3x3 Cholesky in fp64.  Equal inputs give equal
 *            bits.  The fit stops with ok = 0 at the last good iterate (zeros if none: the seed is no iterate) when n <
 *            min_valid, a Cholesky pivot (the diagonal entry before its square root) is <= 1e-12 * trace(A), or a sum or
 *            a coefficient is not finite.
 *   metric   fp64, from the final c, fx, fy, calib as doubles of the floats passed: N = (c0 fx, c1 fy, c2);  |N| = sqrt((N0 N0 +
 *            N1 N1) + N2 N2);  Hc = calib / |N|;  n = -N / |N|;  tilt = acos(clamp((n0 u0 + n1 u1) + n2 u2, -1, 1)) in degrees,
 *            u = `up` (HOST, 3 floats; the entry normalises it in fp64; image y points down, so a level camera has
 *            up = (0, -1, 0));  g = z - (z.n) n = (-n2 n0, -n2 n1, 1 - n2 n2);  forward f = g / |g|;  right r = f x n.
 *            ok = 0 as well when |N| is 0 or not finite or Hc is not finite (n, Hc, tilt, f stay 0); tilt > max_tilt_deg;
 *            |g| < 1e-3 (the camera looks along the normal: no forward axis, f stays 0); or the inliers -- fit pixels with
 *            |e| <= delta_px under the final c -- number fewer than min_valid.
 *   pixel    over the WHOLE crop.  labels [h,w] bytes, any alignment; height fp32 [h,w], float alignment, may be NULL.
 *            hgt = ((float)Hc * e) / d.  CODD_GROUND_INVALID: not valid (height NaN).  Otherwise, in this order:
 *            CODD_GROUND_FLOOR iff |e| <= tol_px || |hgt| <= ground_tol;  CODD_GROUND_OVERHEAD iff hgt > clearance;
 *            CODD_GROUND_OBSTACLE iff hgt > 0 (above the floor band, at most clearance);  CODD_GROUND_BELOW otherwise.
 *            height = hgt, in the unit of calib / fx.  With ok = 0 every label is CODD_GROUND_INVALID, every height NaN and
 *            the grid zero.
 *   grid     optional (gh = gw = 0 and both pointers NULL: off).  Floor and obstacle pixels only:  Z = calib / d;  X0 = Z *
 *            (p0 / fx);  X1 = Z * (p1 / fy);  gx = (r0 * X0 + r1 * X1) + r2 * Z;  gz = (f0 * X0 + f1 * X1) + f2 * Z with r, f, Hc
 *            rounded to fp32;  ix = floorf(gx / cell + 0.5f * (float)gw);  iz = floorf(gz / cell);  a pixel outside [0, gw) x
 *            [0, gh) (compared as floats; NaN is outside) is dropped.  The camera stands above the middle of row iz = 0;
 *            iz grows forward, ix to the right.  grid_count int32 [2,gh,gw]: [0,iz,ix] floor pixels, [1,iz,ix] obstacle
 *            pixels;  grid_height fp32 [gh,gw]: the largest hgt of the cell's obstacle pixels, 0 without one.  Counts
 *            are integer atomic adds and the maximum an integer maximum over the bits of a positive float: equal inputs
 *            give equal bytes.  The entry clears the grid on every call: nothing accumulates.
 *   record   32 doubles, never NaN or infinite (an entry that is not finite is written as 0): [0:3] c, [3] ok, [4] fit pixels,
 *            [5] inliers, [6] sqrt(sum (double)(e * e) over the inliers / inliers) (0 without inliers), [7] steps taken,
 *            [8:11] n, [11] Hc, [12] tilt in degrees, [13:19] A of the last step (the sums the final c was solved from, or
 *            would have been had the fit not stopped), upper triangle row by row, [19:22] its b, [22:25] f, [25:32] zero.
 * scratch: codd_ground_scratch(h, w, gh, gw) bytes (-1 for a non-positive h or w, h w >= 2^31, a negative gh or gw, one of
 * them 0 without the other, or gh gw >= 2^30), contents irrelevant, any alignment: the partial sums and the ticket.
 * CODD_EINVAL, before any launch: disp, up, scratch, record or labels NULL; one grid pointer without the other; grid
 * pointers without gh, gw > 0 and a finite cell > 0, or gh, gw != 0 without them; a non-positive size, h > H, w > W or
 * h w >= 2^31; step outside [1, 8], iters outside [1, 32]; fx, fy, calib, delta_px or delta0_px not finite and > 0; cx or cy
 * not finite; asym not finite and >= 1, or (delta_px / asym)^2 not > 0; max_tilt_deg, tol_px or ground_tol negative or
 * NaN; clearance < ground_tol or NaN; cell NaN; up zero or not finite; a seed that is not finite; scratch_bytes below the
 * size function's answer. */
#define CODD_GROUND_FLOOR 0
#define CODD_GROUND_OBSTACLE 1
#define CODD_GROUND_OVERHEAD 2
#define CODD_GROUND_BELOW 3
#define CODD_GROUND_INVALID 255
long long codd_ground_scratch(int h, int w, int gh, int gw);
int codd_ground_plane(const float* disp, int H, int W, int h, int w, float fx, float fy, float cx, float cy, float calib,
                      const double* seed, const float* up, int step, int iters, float delta_px, float delta0_px, float asym,
                      int min_valid, float max_tilt_deg, float tol_px, float ground_tol, float clearance, float cell, int gh,
                      int gw, void* scratch, long long scratch_bytes, double* record, unsigned char* labels, float* height,
                      int* grid_count, float* grid_height, void* stream);

/* Live-session obstacle objects (codd_amd/live.py, objects=): the connected components of the pixels codd_ground_plane
 * labelled, and per component a row of a fixed-size table.  The reference has no such output; this replaces downloading
 * the label map and the disparity every frame and a connected-components pass on the host.  7 launches (6 with ids NULL;
 * one fewer when the crop lies inside one 16 x 64 tile: the shape decides, never the data), no allocation, no host
 * synchronisation, no loop on the host, integer atomics only: equal inputs give equal bytes.
 * disp [H,W]: the padded disparity, read inside [0,h) x [0,w) only; K = (fx, fy, cx, cy), calib as codd_ground_plane took
 * them.  labels [h,w]: the bytes codd_ground_plane wrote.  ground_record: the DEVICE pointer to the 32 doubles it wrote,
 * read on the device: c = [0:3], ok = [3], n = [8:11], Hc = [11], f = [22:25].
 * Every operation below is one fp32 operation rounded on its own (no fused multiply-add; division correctly rounded)
 * unless it says fp64; x, y are the pixel's integer coordinates as floats.
 *   foreground  labels[y,x] < 32 && ((select >> labels[y,x]) & 1) && d = disp[y,x] finite and > 0.  select is a bit set
 *               over the label values (1u << CODD_GROUND_OBSTACLE: the obstacles).
 *   edges       4-connectivity.  Neighbours a, b are joined iff both are foreground and
 *               fabsf(da - db) <= fmaxf(gap_px, gap_rel * fminf(da, db)).
 *   components  the connected components of that graph; a component's KEY is the smallest raster index y * w + x of its
 *               pixels: a function of the input alone, whatever order the merges arrive in.
 *   per pixel   p0 = x - cx;  p1 = y - cy;  e = d - ((c0 * p0 + c1 * p1) + c2);  hgt = ((float)Hc * e) / d  (the bits of
 *               codd_ground_plane's height);  Z = calib / d;  X0 = Z * (p0 / fx);  X1 = Z * (p1 / fy);  gx = (r0 * X0 + r1 *
 *               X1) + r2 * Z;  gz = (f0 * X0 + f1 * X1) + f2 * Z  (the ground grid's frame: gx to the right, gz forward, the
 *               camera above the origin) with c, Hc, f, r rounded to fp32;  r = f x n in fp64 from the record's f and n,
 *               r0 = f1 n2 - f2 n1, r1 = f2 n0 - f0 n2, r2 = f0 n1 - f1 n0, each product and each difference rounded on its
 *               own, then rounded to fp32.  codd_ground_plane forms its r by the same expressions from the same doubles but
 *               does not forbid the compiler a fused multiply-subtract there, so its fp64 r may differ in the last bit
 *               and, where that bit decides the rounding, its fp32 r by one ulp: the two frames agree to one fp32 ulp of
 *               r, not bit for bit.  hgt involves no r: it has the bits of codd_ground_plane's height map.
 *   statistics  per component: pixels (the count); the inclusive box x0, y0, x1, y1; the NEAREST pixel: the largest d,
 *               ties to the smallest raster index (one 64-bit maximum over (bits(d) << 32) | ~index); the minimum and
 *               the maximum of d, hgt, gx and gz, each taken over the order-preserving integer image of the float
 *               (o(v) = ~bits(v) with the sign bit set, bits(v) | 0x80000000 without, compared unsigned): -0 lies below
 *               +0, and a NaN -- possible only where the plane's terms overflow -- orders by its bits (above +inf
 *               with a clear sign bit, below -inf with a set one).
 *   selection   a component PASSES iff pixels >= min_pixels && hgt_max >= min_height (false for a NaN).  Passing
 *               components are numbered in ascending key order; the first max_objects (1 .. 4096) of them are the
 *               objects 0 .. n - 1.
 *   outputs     caller-owned device buffers.  count int32 [4]: n, the number of passing components (> n: the list was
 *               truncated), the number of components, the number of foreground pixels.  obj_i int32 [max_objects,8]:
 *               (pixels, x0, y0, x1, y1, near_x, near_y, key).  obj_f fp32 [max_objects,8]: (gx_min, gx_max, gz_min,
 *               gz_max, hgt_min, hgt_max, d_min, d_max).  Rows >= n of both tables are zero: the entry clears them on
 *               every call.  ids uint16 [h,w], 2-byte aligned, may be NULL: the object number of every pixel, 0xFFFF
 *               where the pixel is not foreground or its component did not become an object.  With ok = 0 in the
 *               record (no floor) nothing is foreground whatever labels holds: count = 0, zero tables, every id 0xFFFF.
 * scratch: codd_objects_scratch(h, w, max_objects) bytes (-1 for a non-positive h or w, h w >= 2^31 or max_objects outside
 * [1, 4096]), contents irrelevant, any alignment: the chunk counts of the numbering, the parent array (int32 per pixel) and
 * the per-root statistics (16 int32 per pixel, touched at the roots only).
 * CODD_EINVAL, before any launch: disp, labels, ground_record, scratch, count, obj_i or obj_f NULL; a non-positive size,
 * h > H, w > W or h w >= 2^31; max_objects outside [1, 4096]; select 0; fx, fy, calib or gap_px not finite and > 0; cx or
 * cy not finite; gap_rel negative or NaN; min_pixels < 1; min_height NaN; scratch_bytes below the size function's answer. */
long long codd_objects_scratch(int h, int w, int max_objects);
int codd_objects(const float* disp, int H, int W, int h, int w, float fx, float fy, float cx, float cy, float calib,
                 const unsigned char* labels, const double* ground_record, unsigned select, float gap_px, float gap_rel,
                 int min_pixels, float min_height, int max_objects, void* scratch, long long scratch_bytes, int* count,
                 int* obj_i, float* obj_f, unsigned short* ids, void* stream);

/* Live-session object tracks (codd_amd/live.py, tracks=): persistent track ids for the objects of codd_objects across
 * frames, and per object the mean 3-D displacement of its pixels under the frame's SE3 field.  The reference has no such
 * output; this replaces downloading both id maps and a flow map every frame, warping one id map onto the other on the
 * host and counting overlaps with np.add.at.  4 launches, no allocation, no host synchronisation, no launch count or grid
 * that depends on the data, integer atomics only: equal inputs give equal bytes.
 * T [H,W,7] and depth_prev [H,W] as codd_ego_motion takes them, read inside the h x w crop only; depth_prev is not written
 * (codd_export_motion rolls it; call this first).  T == NULL: the frame has no field; nothing is associated, every
 * current object starts a track and the ids keep counting.  K = (fx, fy, cx, cy) at full resolution; scale as
 * codd_ego_motion's.  ids_cur uint16 [h,w] and count int32 [4]: the DEVICE outputs of this frame's codd_objects;
 * n_cur = min(count[0], max_objects) (a negative count[0] counts as 0).  ego_record (may be NULL): the DEVICE pointer to
 * the 16 fp32 of codd_ego_motion.  moving [h,w] (may be NULL): its mask.
 * state: caller-owned, persistent between calls, codd_track_state_bytes(h, w, max_objects) bytes of any alignment.  Its
 * layout starts at the first 16-byte boundary at or after the pointer (pass the same pointer every call):
 *   int32 hdr[8] = (n_prev, next_id, frames, 0, 0, 0, 0, 0);
 *   int32 [max_objects,2] = (track, age) of the previous frame's objects, rows >= n_prev zero;
 *   uint16 [h w], the previous frame's id map.
 * fresh != 0: the state's contents are irrelevant; n_prev = 0, next_id = 1, frames = 0.  Otherwise n_prev is hdr[0] clamped
 * to [0, max_objects].
 * Every operation below is one fp32 operation rounded on its own (no fused multiply-add; division correctly rounded)
 * unless it says fp64.
 *   per pixel   p = (x, y) of the crop, on the PREVIOUS frame's grid: a = state.ids[p]; the pixel is skipped if a == 0xFFFF
 *               or a >= n_prev.  X0 = inv_project(depth_prev[y,x], x, y, K); X1 = se3_act(T[y,x], X0) (qrot, then + t);
 *               c = project(X1): the expressions of codd_amd/csrc/se3.h in the order written there (PEPS and MIN_DEPTH as
 *               in projective_ops.py:7-8).  The pixel is VALID iff X0.z >= MIN_DEPTH && X1.z >= MIN_DEPTH and all six
 *               coordinates are finite (codd_ego_motion's rule); an invalid pixel adds nothing and does not vote.
 *   landing     u = floorf(c.x + 0.5f); v = floorf(c.y + 0.5f).  A valid pixel LANDS iff 0 <= u < w && 0 <= v < h, compared
 *               as floats (false for NaN); then b = ids_cur[v,u] and the pixel VOTES for (a, b) iff b < n_cur.
 *   motion      D_k = scale * (X1.k - X0.k), k = x, y, z.  If ego_record != NULL && ego_record[7] != 0: Y = qrot(q =
 *               ego_record[3:7], X0) and O_k = scale * (X1.k - Y.k) - ego_record[k], what is left after the camera's motion.
 *               Q(v) = llrint((double)fminf(fmaxf(v, -4096.f), 4096.f) * 262144.0) (ties to even; fmaxf and fminf return
 *               the other operand for a NaN, which therefore quantises as -4096).  Sums of at most 2^31 such values fit an
 *               int64.
 *   sums        per previous object a, over its valid pixels, in integers: V[a][b] the votes; n_a the valid pixels;
 *               S_a[3] = sum Q(D); So_a[3] = sum Q(O) and no_a their number, accumulated only with a good ego record;
 *               mv_a the valid pixels with moving[p] == 1 (0 without moving).
 *   association best_cur(a): the b with the largest V[a][b] > 0, ties to the smallest b; best_prev(b): the a with the
 *               largest V[a][b] > 0, ties to the smallest a.  Object b CONTINUES a iff best_prev(b) == a && best_cur(a)
 *               == b && V[a][b] >= min_votes: after a split or a merge the id stays with the larger part.  A continued
 *               object keeps a's track id with age + 1; every other object STARTS a track: starting objects take
 *               next_id, next_id + 1, .. in ascending b, with age 1.  If next_id > 2^31 - 1 - max_objects (or < 1) at
 *               the start of a call it restarts at 1; track id 0 is never given.
 *   outputs     caller-owned device buffers; rows >= n_cur are zero, cleared on every call.  trk_count int32 [4]: (n_cur,
 *               continued, started, ended); ended = n_prev - continued, the previous objects that nothing continues.
 *               trk_i int32 [max_objects,8]: (track, age, prev, votes, pixels, moving, own_pixels, 0) = (.., a, V[a][b],
 *               n_a, mv_a, no_a, 0); a started track has prev = -1 and zeros in columns 3 to 6.  trk_f fp32
 *               [max_objects,8]: (Dx, Dy, Dz, Ox, Oy, Oz, 0, 0) with D = (float)(((double)S_a / (double)n_a) / 262144.0)
 *               and O likewise over no_a (fp64 divisions, one rounding to fp32); D is NaN for a started track or n_a ==
 *               0, O for a started track or no_a == 0 (which covers a call without a good ego record).
 *   roll        the state becomes: hdr = (n_cur, next_id + started, frames + 1, 0..); the (track, age) table of the
 *               current objects, rows >= n_cur zero; ids_cur copied into the id map (by the lane that read the old
 *               element, in the per-pixel launch).
 * scratch: codd_track_scratch(h, w, max_objects) bytes, contents irrelevant, any alignment: the vote matrix
 * (max_objects^2 int32, 4 MB at the limit), the per-object sums and the row and column maxima.  Both size functions
 * return -1 for a non-positive h or w, h w >= 2^31 or max_objects outside [1, CODD_TRACK_MAX_OBJECTS].  No pointer needs
 * more than its element's alignment.
 * CODD_EINVAL, before any launch: ids_cur, count, state, scratch, trk_count, trk_i or trk_f NULL; T without depth_prev; a
 * non-positive size, h > H, w > W or h w >= 2^31; max_objects outside [1, 1024]; min_votes < 1; fx, fy or scale not finite
 * and > 0; cx or cy not finite; state_bytes or scratch_bytes below its size function's answer. */
#define CODD_TRACK_MAX_OBJECTS 1024
long long codd_track_state_bytes(int h, int w, int max_objects);
long long codd_track_scratch(int h, int w, int max_objects);
int codd_track_objects(const float* T, const float* depth_prev, int H, int W, int h, int w, float fx, float fy, float cx,
                       float cy, float scale, const unsigned short* ids_cur, const int* count, const float* ego_record,
                       const unsigned char* moving, int min_votes, int max_objects, int fresh, void* state,
                       long long state_bytes, void* scratch, long long scratch_bytes, int* trk_count, int* trk_i,
                       float* trk_f, void* stream);

/* Live-session range scan (codd_amd/live.py, scan=): for every bearing in front of the camera, how far away the first
 * obstacle is and how far the floor was seen before it -- a planar laser scan in the frame of codd_objects' extents.  The
 * reference has no such output; this replaces downloading the label map and the disparity every frame, projecting every
 * pixel into the ground frame on the host, atan2 and np.minimum.at.  3 launches, no allocation, no host synchronisation, no
 * launch count or grid that depends on the data, integer atomics only: equal inputs give equal bytes.
 * disp [H,W], K = (fx, fy, cx, cy), calib, labels [h,w] and ground_record (DEVICE, read on the device) exactly as
 * codd_objects takes them.  ids uint16 [h,w] (may be NULL): the id map codd_objects wrote.  edges: DEVICE fp32 [beams+1,2] =
 * (s_i, c_i) = (sin a_i, cos a_i) of the beam edges' angles, measured from the grid's forward axis (gz), positive to the
 * right (gx), ascending with -pi/2 <= a_0 < a_beams <= pi/2; the entry does not check the table.
 * Every operation below is one fp32 operation rounded on its own (no fused multiply-add; sqrtf and division correctly
 * rounded) unless it says fp64.
 *   per pixel   over the h x w crop.  A pixel TAKES PART iff record[3] != 0 && labels[y,x] < 32 && d = disp[y,x] is finite
 *               and > 0 and it is a FLOOR pixel (labels[y,x] == CODD_GROUND_FLOOR) or an OBSTACLE pixel ((select >>
 *               labels[y,x]) & 1; select is codd_objects' bit set and must not contain the floor).  gx, gz: the expressions
 *               of codd_objects' "per pixel" paragraph, verbatim (r = f x n in fp64, each product and each difference
 *               rounded on its own, then rounded to fp32): the scan lives in the frame of obj_f's extents bit for bit.  The
 *               pixel is dropped unless gz > 0 (false for NaN).  rho = sqrtf((gx * gx) + (gz * gz)); dropped unless rho >=
 *               range_min && rho < range_max.  bin_w = range_max / (float)bins;  k = (int)floorf(rho / bin_w), k == bins
 *               becomes bins - 1.  side(i) = (c_i * gx) - (s_i * gz) for i = 0 .. beams; cnt = the number of edges with
 *               side(i) >= 0; the pixel is dropped when cnt == 0 || cnt == beams + 1, otherwise its beam is cnt - 1.  (For a
 *               table as above and gz > 0 the signs do not increase with i, so the entry finds cnt by bisection.)
 *   tables      [beam][k], in the scratch, cleared on every call: O the obstacle pixels, F the floor pixels (int32 sums);
 *               N the minimum over the obstacle pixels of ((uint64)bits(rho) << 32) | (y * w + x): the nearest pixel, ties to
 *               the smallest raster index (rho > 0: its bits order as it does).
 *   per beam    kh = the smallest k with O[k] >= min_pixels: the HIT bin (nearer bins with fewer pixels do not stop the
 *               beam); limit = kh, or bins without a hit; kf = the largest k < limit with F[k] >= min_pixels; free =
 *               (float)(kf + 1) * bin_w, or 0 without one; floor = the sum of F[k] over k < limit.
 *   outputs     caller-owned device buffers, every row rewritten on every call.  scan_f fp32 [beams,4], scan_i int32
 *               [beams,4]:  a HIT beam: (rho of N[kh], free, gx, gz) and (index of N[kh], object, O[kh], floor), gx and gz
 *               recomputed from the hit pixel by the expressions above, object = ids[index], or -1 when ids == NULL or the
 *               value is 0xFFFF;  no hit and free > 0, a CLEAR beam (clear as far as the floor was seen): (+inf, free, 0,
 *               0) and (-1, -1, 0, floor);  neither, an UNKNOWN beam: (NaN with the bits 0x7fc00000, 0, 0, 0) and (-1, -1, 0,
 *               floor).  scan_count int32 [4]: (hit beams, clear beams, unknown beams, the sum of all O).  With record[3]
 *               == 0 every beam is unknown and scan_count = (0, 0, beams, 0).
 * scratch: codd_range_scan_scratch(beams, bins) bytes (-1 for beams outside [1, 2048], bins outside [1, 1024] or beams bins
 * > 2^20), 16 per (beam, bin) plus the alignment, contents irrelevant, any alignment.  No pointer needs more than its
 * element's alignment.
 * CODD_EINVAL, before any launch: disp, labels, ground_record, edges, scratch, scan_count, scan_i or scan_f NULL; a
 * non-positive size, h > H, w > W or h w >= 2^31; beams, bins outside the limits above; fx, fy, calib or range_max not
 * finite and > 0; cx or cy not finite; range_min negative, NaN or >= range_max; select 0 or with the bit of
 * CODD_GROUND_FLOOR; min_pixels < 1; scratch_bytes below the size function's answer. */
long long codd_range_scan_scratch(int beams, int bins);
int codd_range_scan(const float* disp, int H, int W, int h, int w, float fx, float fy, float cx, float cy, float calib,
                    const unsigned char* labels, const double* ground_record, const unsigned short* ids,
                    const float* edges, int beams, int bins, float range_min, float range_max, unsigned select,
                    int min_pixels, void* scratch, long long scratch_bytes, int* scan_count, int* scan_i, float* scan_f,
                    void* stream);

/* Live-session local map (codd_amd/live.py, localmap=): a rolling occupancy map with integer log-odds in a fixed
 * floor-aligned frame that follows the camera.  codd_ground_plane and codd_range_scan describe one frame; this entry joins
 * the frames: codd_ego_motion's record says how the camera moved, codd_ground_plane's record and labels where the floor is
 * and which pixels stand on it.  The reference has no such output; this replaces downloading the labels and the disparity
 * every frame, composing the poses on the host and rasterising every pixel there.  4 launches, no allocation, no host
 * synchronisation, no launch count or grid that depends on the data, integer atomics only: equal inputs (the state and
 * the map among them) give equal bytes.
 * disp [H,W], K = (fx, fy, cx, cy), calib, labels [h,w] and ground_record (DEVICE, read on the device) exactly as
 * codd_objects takes them.  ego_record: the DEVICE pointer to the 16 fp32 of this frame's codd_ego_motion (t = [0:3] in the
 * unit of calib, q_xyzw = [3:7], ok = [7]; G: X_cur = R(q) X_prev + t), or NULL for a frame without a field.  fresh != 0:
 * the first frame of a sequence.
 * The map frame is the floor frame of the first integrated frame: the origin under the camera, z along that frame's f, x
 * along r = f x n.  The axes stay: the grid never rotates and is never resampled.  The window has gw x gh cells of `cell`
 * units and moves by whole cells.
 * Caller-owned, persistent, DEVICE (zero them once; afterwards only this entry writes them):
 *   logodds int16 [gh,gw], age uint8 [gh,gw]: toroidal storage, world cell (ix, iz) lives at row iz mod gh, column ix mod gw
 *     (the mathematical modulo, also for negatives).  age 255: never observed inside the current window; otherwise the
 *     number of frames since the last observation, saturating at 254.
 *   state, 32 doubles: [0] EXISTS (a pose, a map and a stored floor frame exist); [1:3] (px, pz), the camera's foot point
 *     in the map; [3:5] (hx, hz), the unit heading: the camera's floor-forward axis in the map, its floor-right axis being
 *     (hz, -hx); [5:7] (ix0, iz0), the window origin: out[0,0]'s world cell; [7] frames since the last reset; [8] restarts;
 *     [9:12] n, [12] Hc, [13:16] f: the last floor frame in the last camera's coordinates; and what launch 1 leaves for the
 *     later ones: [16:18] the window origin before this call; [18] CLEARED (this call reset the map); [19] INTEGRATED;
 *     [20] LINKED; [21:23] (dx, dz); [23:32] zero.
 * Launch 1, the pose: fp64 throughout, the operations in the order written, none fused.
 *   cur = ground_record[3] != 0: the current floor frame (n_c, Hc_c, f_c) = record [8:11], [11], [22:25].
 *   The step is tried iff EXISTS && ego_record != NULL && !fresh && ego_record[7] != 0:  q / sqrt(((qx qx + qy qy) + qz qz) +
 *   qw qw) (the step fails unless that root is finite and > 0);  R00 = 1 - 2 (qy qy + qz qz), R01 = 2 (qx qy - qz qw), R02 = 2
 *   (qx qz + qy qw), R10 = 2 (qx qy + qz qw), R11 = 1 - 2 (qx qx + qz qz), R12 = 2 (qy qz - qx qw), R20 = 2 (qx qz - qy qw), R21 =
 *   2 (qy qz + qx qw), R22 = 1 - 2 (qx qx + qy qy);  every 3-term sum below is (a + b) + c.  Without a current floor the
 *   stored one is carried through G: n_c = R n_p;  Hc_c = Hc_p - n_c.t;  g = (-n2 n0, -n2 n1, 1 - n2 n2);  f_c = g / |g| (the
 *   step fails unless |g| >= 1e-3).  r_p = f_p x n_p (codd_objects' expressions);  c = -(R^T t);  dx = r_p.c;  dz = f_p.c;
 *   v = R^T f_c;  a = r_p.v;  b = f_p.v;  m = sqrt(a a + b b) (the step fails unless m >= 1e-6);
 *   p' = ((px + dx hz) + dz hx, (pz - dx hx) + dz hz);  u = ((a hz + b hx) / m, (b hz - a hx) / m);  h' = u / sqrt(ux ux + uz uz);
 *   the step fails unless |p'x / cell| and |p'z / cell| are < 2^30 and |u| is finite and > 0.  Only each frame's own floor
 *   normal levels the step: roll and pitch errors do not accumulate.  No trigonometric function is used.
 *   A step that succeeded: LINKED = 1, the pose advances, the stored floor frame becomes (n_c, Hc_c, f_c), frames += 1,
 *   INTEGRATED = cur.  Otherwise the frame is LOST (LINKED = 0, dx = dz = 0):
 *     lost == CODD_MAP_HOLD && EXISTS && !fresh: pose and map stay as if the camera stood still; the stored floor frame
 *       becomes the current one when there is one; frames += 1; INTEGRATED = cur.
 *     otherwise a reset: CLEARED = 1, p = (0, 0), h = (0, 1), frames = 0, restarts += 1 if EXISTS || fresh; with a current
 *       floor EXISTS = 1, the stored floor frame is the current one and INTEGRATED = 1; without one EXISTS = 0, the stored
 *       frame is zero and INTEGRATED = 0.
 *   ix0 = floor(px / cell) - gw / 2;  iz0 = floor(pz / cell) - gh / 2  (cell as a double, gw / 2 the integer quotient).
 * Launch 2, cells: every cell of the new window that was not in the old one -- all of them when CLEARED -- gets logodds 0,
 *   age 255.  The per-frame tables O, F (int32 [gh,gw] in the scratch, in the order of the outputs) and the counters are
 *   zeroed.
 * Launch 3, pixels, iff INTEGRATED.  Every operation is one fp32 operation rounded on its own (no fused multiply-add;
 *   sqrtf and division correctly rounded) unless it says fp64.  A pixel of the h x w crop is ELIGIBLE iff labels[y,x] ==
 *   CODD_GROUND_FLOOR (a FLOOR pixel) or labels[y,x] < 32 && (select >> labels[y,x]) & 1 (an OBSTACLE pixel; select is
 *   codd_objects' bit set and must not contain the floor), d = disp[y,x] is finite and > 0, and rho = sqrtf((gx * gx) + (gz *
 *   gz)) >= range_min && rho < range_max, with gx, gz the expressions of codd_objects' "per pixel" paragraph, verbatim (the
 *   bits codd_range_scan uses).  oxf = (float)(px - ix0 cell), ozf = (float)(pz - iz0 cell) (fp64, then rounded once); hxf =
 *   (float)hx, hzf = (float)hz;  wx = (gx * hzf + gz * hxf) + oxf;  wz = (gz * hzf - gx * hxf) + ozf;  jx = floorf(wx / cell);
 *   jz = floorf(wz / cell);  a pixel outside [0, gw) x [0, gh) (compared as floats; NaN is outside) is dropped; an obstacle
 *   pixel adds 1 to O[jz,jx], a floor pixel to F[jz,jx].
 * Launch 4, per window cell (j, i), world cell (ix0 + i, iz0 + j), integers only, in this order:
 *   O >= min_pixels: L = min(L + l_occ, l_max), age = 0;  else F >= min_pixels: L = max(L - l_free, l_min), age = 0;
 *   otherwise age = min(age + 1, 254) unless it is 255, and with decay > 0, L = max(L - decay, 0) for L > 0, min(L + decay, 0)
 *   otherwise.  (A frame that is not INTEGRATED has empty tables: every cell ages and decays.)
 *   map_out int16 [gh,gw], age_out uint8 [gh,gw]: the unrolled map, out[j,i] = world cell (ix0 + i, iz0 + j), every element
 *   rewritten on every call.
 *   record, 16 doubles, never NaN: [0] INTEGRATED, [1] LINKED, [2] restarts, [3] frames, [4:8] px, pz, hx, hz, [8:10] ix0, iz0,
 *   [10] pixels integrated (the sum of O and F), [11] cells with L >= occ_level, [12] cells with L <= free_level, [13] cells
 *   with age 255, [14:16] dx, dz.  The counts are integer atomic sums.
 * scratch: codd_local_map_scratch(gh, gw) bytes (-1 for gh or gw outside [1, 4096] or gh gw > 2^22), 8 per cell plus the
 * counters and the alignment, contents irrelevant, any alignment.  state and record need the alignment of a double,
 * logodds and map_out that of an int16.
 * CODD_EINVAL, before any launch: disp, labels, ground_record, state, logodds, age, scratch, map_out, age_out or record NULL;
 * a non-positive size, h > H, w > W or h w >= 2^31; gh, gw outside the limits above; fx, fy, calib, cell or range_max not
 * finite and > 0; cx or cy not finite; range_min negative, NaN or >= range_max; select with the bit of CODD_GROUND_FLOOR
 * (0 is allowed: only the floor is mapped); min_pixels < 1; l_occ, l_free or decay outside [0, 32767]; l_min outside
 * [-32768, 0]; l_max outside [0, 32767]; lost neither CODD_MAP_RESET nor CODD_MAP_HOLD; scratch_bytes below the size
 * function's answer. */
#define CODD_MAP_RESET 0
#define CODD_MAP_HOLD 1
long long codd_local_map_scratch(int gh, int gw);
int codd_local_map(const float* disp, int H, int W, int h, int w, float fx, float fy, float cx, float cy, float calib,
                   const unsigned char* labels, const double* ground_record, const float* ego_record, int fresh, int gh,
                   int gw, float cell, float range_min, float range_max, unsigned select, int min_pixels, int l_occ,
                   int l_free, int l_min, int l_max, int decay, int occ_level, int free_level, int lost, double* state,
                   short* logodds, unsigned char* age, void* scratch, long long scratch_bytes, short* map_out,
                   unsigned char* age_out, double* record, void* stream);

/* Live-session elevation layer (codd_amd/live.py, heightmap=): how high is it, and do I fit?  A rolling 2.5-D layer
 * registered cell for cell to codd_local_map's window -- the same gh x gw, cell, origin and toroidal addressing --
 * integrated from the same pixels by the same floor-frame expressions and kept across frames: per cell the highest and the
 * lowest surface seen and the lowest thing hanging over it, so that a kerb differs from a wall, a pit is a pit and a beam is
 * remembered after it has left the view.  The reference has no such output; this replaces downloading labels, disparity and
 * the height map every frame and rasterising every pixel on the host.  4 launches, no allocation, no host synchronisation,
 * no launch count or grid that depends on the data, integer atomics only (maxima, minima and sums of integers do not
 * depend on the order): equal inputs (the state and the layers among them) give equal bytes.  The entry computes no pose.
 * PRECONDITION: the entry is called exactly once after every codd_local_map call on `state`, from the first one on, with the
 * gh, gw, cell, range_min, range_max that call was given.  That is what makes "the previous origin" and CLEARED mean the same
 * to both maps.
 * Inputs, all DEVICE, never written: disp [H,W], the crop h, w, K = (fx, fy, cx, cy), calib, labels [h,w] and ground_record
 * exactly as codd_local_map takes them; state: the 32 doubles as codd_local_map left them for this frame, of which [1:7]
 * (pose and origin), [16:18] (the previous origin), [18] CLEARED and [19] INTEGRATED are read.
 * Heights are integers in units of h_res (the unit of calib / fx), above the floor plane fitted in the frame that observed
 * them (codd_ground_plane's height, positive upwards): not a global datum.
 * Caller-owned, persistent, DEVICE, toroidal as logodds (world cell (ix, iz) at row iz mod gh, column ix mod gw):
 *   top, bot int16 [gh,gw]: the highest and the lowest surface; -32768: no surface seen inside the current window;
 *   ceil int16 [gh,gw]: the lowest overhead thing; 32767: none seen;
 *   hage uint8 [gh,gw]: 255: never observed inside the current window; otherwise frames since the last observation,
 *     saturating at 254.
 *   The first codd_local_map call on a zeroed state is always CLEARED (nothing exists yet), and a CLEARED call gives every
 *   cell its sentinels: the caller need not initialise the four layers, their contents before the first call are
 *   irrelevant.
 * Launch 1, enter: every cell of the new window that was not in the old one -- all of them when CLEARED; codd_local_map's
 *   launch-2 rule on state[5:7] and [16:18] -- gets top = bot = -32768, ceil = 32767, hage = 255.  The per-frame tables (int32
 *   [gh,gw] each, in the order of the outputs) are set: Tmax = INT_MIN, Tmin = INT_MAX, Tn = 0, Cmin = INT_MAX, Cn = 0; the
 *   counters are zeroed.
 * Launch 2, pixels, iff INTEGRATED.  Every operation is one fp32 operation rounded on its own (no fused multiply-add; sqrtf
 *   and division correctly rounded).  A pixel of the crop is a SURFACE pixel iff labels[y,x] < 32 && (select >> labels[y,x])
 *   & 1 (select must not contain the bit of CODD_GROUND_OVERHEAD; an unsigned holds no bit >= 32), an OVERHEAD pixel iff
 *   labels[y,x] == CODD_GROUND_OVERHEAD.  Either kind needs d = disp[y,x] finite and > 0 and rho in [range_min, range_max);
 *   rho and the cell (jz, jx) are codd_local_map's launch-3 expressions, verbatim (one header, csrc/map_window.h, holds them
 *   for both).  hgt = ((float)Hc * e) / d with e = d - ((c0 * p0 + c1 * p1) + c2), p0 = (float)x - cx, p1 = (float)y - cy and
 *   (c0, c1, c2, Hc) = (float) of record [0], [1], [2], [11]: the bits of codd_ground_plane's height.  A pixel whose hgt is
 *   not finite is dropped.  q = (int)fminf(fmaxf(rintf(hgt / h_res), -32000.f), 32000.f) (rintf: ties to even).  A surface
 *   pixel does Tmax = max(Tmax, q), Tmin = min(Tmin, q), Tn += 1 at [jz,jx]; an overhead pixel Cmin = min(Cmin, q), Cn += 1.
 * Launch 3, update, per window cell (j, i), world cell (ix0 + i, iz0 + j), integers only, in this order, with
 *   f(v, t) = v + (alpha * (t - v)) / 256, C's division truncating toward zero:
 *   Tn >= min_pixels: top = (top == -32768) ? Tmax : f(top, Tmax); bot = (bot == -32768) ? Tmin : f(bot, Tmin);
 *   Cn >= min_pixels: ceil = (ceil == 32767) ? Cmin : f(ceil, Cmin);
 *   if either held hage = 0, otherwise hage = min(hage + 1, 254) unless it is 255.  (A frame that is not INTEGRATED has empty
 *   tables: every cell ages and keeps its values.)  The dead band of the truncation: a target with |t - v| < 256 / alpha
 *   moves nothing (alpha = 128: one unit), so a stored value rests within ceil(256 / alpha) - 1 units of a constant target.
 *   f is monotone in v and in t and Tmin <= Tmax: bot <= top always.  ceil is never forgotten while the cell stays in the
 *   window.
 *   top_out, bot_out, ceil_out int16 [gh,gw], hage_out uint8 [gh,gw]: the unrolled layers, out[j,i] = world cell (ix0 + i,
 *   iz0 + j), every element rewritten on every call.
 * Launch 4, derive, on the unrolled window; neighbours are window neighbours, cells beyond the window's edge are skipped,
 *   never wrapped.  A cell is KNOWN iff top != -32768 (a cell over which only overhead pixels were seen carries its ceil but
 *   is not known).
 *   step_out uint16 [gh,gw]: max(0, top - the minimum of top over the known ones of the 8 neighbours); 0 for an unknown cell
 *   and for a cell without a known neighbour.
 *   flags_out uint8 [gh,gw]: 255 for an unknown cell, otherwise the bit set CODD_HEIGHT_STEP (1): step > max_step_q;
 *   CODD_HEIGHT_HEADROOM (2): ceil != 32767 && ceil - top < robot_height_q; CODD_HEIGHT_HOLE (4): bot < -max_drop_q.  Of an
 *   edge that is too high the upper cell is the blocked one; it blocks the edge both ways.  The thresholds are integers in
 *   units of h_res; the host quantises them once, (int)rint(v / h_res) in fp64.
 *   record, 16 doubles, never NaN: [0] INTEGRATED, [1] surface pixels used (the sum of Tn), [2] overhead pixels used (the sum
 *   of Cn), [3] cells observed this frame (hage 0), [4] known cells, [5:8] cells with STEP, HEADROOM, HOLE, [8] the largest
 *   top and [9] the smallest bot over the known cells (0 without one), [10:12] ix0, iz0, [12:16] 0.  Counts are integer atomic
 *   sums, extrema integer atomics.
 * scratch: codd_height_map_scratch(gh, gw) bytes (-1 outside codd_local_map's limits), 20 per cell plus the counters and the
 * alignment, contents irrelevant, any alignment.  From the first 16-byte boundary at or after the pointer it holds Tmax, Tmin,
 * Tn, Cmin, Cn, then 16 int32 counters; after a call the tables hold the frame's values.
 * CODD_EINVAL, before any launch (a rejected call writes no byte): any pointer NULL; a non-positive size, h > H, w > W or
 * h w >= 2^31; gh, gw outside the limits; fx, fy, calib, cell, range_max or h_res not finite and > 0; cx or cy not finite;
 * range_min negative, NaN or >= range_max; select with the bit of CODD_GROUND_OVERHEAD; min_pixels < 1; alpha outside [1,
 * 256]; max_step_q, robot_height_q or max_drop_q outside [0, 32000]; scratch_bytes below the size function's answer; top,
 * bot, ceil, top_out, bot_out, ceil_out or step_out not aligned to 2 bytes; ground_record, state or record not to 8. */
#define CODD_HEIGHT_STEP 1
#define CODD_HEIGHT_HEADROOM 2
#define CODD_HEIGHT_HOLE 4
long long codd_height_map_scratch(int gh, int gw);
int codd_height_map(const float* disp, int H, int W, int h, int w, float fx, float fy, float cx, float cy, float calib,
                    const unsigned char* labels, const double* ground_record, const double* state, int gh, int gw,
                    float cell, float range_min, float range_max, float h_res, unsigned select, int min_pixels, int alpha,
                    int max_step_q, int robot_height_q, int max_drop_q, short* top, short* bot, short* ceil,
                    unsigned char* hage, void* scratch, long long scratch_bytes, short* top_out, short* bot_out,
                    short* ceil_out, unsigned char* hage_out, unsigned short* step_out, unsigned char* flags_out,
                    double* record, void* stream);

/* Live-session cost map (codd_amd/live.py, costmap=): what a local planner or a safety monitor makes of the occupancy map
 * first.  Per cell of codd_local_map's unrolled window: the squared distance to the nearest occupied cell, an inflated
 * cost (so that the robot can be treated as a point), whether the robot can reach the cell from where it stands, and
 * whether the known space ends there (a frontier).  The reference has no such output; this replaces a download of the map
 * every frame and a distance transform plus a flood fill on the host.  Everything is an integer and everything below
 * defines the result, not the algorithm: equal inputs give equal bytes.  No allocation, no host synchronisation, no launch
 * count or grid that depends on the data, integer atomics only; every output element is rewritten on every call.
 * Inputs, all DEVICE, never written: map int16 [gh,gw] and age uint8 [gh,gw], the map_out / age_out of codd_local_map
 * ([j,i]: row j, column i); lut uint8 [R R + 2], the cost by squared distance (codd_amd/ops.py cost_lut builds one).  gh, gw
 * within codd_local_map's limits, R in [1, CODD_COST_MAX_R].
 * The class of a cell: OCC iff map >= occ_level; otherwise FREE iff age != 255 && map <= free_level; otherwise UNKNOWN.
 * dist2 int32 [gh,gw]: the minimum of (i - i')^2 + (j - j')^2 over the OCC cells (j', i') of the window (cells outside the
 *   window are no sources) if that minimum is <= R R, else CODD_COST_FAR.
 * nearest int32 [gh,gw], or NULL: the raster index j' gw + i' of an OCC cell that attains dist2, the smallest such index;
 *   -1 where dist2 is CODD_COST_FAR.
 * cost uint8 [gh,gw]: c = lut[dist2 <= R R ? dist2 : R R + 1]; the cost is c, except that an UNKNOWN cell with c <
 *   CODD_COST_INSCRIBED gets CODD_COST_NO_INFO.  With cost_lut's table this is the convention of ROS costmap_2d: 254
 *   lethal (an obstacle), 253 inscribed (the robot's centre there means a collision), 1 .. 252 decaying with the distance,
 *   0 free, 255 no information.
 * Traversable.  A cell is a SEED iff (i - start_i)^2 + (j - start_j)^2 <= seed_r2; a SEED cell is traversable iff it is not
 *   OCC (the robot stands there, and a forward-looking camera never observes the floor under and right around itself:
 *   without the seed disk the start cell is UNKNOWN in every real session and nothing is reachable).  Any other cell is
 *   traversable iff c < CODD_COST_INSCRIBED (c as above, before the NO_INFO substitution) and it is FREE, or UNKNOWN with
 *   through_unknown != 0.
 * reach uint8 [gh,gw]: 0 not reachable; 1 traversable and joined to the start cell (start_j, start_i) by a 4-neighbour path
 *   of traversable cells (the start cell itself when it is traversable); 2 reachable and a FRONTIER: one of its 4-neighbours
 *   inside the window is UNKNOWN and not itself reachable.  If the start cell is OCC nothing is reachable.
 * record, 16 doubles, never NaN; every count is an integer atomic sum: [0] OCC cells, [1] cells with cost 253 or 254, [2]
 *   cells with cost 255, [3] reachable cells (frontiers included), [4] frontier cells, [5] 1 iff the start cell is
 *   traversable, [6] dist2 at the start cell (-1 for CODD_COST_FAR), [7] nearest at the start cell (-1; also when nearest is
 *   NULL), [8] the raster index of the frontier cell nearest to the start cell -- by (i - start_i)^2 + (j - start_j)^2, ties
 *   to the smallest raster index, -1 if there is none: one 64-bit integer atomic minimum of (d2 << 32) | raster --, [9] that
 *   cell's squared distance (-1), [10:16] zero.
 * Five launches (column pass, row pass with the tile-local union-find, tile borders, flatten, reach; four for a window
 * of one tile).
 * scratch: codd_cost_map_scratch(gh, gw, R) bytes (-1 for gh, gw or R outside their limits), 7 per cell plus the counters
 * and the alignment, contents irrelevant, any alignment.  dist2 and nearest need the alignment of an int32, map that of
 * an int16, record that of a double.
 * CODD_EINVAL, before any launch: map, age, lut, scratch, dist2, cost, reach or record NULL (nearest may be); gh, gw outside
 * the limits; R outside [1, CODD_COST_MAX_R]; free_level >= occ_level; start_i outside [0, gw) or start_j outside [0, gh);
 * seed_r2 < 0; scratch_bytes below the size function's answer. */
#define CODD_COST_LETHAL 254
#define CODD_COST_INSCRIBED 253
#define CODD_COST_NO_INFO 255
#define CODD_COST_FAR 0x7fffffff
#define CODD_COST_MAX_R 128
long long codd_cost_map_scratch(int gh, int gw, int R);
int codd_cost_map(const short* map, const unsigned char* age, int gh, int gw, int occ_level, int free_level, int R,
                  const unsigned char* lut, int start_i, int start_j, int seed_r2, int through_unknown, void* scratch,
                  long long scratch_bytes, int* dist2, int* nearest, unsigned char* cost, unsigned char* reach,
                  double* record, void* stream);

/* Live-session plan (codd_amd/live.py, plan=): what every user of a cost map computes next.  The navigation function -- the
 * least cost to reach a goal from every cell the robot can reach -- and the path from the robot's cell to the goal, on the
 * cost and reach codd_cost_map left on the device.  The goal is the nearest frontier (exploring), a cell, or a point of the
 * map frame.  The reference has no such output; this replaces a download of cost and reach every frame and Dijkstra on the
 * host.  Everything is an integer and everything below defines the result, not the algorithm: equal inputs give equal
 * bytes.  No allocation, no host synchronisation, one launch of one workgroup whatever the data; every output element is
 * rewritten on every call, inputs are never written.
 * Inputs, DEVICE: cost uint8 [gh,gw] and reach uint8 [gh,gw], the outputs of codd_cost_map ([j,i]: row j, column i);
 * cost_record, its 16 doubles, of which only [8] is read and only in FRONTIER mode (NULL otherwise is fine); map_record, the
 * 16 doubles of codd_local_map, of which only [8:10] = ix0, iz0 are read and only in WORLD mode (NULL otherwise is fine).
 * Host scalars: gh, gw; start_i, start_j, the ones given to codd_cost_map; mode, a CODD_PLAN_GOAL_*; goal_i, goal_j (CELL);
 * goal_x, goal_z and cell (WORLD); goal_r2; neutral in [1, 255], factor in [0, 1024], unknown_cost in [0, 254]; max_path.
 * gh gw <= CODD_PLAN_MAX_CELLS (the default 128 x 128, and 160 x 160: potential and weights of the whole window stay in the
 * 160 KiB of LDS of one gfx950 CU); gh, gw >= 1 is the only limit on a side (a map of codd_local_map has sides of at most 4096).
 * Domain.  D = the cells with reach != 0: by codd_cost_map's definition the 4-connected traversable component of the start
 *   cell, empty when the start cell is not traversable.
 * Weight.  c(q) = unknown_cost if cost[q] == CODD_COST_NO_INFO, else cost[q]; w(q) = neutral + (factor c(q)) / 256 (the
 *   integer quotient), in [1, 1271]; 7 x 1271 x 25600 < 2^32, so a uint32 never overflows.
 * Moves.  The eight neighbours k = 0 .. 7 with (di, dj) = (1,0), (-1,0), (0,1), (0,-1), (1,1), (-1,1), (1,-1), (-1,-1), of
 *   length 5 for k < 4 and 7 otherwise.  A move p -> q is allowed iff p and q are in D and, for a diagonal one, (p.i + di,
 *   p.j) and (p.i, p.j + dj) are in D too: no corner is cut, and every allowed diagonal can be replaced by two allowed
 *   straight moves.
 * Goal cell (gj, gi).  CODD_PLAN_GOAL_CELL: goal_i, goal_j.  CODD_PLAN_GOAL_WORLD: gi = (long long)floor(goal_x /
 *   (double)cell) - (long long)map_record[8], gj likewise from goal_z and [9], each clamped into the window; CLAMPED = 1 iff
 *   either changed (the usual projection of a global goal onto a local window).  CODD_PLAN_GOAL_FRONTIER: r = (long
 *   long)cost_record[8]; no goal cell if r < 0, else (gj, gi) = (r / gw, r % gw).
 * Goal set G = the cells of D with (i - gi)^2 + (j - gj)^2 <= goal_r2.  If that set is empty, a goal cell exists and D is
 *   not empty, G is the single cell of D nearest to the goal cell -- by that squared distance, ties to the smallest raster
 *   index -- and SNAPPED = 1.  Without a goal cell, or with D empty, G is empty.
 * potential uint32 [gh,gw]: P(p) = 0 on G; elsewhere in D, P(p) = the minimum over the allowed moves p -> q of len w(q) +
 *   P(q): the least sum of len w over the cells ENTERED, over all paths of allowed moves from p into G (w >= 1: exactly
 *   one solution; with G not empty it is finite exactly on D); CODD_PLAN_UNREACHED outside D, and everywhere when G is empty.
 * dir uint8 [gh,gw], or NULL: 8 on G; on the other cells with finite P the smallest k whose move is allowed and attains
 *   P(p); 255 elsewhere.
 * path int32 [max_path]: if P at the start cell is finite, the raster index of the start cell, then the cells dir leads
 *   through up to and including the first cell of G; at most max_path entries, -1 behind them.  P decreases strictly along
 *   it, so it has at most gh gw cells.
 * record, 16 doubles, never NaN: [0] FOUND (P at the start cell is finite), [1] P there (-1), [2] the cells of the full
 *   path, also when it was truncated (0), [3] the entries written = min([2], max_path), [4] the goal cell's raster index
 *   after clamping (-1 for none), [5] CLAMPED, [6] SNAPPED, [7] the cells of G, [8] the raster index of the path's last
 *   cell, which is in G (-1), [9] the cells with finite P, [10] the largest finite P (-1 for none), [11] the largest cost byte
 *   other than 255 over the cells of the full path (-1 if not found or no such cell: how close to obstacles the path runs),
 *   [12] the path's length in units of 5 and 7 (the sum of len), [13:16] zero.  Nothing that depends on the algorithm is in
 *   it.
 * scratch: codd_plan_scratch(gh, gw) bytes (-1 for a shape outside the limits): the alignment and a few counters, contents
 * irrelevant, any alignment.  potential and path need the alignment of an int32, the records that of a double.
 * CODD_EINVAL, before any launch: cost, reach, potential, path, record or scratch NULL (dir may be); the record the mode
 * reads NULL; the shape outside the limits; start_i outside [0, gw) or start_j outside [0, gh); an unknown mode; in CELL mode
 * goal_i outside [0, gw) or goal_j outside [0, gh); goal_r2 < 0; max_path < 1; neutral, factor or unknown_cost outside
 * their ranges; in WORLD mode cell, goal_x or goal_z not finite, cell <= 0, or |goal / cell| >= 2^30; scratch_bytes below
 * the size function's answer. */
#define CODD_PLAN_MAX_CELLS 25600
#define CODD_PLAN_UNREACHED 0xffffffffu
#define CODD_PLAN_GOAL_CELL 0
#define CODD_PLAN_GOAL_WORLD 1
#define CODD_PLAN_GOAL_FRONTIER 2
long long codd_plan_scratch(int gh, int gw);
int codd_plan(const unsigned char* cost, const unsigned char* reach, const double* cost_record, const double* map_record,
              int gh, int gw, int start_i, int start_j, int mode, int goal_i, int goal_j, double goal_x, double goal_z,
              float cell, int goal_r2, int neutral, int factor, int unknown_cost, int max_path, void* scratch,
              long long scratch_bytes, unsigned* potential, unsigned char* dir, int* path, double* record, void* stream);

/* Ablation plug-ins.  codd_fusion_select: mode 0 = KalmanFusion (model/fusion/others.py:124-153; constant
 * gain K = Q/(Q+R), the reference never updates P), mode 1 = GTFusion (:54-86; gt [B,1,hg,wg], zero-padded).
 * cur, warp, out: [B,1,H,W]. */
int codd_fusion_select(int mode, const float* cur, const float* warp, const float* gt, int B, int H,
                       int W, int hg, int wg, float K, float* out, void* stream);
/* GTMotion (model/motion/others.py:17-61): nearest warp of the previous image [B,3,H,W], disparity [B,H,W]
 * and features [B,C,H/4,W/4] by the ground-truth flow [B,2,hg,wg] (zero-padded), disparity minus
 * gt_disp_change [B,1,hg,wg], occluded (gt_flow_occ [B,1,hg,wg] bytes != 0) or out-of-image sources -> 0.
 * Outputs = the 5-entry memory: img_warp [B,3,H,W], feat_warp, conf (ones) [B,3,H,W], disp_warp [B,1,H,W],
 * flow3 = [flow, disp change] [B,3,H,W]. */
int codd_gt_motion(const float* img_prev, const float* disp_prev, const float* feat_prev, int C,
                   const float* gt_flow, const float* gt_disp_change, const unsigned char* gt_flow_occ,
                   int B, int H, int W, int hg, int wg, float* img_warp, float* feat_warp, float* conf,
                   float* disp_warp, float* flow3, void* stream);

/* codd_raft_geometry + codd_corr_lookup in one launch (the lookup workgroups project their own pixels; the
 * level-0 workgroups also write xyz [B,h,w,3] and minfo [B,9,h,w]).  Same results as the two separate calls. */
int codd_raft_geometry_lookup(const float* T, const float* depth1, const float* depth2, const float* lvl0,
                              const float* lvl1, const float* lvl2, const float* lvl3, int B, int h, int w,
                              float fx, float fy, float cx, float cy, float* xyz, float* minfo, float* out,
                              void* stream);
/* The same launch writing its two tensor results -- the 9 motion-info channels and the 196 correlation features --
 * directly as split-bf16 records (the inputs of the flow / correlation encoder convolutions); xyz stays fp32. */
int codd_raft_geometry_lookup_xs(const float* T, const float* depth1, const float* depth2, const float* lvl0,
                                 const float* lvl1, const float* lvl2, const float* lvl3, int B, int h, int w,
                                 float fx, float fy, float cx, float cy, float* xyz, codd_xs_view minfo_xs,
                                 codd_xs_view corr_xs, void* stream);

int codd_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CODD_HIP_H */
