// Live-session ingest (codd_amd/live.py): both views of one frame -- packed 8-bit RGB / BGR, mono8, YUYV / UYVY, NV12 or a
// Bayer mosaic -- decoded in integer registers (ingest_decode.h), optionally rectified through a bilinear remap,
// normalised and reflect-padded into fp32 CHW (reference datasets/transforms.py:147-161 Pad, :373-427 Normalize,
// datasets/formating.py:65-85, applied to img and r_img by datasets/custom_stereo_mf.py; the remap is the
// cv2.remap(INTER_LINEAR, BORDER_CONSTANT 0) a user of the reference runs on the host before either).  ONE kernel body
// serves the three entries of include/codd_hip.h: codd_ingest_pair and codd_ingest_frames take the source position of a
// rectified pixel from map arrays, codd_ingest_calibrated evaluates the closed-form map of a stereo calibration (about 25
// numbers per view; THE MAP FUNCTION of the header) in registers instead of streaming two fp32 maps per view (16 B per
// output pixel against 1-3 B of image), and its source frame has a size of its own.  codd_rectify_maps writes that
// function out as map arrays; both kernels call the one calib_map of calib_map.h, whose every operation is pinned (__fmaf_rn and
// friends), as is the blend (blend4), so the entries agree to the bit.  A pure streaming kernel: no LDS, four output
// pixels per thread, 16-byte stores, a scalar tail.
#include "calib_map.h"
#include "ingest_decode.h"

struct MapArgs {
  float* mx[2];
  float* my[2];
  int h, w;
  int mapped[2];
  CalibView cv[2];
};

__global__ __launch_bounds__(256) void rectify_maps_kernel(MapArgs a) {
  const int v = blockIdx.y;
  if (!a.mapped[v]) return;
  const CalibView& cv = a.cv[v];
  float* __restrict__ mx = a.mx[v];
  float* __restrict__ my = a.my[v];
  const int h = a.h, w = a.w;
  const int W4 = (w + FRAME_PX - 1) / FRAME_PX;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)h * W4) return;
  const int y = (int)(t / W4), x4 = (int)(t - (long long)y * W4) * FRAME_PX;
  f32x4 rx, ry;
#pragma unroll
  for (int i = 0; i < FRAME_PX; ++i) {
    float sx, sy;
    calib_map(cv, x4 + i, y, sx, sy);  // (x4 + i >= w in the tail: computed, never stored)
    rx[i] = sx; ry[i] = sy;
  }
  const size_t o = (size_t)y * w + x4;
  if ((w & 3) == 0 && (((uintptr_t)mx | (uintptr_t)my) & 15) == 0) {  // (then x4 + 4 <= w and every row offset is 16-byte aligned)
    *(f32x4*)(mx + o) = rx; *(f32x4*)(my + o) = ry;
  } else {
#pragma unroll
    for (int i = 0; i < FRAME_PX; ++i)
      if (x4 + i < w) { mx[o + i] = rx[i]; my[o + i] = ry[i]; }
  }
}

// ingest_kernel's MAP: where the source position of rectified pixel (y, x) of view v comes from
struct ArrayMaps {  // fp32 arrays of the rectified size; NULL: the view has no map
  const float* mx[2];
  const float* my[2];
  __device__ bool mapped(int v) const { return mx[v] != nullptr; }
  __device__ void at(int v, int rw, int y, int x, float& sx, float& sy) const {
    const size_t o = (size_t)y * rw + x;
    sx = mx[v][o]; sy = my[v][o];
  }
};

struct CalibMaps {  // calib_map in registers; on[v] == 0: the view has no calibration
  int on[2];
  CalibView cv[2];
  __device__ bool mapped(int v) const { return on[v] != 0; }
  __device__ void at(int v, int, int y, int x, float& sx, float& sy) const { calib_map(cv[v], x, y, sx, sy); }
};

template <int FMT, class MAP>
__global__ __launch_bounds__(256) void ingest_kernel(FrameArgs a, MAP m) {
  const int v = blockIdx.y;
  const unsigned char* __restrict__ img = a.img[v];
  float* __restrict__ out = a.out[v];
  const bool mapped = m.mapped(v);
  const int h = a.rh, w = a.rw, H = a.H, W = a.W;
  const int W4 = (W + FRAME_PX - 1) / FRAME_PX;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)H * W4) return;
  const int y = (int)(t / W4), x4 = (int)(t - (long long)y * W4) * FRAME_PX;
  const int sy = y < h ? y : 2 * (h - 1) - y;  // reflect without edge repeat (cv2.BORDER_REFLECT_101), of the RECTIFIED image
  float c[FRAME_PX][3];  // raw (un-normalised) channels in source order
  if (!mapped && x4 + FRAME_PX <= w) {  // map-free interior (the source is the rectified image: a.h, a.w == h, w)
    int ci[FRAME_PX][3];
    frame_px4<FMT>(a, img, sy, x4, ci);
#pragma unroll
    for (int i = 0; i < FRAME_PX; ++i) { c[i][0] = (float)ci[i][0]; c[i][1] = (float)ci[i][1]; c[i][2] = (float)ci[i][2]; }
  } else {
#pragma unroll
    for (int i = 0; i < FRAME_PX; ++i) {
      const int x = x4 + i;
      c[i][0] = c[i][1] = c[i][2] = 0.f;
      if (x < W) {
        const int sx = x < w ? x : 2 * (w - 1) - x;
        if (mapped) {
          float px, py;
          m.at(v, w, sy, sx, px, py);
          frame_blend<FMT>(a, img, px, py, c[i]);
        } else {
          int ci[3];
          frame_px<FMT>(a, img, sy, sx, ci);
          c[i][0] = (float)ci[0]; c[i][1] = (float)ci[1]; c[i][2] = (float)ci[2];
        }
      }
    }
  }
  const size_t N = (size_t)H * W, o = (size_t)y * W + x4;
  const float m0 = a.m0, m1 = a.m1, m2 = a.m2, s0 = a.s0, s1 = a.s1, s2 = a.s2;
  const bool bgr = FMT == CODD_FMT_RGB8 && a.bgr;
  f32x4 r0, r1, r2;
#pragma unroll
  for (int i = 0; i < FRAME_PX; ++i) {
    const float c0 = bgr ? c[i][2] : c[i][0], c1 = c[i][1], c2 = bgr ? c[i][0] : c[i][2];
    r0[i] = (c0 - m0) / s0; r1[i] = (c1 - m1) / s1; r2[i] = (c2 - m2) / s2;  // preprocess_kernel's expression
  }
  if ((W & 3) == 0 && ((uintptr_t)out & 15) == 0) {  // (then x4 + 4 <= W and every row / plane offset is 16-byte aligned)
    *(f32x4*)(out + o) = r0; *(f32x4*)(out + N + o) = r1; *(f32x4*)(out + 2 * N + o) = r2;
  } else {
#pragma unroll
    for (int i = 0; i < FRAME_PX; ++i)
      if (x4 + i < W) { out[o + i] = r0[i]; out[N + o + i] = r1[i]; out[2 * N + o + i] = r2[i]; }
  }
}

extern "C" long long codd_frame_bytes(int fmt, int h, int w, long long pitch) {
  if (fmt < CODD_FMT_MONO8 || fmt > CODD_FMT_BAYER_BGGR || h <= 0 || w <= 0) return -1;
  if ((fmt_is_yuv422(fmt) || fmt == CODD_FMT_NV12) && (w & 1)) return -1;
  if (fmt == CODD_FMT_NV12 && (h & 1)) return -1;
  if (fmt_is_bayer(fmt) && (h < 2 || w < 2)) return -1;
  const long long row = fmt_is_yuv422(fmt) ? 2LL * w : w;
  if (pitch == 0) pitch = row;
  const long long rows = fmt == CODD_FMT_NV12 ? h + h / 2 : h;
  if (pitch < row || pitch > LLONG_MAX / rows) return -1;
  return pitch * rows;
}

// What the three ingest entries share: the checks on pointers, on the source (size, pitch and yuv rules of fmt at
// hs x ws; CODD_FMT_RGB8: codd_frame_bytes' rules with a row of 3 ws bytes) and on the rectified h x w inside H x W, and the
// kernel's arguments.  False: CODD_EINVAL.
static bool frame_args(FrameArgs* a, const unsigned char* left, const unsigned char* right, int fmt, int bgr, int yuv, int hs,
                       int ws, long long pitch, int h, int w, const float* mean, const float* stdv, int H, int W,
                       float* out_left, float* out_right) {
  if (!left || !right || !mean || !stdv || !out_left || !out_right) return false;
  long long bytes;
  if (fmt == CODD_FMT_RGB8) {
    if (hs <= 0 || ws <= 0) return false;
    const long long row = 3LL * ws;
    if (pitch == 0) pitch = row;
    if (pitch < row || pitch > LLONG_MAX / hs) return false;
    bytes = pitch * hs;
  } else {
    bytes = codd_frame_bytes(fmt, hs, ws, pitch);  // -1: an unknown format, a violated size rule, a bad pitch
    if (bytes < 0) return false;
  }
  const bool is_yuv = fmt_is_yuv422(fmt) || fmt == CODD_FMT_NV12;
  if (is_yuv && (yuv < 0 || yuv > 2)) return false;
  if (h <= 0 || w <= 0 || H < h || W < w || H - h >= h || W - w >= w) return false;
  // yoff, then CY, CVR, CUG, CVG, CUB: bt601 and bt709 video range, BT.601 full range (jpeg)
  static const double coef[3][6] = {{16, 1.164, 1.596, 0.391, 0.813, 2.018},
                                    {16, 1.164, 1.793, 0.213, 0.533, 2.112},
                                    {0, 1.000, 1.402, 0.344, 0.714, 1.772}};
  const double* k = coef[is_yuv ? yuv : 0];
  a->img[0] = left; a->img[1] = right;
  a->out[0] = out_left; a->out[1] = out_right;
  a->pitch = bytes / (fmt == CODD_FMT_NV12 ? hs + hs / 2 : hs); a->bytes = bytes;
  a->h = hs; a->w = ws; a->rh = h; a->rw = w; a->H = H; a->W = W;
  a->bgr = bgr != 0;
  a->yoff = (int)k[0];
  a->cy = (int)lrint(k[1] * 1048576.0); a->cvr = (int)lrint(k[2] * 1048576.0); a->cug = (int)lrint(k[3] * 1048576.0);
  a->cvg = (int)lrint(k[4] * 1048576.0); a->cub = (int)lrint(k[5] * 1048576.0);
  a->m0 = mean[0]; a->m1 = mean[1]; a->m2 = mean[2]; a->s0 = stdv[0]; a->s1 = stdv[1]; a->s2 = stdv[2];
  return true;
}

template <class MAP>
static int ingest_launch(int fmt, const FrameArgs& a, const MAP& m, void* stream) {
  const long long threads = (long long)a.H * cdiv(a.W, FRAME_PX);
  const dim3 grid(cdiv(threads, 256), 2);
  switch (fmt) {
#define CODD_INGEST_CASE(F) case F: ingest_kernel<F, MAP><<<grid, 256, 0, (hipStream_t)stream>>>(a, m); break
    CODD_INGEST_CASE(CODD_FMT_RGB8);
    CODD_INGEST_CASE(CODD_FMT_MONO8);
    CODD_INGEST_CASE(CODD_FMT_YUYV);
    CODD_INGEST_CASE(CODD_FMT_UYVY);
    CODD_INGEST_CASE(CODD_FMT_NV12);
    CODD_INGEST_CASE(CODD_FMT_BAYER_RGGB);
    CODD_INGEST_CASE(CODD_FMT_BAYER_GRBG);
    CODD_INGEST_CASE(CODD_FMT_BAYER_GBRG);
    CODD_INGEST_CASE(CODD_FMT_BAYER_BGGR);
#undef CODD_INGEST_CASE
    default: return CODD_EINVAL;
  }
  CODD_LAUNCH_CHECK();
  return CODD_OK;
}

static int ingest_arrays(int fmt, const FrameArgs& a, const float* lmap_x, const float* lmap_y, const float* rmap_x,
                         const float* rmap_y, void* stream) {
  if ((lmap_x == nullptr) != (lmap_y == nullptr) || (rmap_x == nullptr) != (rmap_y == nullptr)) return CODD_EINVAL;
  const ArrayMaps m = {{lmap_x, rmap_x}, {lmap_y, rmap_y}};
  return ingest_launch(fmt, a, m, stream);
}

extern "C" int codd_ingest_pair(const unsigned char* left, const unsigned char* right, int h, int w, int bgr,
                                const float* mean, const float* stdv, const float* lmap_x, const float* lmap_y,
                                const float* rmap_x, const float* rmap_y, int H, int W, float* out_left,
                                float* out_right, void* stream) {
  FrameArgs a;
  if (!frame_args(&a, left, right, CODD_FMT_RGB8, bgr, 0, h, w, 0, h, w, mean, stdv, H, W, out_left, out_right)) return CODD_EINVAL;
  return ingest_arrays(CODD_FMT_RGB8, a, lmap_x, lmap_y, rmap_x, rmap_y, stream);
}

extern "C" int codd_ingest_frames(const unsigned char* left, const unsigned char* right, int fmt, int yuv, int h, int w,
                                  long long pitch, const float* mean, const float* stdv, const float* lmap_x,
                                  const float* lmap_y, const float* rmap_x, const float* rmap_y, int H, int W,
                                  float* out_left, float* out_right, void* stream) {
  FrameArgs a;
  if (fmt == CODD_FMT_RGB8) return CODD_EINVAL;  // (codd_ingest_pair's format)
  if (!frame_args(&a, left, right, fmt, 0, yuv, h, w, pitch, h, w, mean, stdv, H, W, out_left, out_right)) return CODD_EINVAL;
  return ingest_arrays(fmt, a, lmap_x, lmap_y, rmap_x, rmap_y, stream);
}

// the fp32 constants of one view: fp64 on the host, each rounded once.  False: an invalid struct.
static bool calib_constants(const codd_calib_view* s, CalibView* c) {
  if (s->model != CODD_CALIB_BROWN && s->model != CODD_CALIB_FISHEYE) return false;
  const double* all[] = {s->R, &s->f, &s->cx, &s->cy, s->K, s->dist};
  const int counts[] = {9, 1, 1, 1, 4, 8};
  for (int g = 0; g < 6; ++g)
    for (int i = 0; i < counts[g]; ++i)
      if (!isfinite(all[g][i])) return false;
  if (!(s->f > 0.0 && s->K[0] > 0.0 && s->K[1] > 0.0)) return false;
  if (!((float)s->f > 0.f && isfinite((float)s->K[0]) && isfinite((float)s->K[1]))) return false;  // (still so in fp32)
  for (int i = 0; i < 3; ++i) {
    c->m[3 * i] = (float)(s->R[i] / s->f);
    c->m[3 * i + 1] = (float)(s->R[3 + i] / s->f);
    c->m[3 * i + 2] = (float)(s->R[6 + i] - (s->R[i] * s->cx + s->R[3 + i] * s->cy) / s->f);
  }
  c->fx = (float)s->K[0]; c->fy = (float)s->K[1]; c->cx = (float)s->K[2]; c->cy = (float)s->K[3];
  for (int i = 0; i < 8; ++i) c->k[i] = (float)s->dist[i];
  c->model = s->model;
  return true;
}

extern "C" int codd_rectify_maps(const codd_calib_view* left, const codd_calib_view* right, int h, int w, float* lmap_x,
                                 float* lmap_y, float* rmap_x, float* rmap_y, void* stream) {
  if ((!left && !right) || h <= 0 || w <= 0) return CODD_EINVAL;
  if ((left && (!lmap_x || !lmap_y)) || (right && (!rmap_x || !rmap_y))) return CODD_EINVAL;
  MapArgs a = {};
  a.mx[0] = lmap_x; a.my[0] = lmap_y; a.mx[1] = rmap_x; a.my[1] = rmap_y;
  a.h = h; a.w = w;
  const codd_calib_view* views[2] = {left, right};
  for (int v = 0; v < 2; ++v) {
    a.mapped[v] = views[v] != nullptr;
    if (views[v] && !calib_constants(views[v], &a.cv[v])) return CODD_EINVAL;
  }
  const long long threads = (long long)h * cdiv(w, FRAME_PX);
  rectify_maps_kernel<<<dim3(cdiv(threads, 256), 2), 256, 0, (hipStream_t)stream>>>(a);
  CODD_LAUNCH_CHECK();
  return CODD_OK;
}

extern "C" int codd_ingest_calibrated(const unsigned char* left, const unsigned char* right, int fmt, int bgr, int yuv,
                                      int hs, int ws, long long pitch, const codd_calib_view* lcal,
                                      const codd_calib_view* rcal, int h, int w, const float* mean, const float* stdv,
                                      int H, int W, float* out_left, float* out_right, void* stream) {
  FrameArgs a;
  if (!frame_args(&a, left, right, fmt, bgr, yuv, hs, ws, pitch, h, w, mean, stdv, H, W, out_left, out_right)) return CODD_EINVAL;
  if (!lcal && !rcal) return CODD_EINVAL;
  if ((!lcal || !rcal) && (hs != h || ws != w)) return CODD_EINVAL;
  CalibMaps m = {};
  const codd_calib_view* views[2] = {lcal, rcal};
  for (int v = 0; v < 2; ++v) {
    m.on[v] = views[v] != nullptr;
    if (views[v] && !calib_constants(views[v], &m.cv[v])) return CODD_EINVAL;
  }
  return ingest_launch(fmt, a, m, stream);
}
