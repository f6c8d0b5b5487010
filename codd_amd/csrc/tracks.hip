// codd_track_objects: which object of this frame is which object of the last one, and how did it move?  (codd_amd/live.py,
// tracks=)  Every pixel of a previous object is carried by the frame's SE3 field onto the current frame's id map and votes
// for the object it lands on; mutual best matches with enough votes keep their track id, every other object starts one;
// per previous object the mean 3-D displacement of its pixels, and what is left of it after the camera's own motion.
// The reference has no such output; what this replaces is downloading both id maps and a flow map every frame, a warp on
// the host and np.add.at.  The contract is in include/codd_hip.h.
//
// Four launches on one stream, no allocation, no host synchronisation, integer atomics only:
//   1 clear   the vote matrix and the per-object sums in the scratch;
//   2 vote    one pixel per lane, 16 waves a workgroup: the geometry, the landing, the quantised displacements; a wave
//             whose valid lanes share one previous object -- the common case: 64 consecutive pixels of a row -- reduces
//             in registers, and of the workgroup's waves with that object the first adds all their totals through LDS
//             and issues the nine atomics, one field a lane; votes of waves whose voting lanes share (a, b) go the same
//             way; the lanes of any other wave add for themselves.  Every lane first rolls its own element of the
//             state's id map: nobody else reads it (landings read ids_cur);
//   3 best    a wave per row and a wave per column of the vote matrix: the largest count, ties to the smallest index
//             (one 64-bit maximum over (votes << 32) | ~index);
//   4 assign  one workgroup, a thread per current object: mutual best and min_votes, the started tracks numbered by ballot
//             and popcount in ascending b, both tables, the count, and the state's header and (track, age) table.
// Everything relies on the kernel boundaries; there is no hand-off inside a launch.  The per-object sums are laid out
// field by field ([9][max_objects rounded up to 8] int64), so the nine atomics of one object go to nine different 64-byte
// blocks.  profiles/live_tracks.md has this launch against one atomic per lane and value: 33 us a call against 2.5 ms.
#include "common.h"

#pragma clang fp contract(off)  // every operation of the contract rounds once, se3.h's expressions included
#include "se3.h"

#define TRK_NF 9        // per-object sums: [0] n [1] mv [2] no [3:6] S [6:9] So
#define TRK_VT 1024     // threads of a workgroup of launch 2
#define TRK_VW (TRK_VT / 64)
#define TRK_QSCALE 262144.0
#define TRK_QMAX 4096.f

struct TrkArgs {
  const float* T;
  const float* depth;
  const unsigned short* ids_cur;
  const int* count;
  const float* ego;
  const unsigned char* moving;
  int* hdr;                // state: [8]
  int* table;              //        [m][2]
  unsigned short* sids;    //        [h w]
  int* V;                  // scratch: [m][m]
  unsigned long long* acc; //          [TRK_NF][mp]
  int* best;               //          [2][m]: best_cur of every row, best_prev of every column
  int* trk_count;
  int* trk_i;
  float* trk_f;
  int W, h, w, m, mp, min_votes, fresh;
  long long nclear;        // int32 words of V and acc together
  float fx, fy, cx, cy, scale;
};

__device__ __forceinline__ int trk_n_prev(const TrkArgs& a) { return a.fresh ? 0 : min(max(a.hdr[0], 0), a.m); }
__device__ __forceinline__ int trk_n_cur(const TrkArgs& a) { return min(max(a.count[0], 0), a.m); }

__device__ __forceinline__ bool trk_finite3(V3 v) {
  return fabsf(v.x) < INFINITY && fabsf(v.y) < INFINITY && fabsf(v.z) < INFINITY;  // (false for NaN)
}

// (fmaxf and fminf return the other operand for a NaN: a NaN quantises as -4096)
__device__ __forceinline__ long long trk_q(float v) { return llrint((double)fminf(fmaxf(v, -TRK_QMAX), TRK_QMAX) * TRK_QSCALE); }

__device__ __forceinline__ long long trk_shfl_xor(long long v, int o) {
  const int lo = __shfl_xor((int)(unsigned)(unsigned long long)v, o, 64);
  const int hi = __shfl_xor((int)(unsigned)((unsigned long long)v >> 32), o, 64);
  return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

// ---- 1: clear
__global__ __launch_bounds__(256) void trk_clear_kernel(TrkArgs a) {
  for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < a.nclear; k += (long long)gridDim.x * 256) a.V[k] = 0;
}

// ---- 2: votes and sums, and the roll of the id map
__device__ __forceinline__ void trk_add(const TrkArgs& a, int obj, int field, unsigned long long v) {
  if (v) atomicAdd(a.acc + (size_t)field * a.mp + obj, v);
}

__global__ __launch_bounds__(TRK_VT) void trk_vote_kernel(TrkArgs a) {
  __shared__ int sObj[TRK_VW], sKey[TRK_VW], sVotes[TRK_VW];  // a wave's one object and one vote key, or -1
  __shared__ unsigned long long sAcc[TRK_VW][TRK_NF];
  const long long n = (long long)a.h * a.w, e = (long long)blockIdx.x * TRK_VT + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned pa = 0xFFFFu;
  if (e < n) {
    pa = a.sids[e];
    a.sids[e] = a.ids_cur[e];
  }
  const bool cand = a.T != nullptr && (int)pa < trk_n_prev(a);
  int wobj = -1, wkey = -1, wvotes = 0;
  unsigned long long acc[TRK_NF] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // n, mv, no, Q(D), Q(O) of this lane
  if (__ballot(cand)) {
    const int n_cur = trk_n_cur(a);
    const bool ego_ok = a.ego != nullptr && a.ego[7] != 0.f;
    bool val = false, vote = false;
    int b = 0;
    if (cand) {
      const int y = (int)(e / a.w), x = (int)(e - (long long)y * a.w);
      const size_t p = (size_t)y * a.W + x;
      const V3 X0 = inv_project(a.depth[p], x, y, a.fx, a.fy, a.cx, a.cy);
      const V3 X1 = se3_act(se3_load(a.T + p * 7), X0);
      val = X0.z >= MIN_DEPTH && X1.z >= MIN_DEPTH && trk_finite3(X0) && trk_finite3(X1);
      if (val) {
        const V3 c = project(X1, a.fx, a.fy, a.cx, a.cy);
        const float u = floorf(c.x + 0.5f), v = floorf(c.y + 0.5f);
        if (u >= 0.f && u < (float)a.w && v >= 0.f && v < (float)a.h) {  // (false for NaN)
          b = a.ids_cur[(size_t)(int)v * a.w + (int)u];
          vote = b < n_cur;
        }
        acc[0] = 1ull;
        acc[1] = a.moving != nullptr && a.moving[e] == 1 ? 1ull : 0ull;
        acc[3] = (unsigned long long)trk_q(a.scale * (X1.x - X0.x));
        acc[4] = (unsigned long long)trk_q(a.scale * (X1.y - X0.y));
        acc[5] = (unsigned long long)trk_q(a.scale * (X1.z - X0.z));
        if (ego_ok) {
          const V3 Y = qrot(Q4{a.ego[3], a.ego[4], a.ego[5], a.ego[6]}, X0);
          acc[2] = 1ull;
          acc[6] = (unsigned long long)trk_q(a.scale * (X1.x - Y.x) - a.ego[0]);
          acc[7] = (unsigned long long)trk_q(a.scale * (X1.y - Y.y) - a.ego[1]);
          acc[8] = (unsigned long long)trk_q(a.scale * (X1.z - Y.z) - a.ego[2]);
        }
      }
    }
    // the sums of the previous object: a wave with one object adds its lanes up and leaves the total to the workgroup
    const unsigned long long mval = __ballot(val);
    if (mval) {
      bool own = val;
      const int a0 = __shfl((int)pa, __ffsll((long long)mval) - 1, 64);
      if (__all(!val || (int)pa == a0)) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
          for (int k = 0; k < TRK_NF; ++k) acc[k] += (unsigned long long)trk_shfl_xor((long long)acc[k], o);
        }
        wobj = a0;
        own = false;
      }
      if (own) {
#pragma unroll
        for (int k = 0; k < TRK_NF; ++k) trk_add(a, (int)pa, k, acc[k]);
      }
    }
    // the votes, likewise
    const unsigned long long mvote = __ballot(vote);
    if (mvote) {
      const int key = (int)pa * a.m + b;  // (pa < m and b < m where vote)
      bool own = vote;
      const int key0 = __shfl(key, __ffsll((long long)mvote) - 1, 64);
      if (__all(!vote || key == key0)) {
        wkey = key0;
        wvotes = __popcll(mvote);
        own = false;
      }
      if (own) atomicAdd(a.V + key, 1);
    }
  }
  // the workgroup: of the waves that share an object (a key) the first adds the totals of all of them, one field a lane
  if (lane == 0) {
    sObj[wave] = wobj; sKey[wave] = wkey; sVotes[wave] = wvotes;
#pragma unroll
    for (int k = 0; k < TRK_NF; ++k) sAcc[wave][k] = acc[k];
  }
  __syncthreads();
  if (wobj >= 0 && lane < TRK_NF) {
    bool leader = true;
    for (int k = 0; k < wave; ++k) leader = leader && sObj[k] != wobj;
    if (leader) {
      unsigned long long sum = 0ull;
      for (int k = wave; k < TRK_VW; ++k) sum += sObj[k] == wobj ? sAcc[k][lane] : 0ull;
      trk_add(a, wobj, lane, sum);
    }
  }
  if (wkey >= 0 && lane == TRK_NF) {
    bool leader = true;
    for (int k = 0; k < wave; ++k) leader = leader && sKey[k] != wkey;
    if (leader) {
      int sum = 0;
      for (int k = wave; k < TRK_VW; ++k) sum += sKey[k] == wkey ? sVotes[k] : 0;
      atomicAdd(a.V + wkey, sum);
    }
  }
}

// ---- 3: row and column maxima
__global__ __launch_bounds__(256) void trk_best_kernel(TrkArgs a) {
  const int wv = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (wv >= 2 * a.m) return;
  const int n_prev = trk_n_prev(a), n_cur = trk_n_cur(a);
  const bool row = wv < a.m;
  const int i = row ? wv : wv - a.m;
  const int own = row ? n_prev : n_cur, len = row ? n_cur : n_prev;
  unsigned long long best = 0ull;
  if (i < own) {
    for (int j = lane; j < len; j += 64) {
      const int v = row ? a.V[(size_t)i * a.m + j] : a.V[(size_t)j * a.m + i];
      if (v > 0) {
        const unsigned long long key = ((unsigned long long)(unsigned)v << 32) | (unsigned)~(unsigned)j;
        best = key > best ? key : best;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long ob = (unsigned long long)trk_shfl_xor((long long)best, o);
    best = ob > best ? ob : best;
  }
  if (lane == 0) a.best[wv] = best ? (int)~(unsigned)best : -1;
}

// ---- 4: association, numbering, tables, roll of the header and the (track, age) table
__device__ __forceinline__ float trk_mean(unsigned long long sum, unsigned long long cnt) {
  if (cnt == 0ull) return NAN;
  return (float)(((double)(long long)sum / (double)(long long)cnt) / TRK_QSCALE);
}

__global__ __launch_bounds__(1024) void trk_assign_kernel(TrkArgs a) {
  __shared__ int sStart[16], sCont[16];
  const int b = threadIdx.x, lane = b & 63, wave = b >> 6;
  const int n_prev = trk_n_prev(a), n_cur = trk_n_cur(a);
  int nid = a.fresh ? 1 : a.hdr[1];
  if (nid < 1 || nid > 0x7fffffff - a.m) nid = 1;
  const int frames = a.fresh ? 0 : a.hdr[2];
  int prev = -1, votes = 0;
  if (a.T != nullptr && b < n_cur) {
    const int pa = a.best[a.m + b];
    if (pa >= 0 && pa < n_prev && a.best[pa] == b) {
      const int v = a.V[(size_t)pa * a.m + b];
      if (v >= a.min_votes) { prev = pa; votes = v; }
    }
  }
  const bool cont = prev >= 0, start = b < n_cur && !cont;
  int track = 0, age = 0;
  if (cont) {
    track = a.table[2 * prev];
    age = (int)((unsigned)a.table[2 * prev + 1] + 1u);
  }
  const unsigned long long ms = __ballot(start), mc = __ballot(cont);
  if (lane == 0) { sStart[wave] = __popcll(ms); sCont[wave] = __popcll(mc); }
  __syncthreads();  // (also: every read of the old header and table lies before this barrier, every write behind it)
  int rank = __popcll(ms & ((1ull << lane) - 1ull)), started = 0, continued = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    rank += k < wave ? sStart[k] : 0;
    started += sStart[k];
    continued += sCont[k];
  }
  if (start) { track = nid + rank; age = 1; }
  if (b < a.m) {
    a.table[2 * b] = track;
    a.table[2 * b + 1] = age;
    int* ri = a.trk_i + 8 * b;
    float* rf = a.trk_f + 8 * b;
    int pixels = 0, moving = 0, own = 0;
    float d[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (cont) {
      const unsigned long long* f = a.acc + prev;
      const unsigned long long na = f[0], no = f[2 * (size_t)a.mp];
      pixels = (int)na; moving = (int)f[a.mp]; own = (int)no;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        d[k] = trk_mean(f[(size_t)(3 + k) * a.mp], na);
        d[3 + k] = trk_mean(f[(size_t)(6 + k) * a.mp], no);
      }
    } else if (start) {
#pragma unroll
      for (int k = 0; k < 6; ++k) d[k] = NAN;
    }
    ri[0] = track; ri[1] = age; ri[2] = b < n_cur ? prev : 0; ri[3] = votes; ri[4] = pixels; ri[5] = moving; ri[6] = own; ri[7] = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) rf[k] = d[k];
    rf[6] = 0.f; rf[7] = 0.f;
  }
  if (b == 0) {
    a.hdr[0] = n_cur; a.hdr[1] = nid + started; a.hdr[2] = (int)((unsigned)frames + 1u);
    for (int k = 3; k < 8; ++k) a.hdr[k] = 0;
    a.trk_count[0] = n_cur; a.trk_count[1] = continued; a.trk_count[2] = started; a.trk_count[3] = n_prev - continued;
  }
}

// ---- the state and the scratch: both 16-byte aligned by the call itself
static inline long long trk_v_bytes(long long m) { return (4 * m * m + 63) & ~63LL; }
static inline long long trk_mp(long long m) { return (m + 7) & ~7LL; }
static inline bool trk_shape_ok(int h, int w, int m) {
  return h > 0 && w > 0 && (long long)h * w < (1LL << 31) && m >= 1 && m <= CODD_TRACK_MAX_OBJECTS;
}

extern "C" long long codd_track_state_bytes(int h, int w, int max_objects) {
  if (!trk_shape_ok(h, w, max_objects)) return -1;
  return 16 + 32 + 8LL * max_objects + 2LL * h * w;
}

extern "C" long long codd_track_scratch(int h, int w, int max_objects) {
  if (!trk_shape_ok(h, w, max_objects)) return -1;
  return 16 + trk_v_bytes(max_objects) + 8LL * TRK_NF * trk_mp(max_objects) + 8LL * max_objects;
}

extern "C" int codd_track_objects(const float* T, const float* depth_prev, int H, int W, int h, int w, float fx, float fy,
                                  float cx, float cy, float scale, const unsigned short* ids_cur, const int* count,
                                  const float* ego_record, const unsigned char* moving, int min_votes, int max_objects,
                                  int fresh, void* state, long long state_bytes, void* scratch, long long scratch_bytes,
                                  int* trk_count, int* trk_i, float* trk_f, void* stream) {
  if (!ids_cur || !count || !state || !scratch || !trk_count || !trk_i || !trk_f) return CODD_EINVAL;
  if (T && !depth_prev) return CODD_EINVAL;
  if (H <= 0 || W <= 0 || h > H || w > W || !trk_shape_ok(h, w, max_objects) || min_votes < 1) return CODD_EINVAL;
  if (!(fx > 0.f && fx < INFINITY) || !(fy > 0.f && fy < INFINITY) || !(scale > 0.f && scale < INFINITY)) return CODD_EINVAL;
  if (!(fabsf(cx) < INFINITY) || !(fabsf(cy) < INFINITY)) return CODD_EINVAL;
  if (state_bytes < codd_track_state_bytes(h, w, max_objects)) return CODD_EINVAL;
  if (scratch_bytes < codd_track_scratch(h, w, max_objects)) return CODD_EINVAL;
  const long long n = (long long)h * w, m = max_objects;
  char* sb = (char*)(((uintptr_t)state + 15) & ~(uintptr_t)15);
  char* cb = (char*)(((uintptr_t)scratch + 15) & ~(uintptr_t)15);
  TrkArgs a;
  a.T = T; a.depth = depth_prev; a.ids_cur = ids_cur; a.count = count; a.ego = ego_record; a.moving = moving;
  a.hdr = (int*)sb; a.table = (int*)(sb + 32); a.sids = (unsigned short*)(sb + 32 + 8 * m);
  a.V = (int*)cb;
  a.acc = (unsigned long long*)(cb + trk_v_bytes(m));
  a.best = (int*)(cb + trk_v_bytes(m) + 8LL * TRK_NF * trk_mp(m));
  a.trk_count = trk_count; a.trk_i = trk_i; a.trk_f = trk_f;
  a.W = W; a.h = h; a.w = w; a.m = max_objects; a.mp = (int)trk_mp(m); a.min_votes = min_votes; a.fresh = fresh != 0;
  a.nclear = (trk_v_bytes(m) + 8LL * TRK_NF * trk_mp(m)) / 4;
  a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.scale = scale;
  hipStream_t s = (hipStream_t)stream;
  const long long cw = (a.nclear + 255) / 256;
  trk_clear_kernel<<<(unsigned)(cw < 1024 ? cw : 1024), 256, 0, s>>>(a);
  CODD_LAUNCH_CHECK();
  trk_vote_kernel<<<(unsigned)((n + TRK_VT - 1) / TRK_VT), TRK_VT, 0, s>>>(a);
  CODD_LAUNCH_CHECK();
  trk_best_kernel<<<(unsigned)((2 * m + 3) / 4), 256, 0, s>>>(a);
  CODD_LAUNCH_CHECK();
  trk_assign_kernel<<<1, 1024, 0, s>>>(a);
  CODD_LAUNCH_CHECK();
  return CODD_OK;
}
