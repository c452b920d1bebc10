// Streaming tracking (AudioDetector.track_stream): links the boxes decode / NMS leave for a group of windows to the tracks of the
// windows before, on the device, in front of the record append of the same group (stream.hip) - so the stream keeps its one host copy
// at the end of the recording.  A greedy IoU tracker with a constant-velocity alpha-beta model (alpha = 1); the rule is written out in
// DESIGN.md (streaming tracking) and restated in numpy float32 by tests/track_ref.py.
//
// One 256-thread block per call: window w needs the tracks window w-1 left.  Thread t owns slot t of the track table in registers for
// the whole call; the window's detections (the first TRK_DMAX of its cnt[i] rows: nothing behind a count is read) sit in LDS.  Per
// window every live slot finds its best unmatched detection (live slots x detections IoUs), then the greedy step is a block-wide
// arg-max over one 64-bit key per slot, (IoU bits, 0xFFFF - slot, 0xFFFF - detection): the largest IoU wins, ties go to the lowest slot,
// then to the lowest detection, in ONE max reduction (wave shuffles, then the four wave maxima through LDS).  Only the slots whose best
// detection was just taken look again.  Every fp32 operation is rounded on its own (__fadd_rn / __fsub_rn / __fmul_rn / __fdiv_rn, no
// contraction, the idiom of postproc.hip), so the restatement gives the same bits.  No atomics; plain vector stores only.
//
// Offsets: the clamped exclusive scan of cnt[0 .. n_valid-1] on top of *rec_count that det_record_append_kernel does - *rec_count is
// read, never written, so the launch has to precede the append of the same group.
#include "common.h"

#define TRK_BMAX 1024       // windows per call (DR_BMAX of stream.hip)
#define TRK_SMAX 256        // track slots = threads of the block
#define TRK_DMAX 256        // detections of one window that take part
#define TRK_WORDS 16        // 4-byte words per slot in the state buffer (13 used)

struct TrackParams { int max_tracks; int max_age; float iou_min; float beta; float birth_score; };

__device__ __forceinline__ unsigned long long trk_wave_max(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  return v;
}

__global__ __launch_bounds__(256) void track_update_kernel(const float* __restrict__ rows, const int* __restrict__ cnt, int B, int cap_img,
                                                           const int* __restrict__ ctl, const int* __restrict__ rec_count, int rec_cap,
                                                           int* __restrict__ rec_track, int* __restrict__ slots, int* __restrict__ glob,
                                                           TrackParams p) {
  __shared__ long long s_off[TRK_BMAX + 1];     // as det_record_append_kernel: record row of window i's first row
  __shared__ int s_nv;
  __shared__ float s_dx1[TRK_DMAX], s_dy1[TRK_DMAX], s_dx2[TRK_DMAX], s_dy2[TRK_DMAX], s_darea[TRK_DMAX], s_dscore[TRK_DMAX],
      s_dlabel[TRK_DMAX];
  __shared__ int s_dtrack[TRK_DMAX];            // the id detection d's row gets (-1: none)
  __shared__ int s_dused[TRK_DMAX];             // detection d is matched
  __shared__ int s_live[TRK_SMAX];              // slot t is live (for the births)
  __shared__ int s_birth[TRK_SMAX];             // 1 + the detection that is born into slot t (0: none)
  __shared__ unsigned long long s_wmax[4];
  __shared__ int s_next, s_over;
  const int tid = threadIdx.x;
  if (tid == 0) {
    const int nv = max(0, min(ctl[0], B));
    long long o = max(*rec_count, 0);
    for (int i = 0; i < nv; ++i) {
      s_off[i] = o;
      o += max(0, min(cnt[i], cap_img));
    }
    s_off[nv] = o;
    s_nv = nv;
    s_next = glob[0];
    s_over = 0;
  }
  // slot tid in registers
  const bool mine = tid < p.max_tracks;
  int live = 0, id = 0, hits = 0, misses = 0, last = 0;
  float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f, vx = 0.f, vy = 0.f, label = 0.f, score = 0.f;
  if (mine) {
    const int* s = slots + tid * TRK_WORDS;
    live = s[0] != 0;
    if (live) {
      id = s[1];
      x1 = __int_as_float(s[2]); y1 = __int_as_float(s[3]); x2 = __int_as_float(s[4]); y2 = __int_as_float(s[5]);
      vx = __int_as_float(s[6]); vy = __int_as_float(s[7]); label = __int_as_float(s[8]); score = __int_as_float(s[9]);
      hits = s[10]; misses = s[11]; last = s[12];
    }
  }
  __syncthreads();
  const int nv = s_nv, first = ctl[1];

  for (int i = 0; i < nv; ++i) {
    const long long o = s_off[i];
    const int n_all = (int)(s_off[i + 1] - o);          // 0 .. cap_img
    const int n = min(n_all, TRK_DMAX);
    const float* src = rows + (size_t)i * cap_img * 6;
    if (tid < n) {
      const float* r = src + tid * 6;
      const float a = r[0], b = r[1], c = r[2], d = r[3];
      s_dx1[tid] = a; s_dy1[tid] = b; s_dx2[tid] = c; s_dy2[tid] = d;
      s_darea[tid] = __fmul_rn(__fsub_rn(c, a), __fsub_rn(d, b));
      s_dscore[tid] = r[4]; s_dlabel[tid] = r[5];
      s_dtrack[tid] = -1; s_dused[tid] = 0;
    }
    s_birth[tid] = 0;
    if (tid == 0 && n_all > TRK_DMAX) s_over = 1;
    // 1. predict
    float area = 0.f;
    if (live) {
      x1 = __fadd_rn(x1, vx); x2 = __fadd_rn(x2, vx); y1 = __fadd_rn(y1, vy); y2 = __fadd_rn(y2, vy);
      area = __fmul_rn(__fsub_rn(x2, x1), __fsub_rn(y2, y1));
    }
    __syncthreads();

    // 2. this slot's best candidate among the unmatched detections: 0 = none
    auto best = [&]() -> unsigned long long {
      unsigned long long k = 0;
      for (int d = 0; d < n; ++d) {
        if (s_dused[d] || !(s_dlabel[d] == label)) continue;
        const float ww = __fsub_rn(fminf(x2, s_dx2[d]), fmaxf(x1, s_dx1[d]));
        const float hh = __fsub_rn(fminf(y2, s_dy2[d]), fmaxf(y1, s_dy1[d]));
        float iou = 0.f;
        if (!(ww <= 0.f) && !(hh <= 0.f)) {
          const float inter = __fmul_rn(ww, hh);
          const float u = __fsub_rn(__fadd_rn(area, s_darea[d]), inter);
          iou = u > 0.f ? __fdiv_rn(inter, u) : 0.f;
        }
        if (!(iou >= p.iou_min)) continue;                // false for NaN; iou >= +0, and a non-negative float's bits order like the float
        const unsigned long long key = ((unsigned long long)__float_as_uint(iou) << 32) |
                                       ((unsigned long long)(0xFFFFu - (unsigned)tid) << 16) | (unsigned long long)(0xFFFFu - (unsigned)d);
        k = key > k ? key : k;
      }
      return k;
    };
    bool matched = false;
    unsigned long long key = (live && n > 0) ? best() : 0ull;

    // 3. greedy match: the block-wide largest key, until none is left (at most min(live slots, n) rounds)
    for (;;) {
      const unsigned long long wm = trk_wave_max(key);
      if ((tid & 63) == 0) s_wmax[tid >> 6] = wm;
      __syncthreads();
      unsigned long long m = s_wmax[0];
      m = s_wmax[1] > m ? s_wmax[1] : m;
      m = s_wmax[2] > m ? s_wmax[2] : m;
      m = s_wmax[3] > m ? s_wmax[3] : m;
      if (m == 0) break;                                  // uniform: every thread read the same four words
      const int ms = 0xFFFF - (int)((m >> 16) & 0xFFFFu), md = 0xFFFF - (int)(m & 0xFFFFu);
      if (tid == ms) {
        // 4. matched slot: the velocity takes beta of the residual of the centre, the box and the score become the detection's
        const float dx1 = s_dx1[md], dy1 = s_dy1[md], dx2 = s_dx2[md], dy2 = s_dy2[md];
        const float rx = __fsub_rn(__fmul_rn(__fadd_rn(dx1, dx2), 0.5f), __fmul_rn(__fadd_rn(x1, x2), 0.5f));
        const float ry = __fsub_rn(__fmul_rn(__fadd_rn(dy1, dy2), 0.5f), __fmul_rn(__fadd_rn(y1, y2), 0.5f));
        vx = __fadd_rn(vx, __fmul_rn(p.beta, rx));
        vy = __fadd_rn(vy, __fmul_rn(p.beta, ry));
        x1 = dx1; y1 = dy1; x2 = dx2; y2 = dy2; score = s_dscore[md];
        hits += 1; misses = 0; last = first + i;
        matched = true;
        key = 0;
        s_dtrack[md] = id;
        s_dused[md] = 1;
      }
      __syncthreads();                                    // s_dused[md] is visible, and every thread is done with s_wmax
      if (key != 0 && 0xFFFF - (int)(key & 0xFFFFu) == md) key = best();
    }

    // 5. unmatched live slots age; freeing comes before the births
    if (live && !matched) {
      misses += 1;
      if (misses > p.max_age) {
        live = 0; id = 0; hits = 0; misses = 0; last = 0;
        x1 = y1 = x2 = y2 = vx = vy = label = score = 0.f;
      }
    }
    s_live[tid] = mine ? live : 1;                        // slots behind max_tracks are never free
    __syncthreads();
    // 6. births, in detection order, each into the lowest free slot (the free slots are taken in rising order: one pointer)
    if (tid == 0) {
      int t = 0, next = s_next, over = s_over;
      for (int d = 0; d < n; ++d) {
        if (s_dused[d] || !(s_dscore[d] >= p.birth_score)) continue;
        while (t < p.max_tracks && s_live[t]) ++t;
        if (t < p.max_tracks) {
          s_birth[t] = d + 1;
          s_dtrack[d] = next++;
          ++t;
        } else {
          over = 1;
        }
      }
      s_next = next; s_over = over;
    }
    __syncthreads();
    if (mine && s_birth[tid]) {
      const int d = s_birth[tid] - 1;
      live = 1; id = s_dtrack[d];
      x1 = s_dx1[d]; y1 = s_dy1[d]; x2 = s_dx2[d]; y2 = s_dy2[d];
      vx = 0.f; vy = 0.f; label = s_dlabel[d]; score = s_dscore[d];
      hits = 1; misses = 0; last = first + i;
    }
    // 7. the rows' ids: -1 for every row that was neither matched nor born, and for the rows behind TRK_DMAX
    for (int j = tid; j < n_all; j += 256)
      if (o + j < rec_cap) rec_track[o + j] = j < n ? s_dtrack[j] : -1;
    __syncthreads();                                      // the next window overwrites the detections
  }

  if (mine) {
    int* s = slots + tid * TRK_WORDS;
    s[0] = live; s[1] = id;
    s[2] = __float_as_int(x1); s[3] = __float_as_int(y1); s[4] = __float_as_int(x2); s[5] = __float_as_int(y2);
    s[6] = __float_as_int(vx); s[7] = __float_as_int(vy); s[8] = __float_as_int(label); s[9] = __float_as_int(score);
    s[10] = hits; s[11] = misses; s[12] = last;
  }
  if (tid == 0) {
    glob[0] = s_next;
    if (s_over) glob[1] = 1;
  }
}

extern "C" int mmd_track_update(const float* rows, const int* cnt, int B, int cap_img, const int* ctl, const int* rec_count, int rec_cap,
                                int* rec_track, int* trk_slots, int* trk_glob, int max_tracks, float iou_min, float beta, int max_age,
                                float birth_score, hipStream_t stream) {
  if (!rows || !cnt || !ctl || !rec_count || !rec_track || !trk_slots || !trk_glob) return MMD_EINVAL;
  if (B <= 0 || B > TRK_BMAX || cap_img <= 0 || rec_cap <= 0 || (long long)cap_img * 6 > 0x7fffffffLL) return MMD_EINVAL;
  if (max_tracks < 1 || max_tracks > TRK_SMAX || max_age < 0) return MMD_EINVAL;
  TrackParams p;
  p.max_tracks = max_tracks; p.max_age = max_age; p.iou_min = iou_min; p.beta = beta; p.birth_score = birth_score;
  hipLaunchKernelGGL(track_update_kernel, dim3(1), dim3(256), 0, stream, rows, cnt, B, cap_img, ctl, rec_count, rec_cap, rec_track,
                     trk_slots, trk_glob, p);
  return mmd_check_launch();
}
