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
//
// A bank of sessions (mmd_track_update_bank) keeps one such table per session and runs one block per session over the same group: the
// per-window body is ONE __device__ function, trk_window, that both kernels call.
//
// A second association rule, assign = 1 (mmd_track_update_assign / mmd_track_update_bank_assign; TrackConfig(assign="optimal")): steps
// 2 - 3 become the matching of maximum IoU sum.  trk_window takes the rule as a compile-time parameter; the greedy instantiation is the
// code above, the optimal one writes every live slot's predicted box, area and label to LDS, lists the slots and the detections that
// have an allowed pair at all (the optimum lies among them, and in the common case they are few), calls mot_assign<256> (mot_assign.h:
// the solver of the tracking evaluation) with cost = -(double)iou on allowed pairs and 0 elsewhere - transposed when the listed slots
// outnumber the listed detections - drops the pairs that are not allowed, and lets each matched slot apply step 4 to itself.  Ties
// between matchings of equal weight are unspecified.  Its IoU is trk_iou below: the greedy step's expression compiled without
// contraction, so the weights are the bits of tests/track_ref.iou_matrix.  A `false` from mot_assign (impossible for finite costs)
// matches nothing in that window and sets the overflow flag.
//
// Static LDS per block: greedy 19 512 bytes (track_update_kernel) / 23 616 (track_update_bank_kernel); optimal 39 080 / 43 184 - the
// greedy figures plus TrackOptimal, 19 568 bytes: MotAssign<256> (9 304) and the slot table, the match table and the lists (10 KB).
#include "common.h"
#include "mot_assign.h"

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

// The detections of one window and the block's scratch, in LDS
struct TrackShared {
  float dx1[TRK_DMAX], dy1[TRK_DMAX], dx2[TRK_DMAX], dy2[TRK_DMAX], darea[TRK_DMAX], dscore[TRK_DMAX], dlabel[TRK_DMAX];
  int dtrack[TRK_DMAX];            // the id detection d's row gets (-1: none)
  int dused[TRK_DMAX];             // detection d is matched
  int live[TRK_SMAX];              // slot t is live (for the births)
  int birth[TRK_SMAX];             // 1 + the detection that is born into slot t (0: none)
  unsigned long long wmax[4];
  int next, over;                  // the tracker's {next_id, overflow} while the block runs
};

// Slot tid of the track table, in registers for the whole call
struct TrackSlot {
  int live, id, hits, misses, last;
  float x1, y1, x2, y2, vx, vy, label, score;
};

// The association rule of trk_window: what the optimal form keeps in LDS beside TrackShared; the greedy form keeps nothing
#define TRK_GREEDY 0
#define TRK_OPTIMAL 1
struct TrackGreedy {};
struct TrackOptimal {
  float tx1[TRK_SMAX], ty1[TRK_SMAX], tx2[TRK_SMAX], ty2[TRK_SMAX], tarea[TRK_SMAX], tlabel[TRK_SMAX];      // slot t after the predict step
  int tmatch[TRK_SMAX];            // the detection slot t is matched to (-1: none)
  int dany[TRK_DMAX];              // detection d has an allowed pair
  int tlist[TRK_SMAX], dlist[TRK_DMAX];      // the slots / detections with an allowed pair, rising
  int wsum[4];
  MotAssign<TRK_DMAX> as;
};
template <int ASSIGN> struct TrackRule { typedef TrackGreedy Shared; };
template <> struct TrackRule<TRK_OPTIMAL> { typedef TrackOptimal Shared; };

__device__ __forceinline__ void trk_slot_load(TrackSlot& t, const int* __restrict__ slots, int tid, bool mine) {
  t.live = 0; t.id = 0; t.hits = 0; t.misses = 0; t.last = 0;
  t.x1 = t.y1 = t.x2 = t.y2 = t.vx = t.vy = t.label = t.score = 0.f;
  if (mine) {
    const int* s = slots + tid * TRK_WORDS;
    t.live = s[0] != 0;
    if (t.live) {
      t.id = s[1];
      t.x1 = __int_as_float(s[2]); t.y1 = __int_as_float(s[3]); t.x2 = __int_as_float(s[4]); t.y2 = __int_as_float(s[5]);
      t.vx = __int_as_float(s[6]); t.vy = __int_as_float(s[7]); t.label = __int_as_float(s[8]); t.score = __int_as_float(s[9]);
      t.hits = s[10]; t.misses = s[11]; t.last = s[12];
    }
  }
}

__device__ __forceinline__ void trk_slot_store(const TrackSlot& t, int* __restrict__ slots, int tid, bool mine) {
  if (mine) {
    int* s = slots + tid * TRK_WORDS;
    s[0] = t.live; s[1] = t.id;
    s[2] = __float_as_int(t.x1); s[3] = __float_as_int(t.y1); s[4] = __float_as_int(t.x2); s[5] = __float_as_int(t.y2);
    s[6] = __float_as_int(t.vx); s[7] = __float_as_int(t.vy); s[8] = __float_as_int(t.label); s[9] = __float_as_int(t.score);
    s[10] = t.hits; s[11] = t.misses; s[12] = t.last;
  }
}

// 4. matched slot: the velocity takes beta of the residual of the centre, the box and the score become the detection's
__device__ __forceinline__ void trk_match(TrackShared& sh, TrackSlot& t, int md, int widx, const TrackParams& p) {
  const float dx1 = sh.dx1[md], dy1 = sh.dy1[md], dx2 = sh.dx2[md], dy2 = sh.dy2[md];
  const float rx = __fsub_rn(__fmul_rn(__fadd_rn(dx1, dx2), 0.5f), __fmul_rn(__fadd_rn(t.x1, t.x2), 0.5f));
  const float ry = __fsub_rn(__fmul_rn(__fadd_rn(dy1, dy2), 0.5f), __fmul_rn(__fadd_rn(t.y1, t.y2), 0.5f));
  t.vx = __fadd_rn(t.vx, __fmul_rn(p.beta, rx));
  t.vy = __fadd_rn(t.vy, __fmul_rn(p.beta, ry));
  t.x1 = dx1; t.y1 = dy1; t.x2 = dx2; t.y2 = dy2; t.score = sh.dscore[md];
  t.hits += 1; t.misses = 0; t.last = widx;
  sh.dtrack[md] = t.id;
  sh.dused[md] = 1;
}

// The optimal rule's pair (slot s, detection d): allowed = equal labels and iou >= iou_min (false for NaN).  The IoU is step 2's
// expression with every operation rounded on its own - the pragma keeps the union from being fused into an fma, so the weights are
// tests/track_ref.iou_matrix bit for bit.
__device__ __forceinline__ bool trk_allowed(const TrackShared& sh, const TrackOptimal& op, int s, int d, float iou_min, float& iou) {
#pragma clang fp contract(off)
  if (!(op.tlabel[s] == sh.dlabel[d])) return false;
  const float ww = fminf(op.tx2[s], sh.dx2[d]) - fmaxf(op.tx1[s], sh.dx1[d]);
  const float hh = fminf(op.ty2[s], sh.dy2[d]) - fmaxf(op.ty1[s], sh.dy1[d]);
  iou = 0.f;
  if (!(ww <= 0.f) && !(hh <= 0.f)) {
    const float inter = ww * hh;
    const float u = (op.tarea[s] + sh.darea[d]) - inter;
    iou = u > 0.f ? inter / u : 0.f;
  }
  return iou >= iou_min;
}

// 2. - 4. of the optimal rule.  Called by all 256 threads behind the predict step's __syncthreads; `matched` comes back true for the
// slots that took a detection.  Ends with the matched slots' sh.dtrack / sh.dused written but not yet synchronised (step 5 does that).
__device__ __forceinline__ bool trk_assign_optimal(TrackShared& sh, TrackOptimal& op, TrackSlot& t, float area, int n, int widx,
                                                   const TrackParams& p) {
  const int tid = threadIdx.x;
  op.tx1[tid] = t.x1; op.ty1[tid] = t.y1; op.tx2[tid] = t.x2; op.ty2[tid] = t.y2; op.tarea[tid] = area; op.tlabel[tid] = t.label;
  op.tmatch[tid] = -1;
  op.dany[tid] = 0;
  __syncthreads();
  bool any = false;
  if (t.live) {
    for (int d = 0; d < n; ++d) {
      float iou;
      if (trk_allowed(sh, op, tid, d, p.iou_min, iou)) { any = true; op.dany[d] = 1; }      // every writer stores the same 1
    }
  }
  __syncthreads();
  const int nl = mot_compact(any, op.tlist, op.wsum);
  if (nl == 0) return false;                              // uniform: no allowed pair, nothing is matched
  const int ml = mot_compact(tid < n && op.dany[tid] != 0, op.dlist, op.wsum);
  bool ok;
  if (nl <= ml) {
    ok = mot_assign<TRK_DMAX>(op.as, nl, ml, [&](int r, int c) -> double {
      float iou;
      return trk_allowed(sh, op, op.tlist[r], op.dlist[c], p.iou_min, iou) ? -(double)iou : 0.0;
    });
    if (ok && tid < ml) {
      const int r = op.as.p[tid + 1] - 1;
      float iou;
      if (r >= 0 && trk_allowed(sh, op, op.tlist[r], op.dlist[tid], p.iou_min, iou)) op.tmatch[op.tlist[r]] = op.dlist[tid];
    }
  } else {
    ok = mot_assign<TRK_DMAX>(op.as, ml, nl, [&](int r, int c) -> double {
      float iou;
      return trk_allowed(sh, op, op.tlist[c], op.dlist[r], p.iou_min, iou) ? -(double)iou : 0.0;
    });
    if (ok && tid < nl) {
      const int r = op.as.p[tid + 1] - 1;
      float iou;
      if (r >= 0 && trk_allowed(sh, op, op.tlist[tid], op.dlist[r], p.iou_min, iou)) op.tmatch[op.tlist[tid]] = op.dlist[r];
    }
  }
  if (!ok && tid == 0) sh.over = 1;                       // not reachable with finite costs: the window matches nothing
  __syncthreads();
  const int md = op.tmatch[tid];
  if (md < 0) return false;
  trk_match(sh, t, md, widx, p);
  return true;
}

// 2. - 4. of the greedy rule.  Called by all 256 threads behind the predict step's __syncthreads; true for the slots that took a detection.
__device__ __forceinline__ bool trk_assign_greedy(TrackShared& sh, TrackSlot& t, float area, int n, int widx, const TrackParams& p) {
  const int tid = threadIdx.x;
  // 2. this slot's best candidate among the unmatched detections: 0 = none
  auto best = [&]() -> unsigned long long {
    unsigned long long k = 0;
    for (int d = 0; d < n; ++d) {
      if (sh.dused[d] || !(sh.dlabel[d] == t.label)) continue;
      const float ww = __fsub_rn(fminf(t.x2, sh.dx2[d]), fmaxf(t.x1, sh.dx1[d]));
      const float hh = __fsub_rn(fminf(t.y2, sh.dy2[d]), fmaxf(t.y1, sh.dy1[d]));
      float iou = 0.f;
      if (!(ww <= 0.f) && !(hh <= 0.f)) {
        const float inter = __fmul_rn(ww, hh);
        const float u = __fsub_rn(__fadd_rn(area, sh.darea[d]), inter);
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
  unsigned long long key = (t.live && n > 0) ? best() : 0ull;

  // 3. greedy match: the block-wide largest key, until none is left (at most min(live slots, n) rounds)
  for (;;) {
    const unsigned long long wm = trk_wave_max(key);
    if ((tid & 63) == 0) sh.wmax[tid >> 6] = wm;
    __syncthreads();
    unsigned long long m = sh.wmax[0];
    m = sh.wmax[1] > m ? sh.wmax[1] : m;
    m = sh.wmax[2] > m ? sh.wmax[2] : m;
    m = sh.wmax[3] > m ? sh.wmax[3] : m;
    if (m == 0) break;                                  // uniform: every thread read the same four words
    const int ms = 0xFFFF - (int)((m >> 16) & 0xFFFFu), md = 0xFFFF - (int)(m & 0xFFFFu);
    if (tid == ms) {
      trk_match(sh, t, md, widx, p);                    // 4.
      matched = true;
      key = 0;
    }
    __syncthreads();                                    // sh.dused[md] is visible, and every thread is done with sh.wmax
    if (key != 0 && 0xFFFF - (int)(key & 0xFFFFu) == md) key = best();
  }
  return matched;
}

// One window through the tracker - the rule and the rounding of both kernels below.  Called by all 256 threads of the block: src = the
// window's rows [n_all, 6], o = the record row of its first row, widx = the window's index (a track's `last`).  sh.next / sh.over were
// set before the first window and are visible (a __syncthreads behind them); the call ends with a __syncthreads.
// ASSIGN: TRK_GREEDY or TRK_OPTIMAL, steps 2 - 4; op: the optimal rule's LDS (greedy: an empty struct).
template <int ASSIGN>
__device__ __forceinline__ void trk_window(TrackShared& sh, typename TrackRule<ASSIGN>::Shared& op, TrackSlot& t,
                                           const float* __restrict__ src, int n_all, long long o, int widx, int rec_cap,
                                           int* __restrict__ rec_track, bool mine, const TrackParams& p) {
  const int tid = threadIdx.x;
  const int n = min(n_all, TRK_DMAX);
  if (tid < n) {
    const float* r = src + tid * 6;
    const float a = r[0], b = r[1], c = r[2], d = r[3];
    sh.dx1[tid] = a; sh.dy1[tid] = b; sh.dx2[tid] = c; sh.dy2[tid] = d;
    sh.darea[tid] = __fmul_rn(__fsub_rn(c, a), __fsub_rn(d, b));
    sh.dscore[tid] = r[4]; sh.dlabel[tid] = r[5];
    sh.dtrack[tid] = -1; sh.dused[tid] = 0;
  }
  sh.birth[tid] = 0;
  if (tid == 0 && n_all > TRK_DMAX) sh.over = 1;
  // 1. predict
  float area = 0.f;
  if (t.live) {
    t.x1 = __fadd_rn(t.x1, t.vx); t.x2 = __fadd_rn(t.x2, t.vx); t.y1 = __fadd_rn(t.y1, t.vy); t.y2 = __fadd_rn(t.y2, t.vy);
    area = __fmul_rn(__fsub_rn(t.x2, t.x1), __fsub_rn(t.y2, t.y1));
  }
  __syncthreads();

  // 2. - 4. the association rule (uniform: n is the block's)
  bool matched = false;
  if constexpr (ASSIGN == TRK_OPTIMAL) {
    if (n > 0) matched = trk_assign_optimal(sh, op, t, area, n, widx, p);
  } else {
    matched = trk_assign_greedy(sh, t, area, n, widx, p);
  }

  // 5. unmatched live slots age; freeing comes before the births
  if (t.live && !matched) {
    t.misses += 1;
    if (t.misses > p.max_age) {
      t.live = 0; t.id = 0; t.hits = 0; t.misses = 0; t.last = 0;
      t.x1 = t.y1 = t.x2 = t.y2 = t.vx = t.vy = t.label = t.score = 0.f;
    }
  }
  sh.live[tid] = mine ? t.live : 1;                      // slots behind max_tracks are never free
  __syncthreads();
  // 6. births, in detection order, each into the lowest free slot (the free slots are taken in rising order: one pointer)
  if (tid == 0) {
    int f = 0, next = sh.next, over = sh.over;
    for (int d = 0; d < n; ++d) {
      if (sh.dused[d] || !(sh.dscore[d] >= p.birth_score)) continue;
      while (f < p.max_tracks && sh.live[f]) ++f;
      if (f < p.max_tracks) {
        sh.birth[f] = d + 1;
        sh.dtrack[d] = next++;
        ++f;
      } else {
        over = 1;
      }
    }
    sh.next = next; sh.over = over;
  }
  __syncthreads();
  if (mine && sh.birth[tid]) {
    const int d = sh.birth[tid] - 1;
    t.live = 1; t.id = sh.dtrack[d];
    t.x1 = sh.dx1[d]; t.y1 = sh.dy1[d]; t.x2 = sh.dx2[d]; t.y2 = sh.dy2[d];
    t.vx = 0.f; t.vy = 0.f; t.label = sh.dlabel[d]; t.score = sh.dscore[d];
    t.hits = 1; t.misses = 0; t.last = widx;
  }
  // 7. the rows' ids: -1 for every row that was neither matched nor born, and for the rows behind TRK_DMAX
  for (int j = tid; j < n_all; j += 256)
    if (o + j < rec_cap) rec_track[o + j] = j < n ? sh.dtrack[j] : -1;
  __syncthreads();                                      // the next window overwrites the detections
}

template <int ASSIGN>
__global__ __launch_bounds__(256) void track_update_kernel(const float* __restrict__ rows, const int* __restrict__ cnt, int B, int cap_img,
                                                           const int* __restrict__ ctl, const int* __restrict__ rec_count, int rec_cap,
                                                           int* __restrict__ rec_track, int* __restrict__ slots, int* __restrict__ glob,
                                                           TrackParams p) {
  __shared__ long long s_off[TRK_BMAX + 1];     // as det_record_append_kernel: record row of window i's first row
  __shared__ int s_nv;
  __shared__ TrackShared sh;
  __shared__ typename TrackRule<ASSIGN>::Shared op;
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
    sh.next = glob[0];
    sh.over = 0;
  }
  const bool mine = tid < p.max_tracks;
  TrackSlot t;
  trk_slot_load(t, slots, tid, mine);
  __syncthreads();
  const int nv = s_nv, first = ctl[1];
  for (int i = 0; i < nv; ++i)
    trk_window<ASSIGN>(sh, op, t, rows + (size_t)i * cap_img * 6, (int)(s_off[i + 1] - s_off[i]), s_off[i], first + i, rec_cap, rec_track, mine, p);
  trk_slot_store(t, slots, tid, mine);
  if (tid == 0) {
    glob[0] = sh.next;
    if (sh.over) glob[1] = 1;
  }
}

// The tracker of a bank of sessions (AudioDetector.open_bank): block s owns slots[s] / glob[s] and runs, in row order, the rows i <
// n_valid of the group with win_sess[i] == s through trk_window, with the row's own window index win_idx[i].  Every block does the
// whole scan of the offsets itself (it is the append's); the blocks write disjoint rows of rec_track.  A block whose session has no
// row in the group returns before it touches its state.
template <int ASSIGN>
__global__ __launch_bounds__(256) void track_update_bank_kernel(const float* __restrict__ rows, const int* __restrict__ cnt, int B,
                                                                int cap_img, const int* __restrict__ n_valid,
                                                                const int* __restrict__ win_sess, const int* __restrict__ win_idx,
                                                                const int* __restrict__ rec_count, int rec_cap,
                                                                int* __restrict__ rec_track, int* __restrict__ slots,
                                                                int* __restrict__ glob, TrackParams p) {
  __shared__ long long s_off[TRK_BMAX + 1];
  __shared__ int s_mine[TRK_BMAX];              // row i is this block's session's
  __shared__ int s_nv, s_any;
  __shared__ TrackShared sh;
  __shared__ typename TrackRule<ASSIGN>::Shared op;
  const int tid = threadIdx.x, sess = blockIdx.x;
  slots += (size_t)sess * p.max_tracks * TRK_WORDS;
  glob += (size_t)sess * 2;
  if (tid == 0) {
    const int nv = max(0, min(*n_valid, B));
    long long o = max(*rec_count, 0);
    int any = 0;
    for (int i = 0; i < nv; ++i) {
      s_off[i] = o;
      o += max(0, min(cnt[i], cap_img));
      const int m = win_sess[i] == sess;
      s_mine[i] = m;
      any |= m;
    }
    s_off[nv] = o;
    s_nv = nv;
    s_any = any;
    sh.next = glob[0];
    sh.over = 0;
  }
  __syncthreads();
  if (!s_any) return;                                     // uniform: an absent session's state is not touched, nothing ages
  const bool mine = tid < p.max_tracks;
  TrackSlot t;
  trk_slot_load(t, slots, tid, mine);
  const int nv = s_nv;
  for (int i = 0; i < nv; ++i) {
    if (!s_mine[i]) continue;                             // uniform
    trk_window<ASSIGN>(sh, op, t, rows + (size_t)i * cap_img * 6, (int)(s_off[i + 1] - s_off[i]), s_off[i], win_idx[i], rec_cap, rec_track, mine, p);
  }
  trk_slot_store(t, slots, tid, mine);
  if (tid == 0) {
    glob[0] = sh.next;
    if (sh.over) glob[1] = 1;
  }
}

static int trk_launch(const float* rows, const int* cnt, int B, int cap_img, const int* ctl, const int* rec_count, int rec_cap,
                      int* rec_track, int* trk_slots, int* trk_glob, int max_tracks, float iou_min, float beta, int max_age,
                      float birth_score, int assign, hipStream_t stream) {
  if (!rows || !cnt || !ctl || !rec_count || !rec_track || !trk_slots || !trk_glob) return MMD_EINVAL;
  if (B <= 0 || B > TRK_BMAX || cap_img <= 0 || rec_cap <= 0 || (long long)cap_img * 6 > 0x7fffffffLL) return MMD_EINVAL;
  if (max_tracks < 1 || max_tracks > TRK_SMAX || max_age < 0) return MMD_EINVAL;
  TrackParams p;
  p.max_tracks = max_tracks; p.max_age = max_age; p.iou_min = iou_min; p.beta = beta; p.birth_score = birth_score;
  if (assign == TRK_OPTIMAL)
    hipLaunchKernelGGL(track_update_kernel<TRK_OPTIMAL>, dim3(1), dim3(256), 0, stream, rows, cnt, B, cap_img, ctl, rec_count, rec_cap,
                       rec_track, trk_slots, trk_glob, p);
  else
    hipLaunchKernelGGL(track_update_kernel<TRK_GREEDY>, dim3(1), dim3(256), 0, stream, rows, cnt, B, cap_img, ctl, rec_count, rec_cap,
                       rec_track, trk_slots, trk_glob, p);
  return mmd_check_launch();
}

static int trk_launch_bank(const float* rows, const int* cnt, int B, int cap_img, const int* n_valid, const int* win_sess,
                           const int* win_idx, int n_sessions, const int* rec_count, int rec_cap, int* rec_track, int* trk_slots,
                           int* trk_glob, int max_tracks, float iou_min, float beta, int max_age, float birth_score, int assign,
                           hipStream_t stream) {
  if (!rows || !cnt || !n_valid || !win_sess || !win_idx || !rec_count || !rec_track || !trk_slots || !trk_glob) return MMD_EINVAL;
  if (B <= 0 || B > TRK_BMAX || cap_img <= 0 || rec_cap <= 0 || (long long)cap_img * 6 > 0x7fffffffLL) return MMD_EINVAL;
  if (n_sessions < 1 || n_sessions > 65535 || max_tracks < 1 || max_tracks > TRK_SMAX || max_age < 0) return MMD_EINVAL;
  TrackParams p;
  p.max_tracks = max_tracks; p.max_age = max_age; p.iou_min = iou_min; p.beta = beta; p.birth_score = birth_score;
  if (assign == TRK_OPTIMAL)
    hipLaunchKernelGGL(track_update_bank_kernel<TRK_OPTIMAL>, dim3(n_sessions), dim3(256), 0, stream, rows, cnt, B, cap_img, n_valid,
                       win_sess, win_idx, rec_count, rec_cap, rec_track, trk_slots, trk_glob, p);
  else
    hipLaunchKernelGGL(track_update_bank_kernel<TRK_GREEDY>, dim3(n_sessions), dim3(256), 0, stream, rows, cnt, B, cap_img, n_valid,
                       win_sess, win_idx, rec_count, rec_cap, rec_track, trk_slots, trk_glob, p);
  return mmd_check_launch();
}

extern "C" int mmd_track_update(const float* rows, const int* cnt, int B, int cap_img, const int* ctl, const int* rec_count, int rec_cap,
                                int* rec_track, int* trk_slots, int* trk_glob, int max_tracks, float iou_min, float beta, int max_age,
                                float birth_score, hipStream_t stream) {
  return trk_launch(rows, cnt, B, cap_img, ctl, rec_count, rec_cap, rec_track, trk_slots, trk_glob, max_tracks, iou_min, beta, max_age,
                    birth_score, TRK_GREEDY, stream);
}

// assign: 0 greedy (the kernel mmd_track_update launches), 1 optimal
extern "C" int mmd_track_update_assign(const float* rows, const int* cnt, int B, int cap_img, const int* ctl, const int* rec_count,
                                       int rec_cap, int* rec_track, int* trk_slots, int* trk_glob, int max_tracks, float iou_min,
                                       float beta, int max_age, float birth_score, int assign, hipStream_t stream) {
  if (assign != TRK_GREEDY && assign != TRK_OPTIMAL) return MMD_EINVAL;
  return trk_launch(rows, cnt, B, cap_img, ctl, rec_count, rec_cap, rec_track, trk_slots, trk_glob, max_tracks, iou_min, beta, max_age,
                    birth_score, assign, stream);
}

extern "C" int mmd_track_update_bank(const float* rows, const int* cnt, int B, int cap_img, const int* n_valid, const int* win_sess,
                                     const int* win_idx, int n_sessions, const int* rec_count, int rec_cap, int* rec_track,
                                     int* trk_slots, int* trk_glob, int max_tracks, float iou_min, float beta, int max_age,
                                     float birth_score, hipStream_t stream) {
  return trk_launch_bank(rows, cnt, B, cap_img, n_valid, win_sess, win_idx, n_sessions, rec_count, rec_cap, rec_track, trk_slots, trk_glob,
                         max_tracks, iou_min, beta, max_age, birth_score, TRK_GREEDY, stream);
}

extern "C" int mmd_track_update_bank_assign(const float* rows, const int* cnt, int B, int cap_img, const int* n_valid, const int* win_sess,
                                            const int* win_idx, int n_sessions, const int* rec_count, int rec_cap, int* rec_track,
                                            int* trk_slots, int* trk_glob, int max_tracks, float iou_min, float beta, int max_age,
                                            float birth_score, int assign, hipStream_t stream) {
  if (assign != TRK_GREEDY && assign != TRK_OPTIMAL) return MMD_EINVAL;
  return trk_launch_bank(rows, cnt, B, cap_img, n_valid, win_sess, win_idx, n_sessions, rec_count, rec_cap, rec_track, trk_slots, trk_glob,
                         max_tracks, iou_min, beta, max_age, birth_score, assign, stream);
}
