// Tracking evaluation (mm_distillnet_amd/mot.py, evaluate_tracks.py): the CLEAR-MOT counts (Bernardin & Stiefelhagen 2008) and the
// identity measures (Ristani et al. 2016) of a tracked record - the rows / window / track[/ session] that track_stream, track_rows or a
// LiveBank return - against a ground-truth record of the same shape.  The rule is written out in DESIGN.md (tracking evaluation) and
// restated in numpy / scipy by tests/mot_ref.py.
//
// Both measures rest on an OPTIMAL assignment, which the tracker's greedy pairing is not.  mot_assign (mot_assign.h) is the one routine for
// both: the shortest-augmenting-path algorithm with potentials (Jonker-Volgenant, the "Hungarian algorithm with potentials") for an
// n x m cost matrix, n <= m (the caller transposes), minimising; the callers pass cost = -weight.  One 256-thread block.  Thread t owns
// the columns t, t + 256, .. - so m may exceed 256 - and each inner step is one pass over the owned columns (relax minv / way against
// the row just added to the tree) and ONE block-wide arg-min of (minv, column): a wave shuffle inside the four waves, then LDS across
// them, ties to the lowest column.  Potentials, minv, way and the column-to-row table live in LDS as float64 / int (37 KB at
// m = 1024).  The cost is a functor: CLEAR computes the IoU on the fly from the window's boxes staged in LDS, identity reads C from
// global memory.  The arithmetic is float64 on float32 IoUs (CLEAR) or on integers (identity: exact).
//
// IoU: mmd_box_iou below, the tracker's expression with every operation rounded on its own.  A pair is ALLOWED when the labels are equal and iou >= iou_min (false for NaN).
//
// mmd_mot_clear: one block per session walks the session's windows in order (window w needs the map window w-1 left).  Per window the
// first MOT_RMAX rows of each side are staged in LDS, then keep / assign / count as DESIGN.md says.  Thread i counts for ground-truth
// row i and hypothesis row i in registers for the whole walk; one block reduction at the end.  No atomics: two runs give the same bits.
// mmd_mot_id_counts: one block per (window, session) adds 1 to C[g][h] for every allowed pair of its window - integer atomicAdd, so the
// order of arrival does not matter.  mmd_mot_id_assign: one block per session, mot_assign on C, IDTP = the matching's weight.
// HOTA (Luiten et al. 2021; the section at the end of this file): mmd_hota_align and mmd_hota_match run one block per (window, session)
// - no window needs another window's result inside a pass - and accumulate integers only; mmd_hota_assoc, one block per session, turns
// the per-cell histograms into the association numerators.  They share mot_assign, MotSide / mot_stage / mot_span and mmd_box_iou.
// Plain HIP, vector stores only.
#include "common.h"
#include "mot_assign.h"      // MotAssign / mot_assign / MOT_INF / mot_compact: shared with the tracker (track.hip)

// The float32 IoU of the rule, ONE function for every user in this file: areas without +1 (area = (x2 - x1) * (y2 - y1), kept beside
// the boxes), ww = min(x2) - max(x1), hh likewise; 0 where either is <= 0 or the union is not positive; otherwise
// inter / ((area_a + area_b) - inter).  Every operation is rounded on its own; fminf / fmaxf let the non-NaN operand win:
// tests/track_ref.iou_matrix is the numpy float32 restatement, bit for bit (iou_sum is compared to the last bits).  The contraction
// pragma is what makes that true: __fmul_rn / __fsub_rn are plain `*` / `-` in this toolchain's headers, and left to the default
// contraction the compiler fuses the union into fma(-ww, hh, area_a + area_b) - it does so in track.hip's own copy of this
// expression, whose IoUs can therefore differ from these by an ulp.  The tracker only compares and ranks its IoUs and keeps its code
// and its bits; it does not include this function.
__device__ __forceinline__ float mmd_box_area(float x1, float y1, float x2, float y2) {
#pragma clang fp contract(off)
  return (x2 - x1) * (y2 - y1);
}
__device__ __forceinline__ float mmd_box_iou(float ax1, float ay1, float ax2, float ay2, float a_area, float bx1, float by1, float bx2,
                                             float by2, float b_area) {
#pragma clang fp contract(off)
  const float ww = fminf(ax2, bx2) - fmaxf(ax1, bx1);
  const float hh = fminf(ay2, by2) - fmaxf(ay1, by1);
  float iou = 0.f;
  if (!(ww <= 0.f) && !(hh <= 0.f)) {
    const float inter = ww * hh;
    const float u = (a_area + b_area) - inter;
    iou = u > 0.f ? inter / u : 0.f;                      // `/` is the correctly rounded division (hipcc's default)
  }
  return iou;
}

#define MOT_RMAX 256       // rows of one side in one window (the tracker's TRK_DMAX)
#define MOT_TMAX 1024       // tracks per side and session of the identity measures

// ---- one window of both records in LDS ------------------------------------------------------------------------------------------------
struct MotSide {
  float x1[MOT_RMAX], y1[MOT_RMAX], x2[MOT_RMAX], y2[MOT_RMAX], area[MOT_RMAX], label[MOT_RMAX];
  int trk[MOT_RMAX];          // dense track id (-1: a hypothesis row without a track; out of range: the row takes no part)
  int pair[MOT_RMAX];         // the other side's row this row is paired with (-1: none)
};

__device__ __forceinline__ void mot_stage(MotSide& s, const float* __restrict__ rows, const int* __restrict__ track, int lo, int n,
                                          int n_tracks) {
  const int tid = threadIdx.x;
  if (tid < n) {
    const float* r = rows + (size_t)(lo + tid) * 6;
    const float a = r[0], b = r[1], c = r[2], d = r[3];
    s.x1[tid] = a; s.y1[tid] = b; s.x2[tid] = c; s.y2[tid] = d;
    s.area[tid] = mmd_box_area(a, b, c, d);
    s.label[tid] = r[5];
    const int t = track[lo + tid];
    s.trk[tid] = (t >= 0 && t < n_tracks) ? t : -1;
    s.pair[tid] = -1;
  }
}

__device__ __forceinline__ float mot_iou(const MotSide& g, int i, const MotSide& h, int j) {
  return mmd_box_iou(g.x1[i], g.y1[i], g.x2[i], g.y2[i], g.area[i], h.x1[j], h.y1[j], h.x2[j], h.y2[j], h.area[j]);
}
__device__ __forceinline__ bool mot_allowed(const MotSide& g, int i, const MotSide& h, int j, float iou_min, float& iou) {
  if (!(g.label[i] == h.label[j])) return false;
  iou = mot_iou(g, i, h, j);
  return iou >= iou_min;                                 // false for NaN
}

// rows of [lo, lo + n) clamped into the table's range: a corrupt offset table reads nothing out of bounds
__device__ __forceinline__ void mot_span(const int* __restrict__ off, long long k, int total, int& lo, int& n) {
  const int a = off[k], b = off[k + 1];
  lo = min(max(a, 0), total);
  n = min(max(b, lo), total) - lo;
  n = min(n, MOT_RMAX);
}

struct ClearShared {
  MotSide g, h;
  int gmap[MOT_RMAX];         // map[track of ground-truth row i] when the window starts
  int glist[MOT_RMAX], hlist[MOT_RMAX];
  int wsum[4];
  double wred[4];
  long long ired[4][5];
  MotAssign<MOT_RMAX> as;
};

// ws per ground-truth track: {map, state}; state bit 0: paired in the last window the track was present in, bit 1: paired before
__global__ __launch_bounds__(256) void mot_clear_kernel(const float* __restrict__ gt_rows, const int* __restrict__ gt_track,
                                                        const int* __restrict__ gt_off, int n_gt_rows, const float* __restrict__ hyp_rows,
                                                        const int* __restrict__ hyp_track, const int* __restrict__ hyp_off, int n_hyp_rows,
                                                        int n_windows, const int* __restrict__ gt_trk_off, int n_gt_tracks, float iou_min,
                                                        long long* __restrict__ counts, double* __restrict__ iou_sum,
                                                        int* __restrict__ present, int* __restrict__ matched, int* __restrict__ ws) {
  __shared__ ClearShared sh;
  const int tid = threadIdx.x, sess = blockIdx.x;
  int t_lo = min(max(gt_trk_off[sess], 0), n_gt_tracks);
  const int G = min(max(gt_trk_off[sess + 1], t_lo), n_gt_tracks) - t_lo;
  present += t_lo; matched += t_lo;
  int* map = ws + 2 * (size_t)t_lo;
  int* state = map + G;
  for (int g = tid; g < G; g += 256) { map[g] = -1; state[g] = 0; present[g] = 0; matched[g] = 0; }
  long long c_gt = 0, c_hyp = 0, c_tp = 0, c_fp = 0, c_fn = 0, c_idsw = 0, c_frag = 0;
  double c_iou = 0.0;
  __syncthreads();

  for (int w = 0; w < n_windows; ++w) {
    const long long k = (long long)sess * n_windows + w;
    int glo, ng, hlo, nh;
    mot_span(gt_off, k, n_gt_rows, glo, ng);
    mot_span(hyp_off, k, n_hyp_rows, hlo, nh);
    if (ng == 0 && nh == 0) continue;                    // uniform
    mot_stage(sh.g, gt_rows, gt_track, glo, ng, G);
    mot_stage(sh.h, hyp_rows, hyp_track, hlo, nh, 0x7fffffff);
    if (tid < ng) sh.gmap[tid] = sh.g.trk[tid] >= 0 ? map[sh.g.trk[tid]] : -1;
    __syncthreads();
    // 1. keep: hypothesis row j of track t looks for the FIRST ground-truth row whose map is t and whose pair with it is allowed.  A
    // window holds a track once per side, so no two hypothesis rows want the same ground-truth row: this is the rule's walk in row order.
    if (ng > 0 && tid < nh && sh.h.trk[tid] >= 0) {
      const int t = sh.h.trk[tid];
      for (int i = 0; i < ng; ++i) {
        float iou;
        if (sh.gmap[i] == t && mot_allowed(sh.g, i, sh.h, tid, iou_min, iou)) {
          sh.h.pair[tid] = i;
          sh.g.pair[i] = tid;
          break;
        }
      }
    }
    __syncthreads();
    // 2. assign: what is left of both sides
    const int nl = mot_compact(tid < ng && sh.g.pair[tid] < 0 && sh.g.trk[tid] >= 0, sh.glist, sh.wsum);
    const int ml = mot_compact(tid < nh && sh.h.pair[tid] < 0 && sh.h.trk[tid] >= 0, sh.hlist, sh.wsum);
    if (nl > 0 && ml > 0) {                              // uniform
      bool any = false;
      if (tid < nl) {
        const int i = sh.glist[tid];
        for (int c = 0; c < ml && !any; ++c) {
          float iou;
          any = mot_allowed(sh.g, i, sh.h, sh.hlist[c], iou_min, iou);
        }
      }
      if (__syncthreads_or(any)) {                       // no allowed pair: nothing to assign
        // mot_iou(g, h) is the expression's order in every use: the functor of the transposed problem swaps its indices back
        bool ok;
        if (nl <= ml) {
          auto cost = [&](int r, int c) -> double {
            float iou = 0.f;
            return mot_allowed(sh.g, sh.glist[r], sh.h, sh.hlist[c], iou_min, iou) ? -(double)iou : 0.0;
          };
          ok = mot_assign<MOT_RMAX>(sh.as, nl, ml, cost);
          if (ok) {
            for (int c = tid; c < ml; c += 256) {
              const int r = sh.as.p[c + 1] - 1;
              if (r < 0) continue;
              const int i = sh.glist[r], j = sh.hlist[c];
              float iou;
              if (mot_allowed(sh.g, i, sh.h, j, iou_min, iou)) { sh.g.pair[i] = j; sh.h.pair[j] = i; }
            }
          }
        } else {
          auto cost = [&](int r, int c) -> double {
            float iou = 0.f;
            return mot_allowed(sh.g, sh.glist[c], sh.h, sh.hlist[r], iou_min, iou) ? -(double)iou : 0.0;
          };
          ok = mot_assign<MOT_RMAX>(sh.as, ml, nl, cost);
          if (ok) {
            for (int c = tid; c < nl; c += 256) {
              const int r = sh.as.p[c + 1] - 1;
              if (r < 0) continue;
              const int i = sh.glist[c], j = sh.hlist[r];
              float iou;
              if (mot_allowed(sh.g, i, sh.h, j, iou_min, iou)) { sh.g.pair[i] = j; sh.h.pair[j] = i; }
            }
          }
        }
        __syncthreads();
      }
    }
    // 3. - 5. count: thread i for ground-truth row i and for hypothesis row i
    if (tid < ng) {
      c_gt += 1;
      const int j = sh.g.pair[tid], g = sh.g.trk[tid];
      if (j >= 0) {
        const int h = sh.h.trk[j], was = sh.gmap[tid];
        c_tp += 1;
        c_iou += (double)mot_iou(sh.g, tid, sh.h, j);
        if (was >= 0 && was != h) c_idsw += 1;
        map[g] = h;
      } else {
        c_fn += 1;
      }
      if (g >= 0) {
        const int st = state[g];
        present[g] += 1;
        if (j >= 0) {
          matched[g] += 1;
          if ((st & 2) && !(st & 1)) c_frag += 1;
        }
        state[g] = (j >= 0) ? 3 : (st & 2);
      }
    }
    if (tid < nh) {
      c_hyp += 1;
      if (sh.h.pair[tid] < 0) c_fp += 1;
    }
    __syncthreads();                                     // map / state are visible, the next window overwrites the rows
  }

  // the block's sums, in a fixed order
  long long v[5] = {c_tp, c_fp, c_fn, c_idsw, c_frag};
#pragma unroll
  for (int q = 0; q < 5; ++q) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[q] += __shfl_xor(v[q], o, 64);
  }
  c_iou = wave_sum_d(c_iou);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int q = 0; q < 5; ++q) sh.ired[tid >> 6][q] = v[q];
    sh.wred[tid >> 6] = c_iou;
  }
  // n_gt / n_hyp: the rows the walk saw (the first MOT_RMAX of a window)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { c_gt += __shfl_xor(c_gt, o, 64); c_hyp += __shfl_xor(c_hyp, o, 64); }
  __shared__ long long s_n[4][2];
  if ((tid & 63) == 0) { s_n[tid >> 6][0] = c_gt; s_n[tid >> 6][1] = c_hyp; }
  __syncthreads();
  if (tid == 0) {
    long long* o = counts + (size_t)sess * 8;
    o[0] = s_n[0][0] + s_n[1][0] + s_n[2][0] + s_n[3][0];
    o[1] = s_n[0][1] + s_n[1][1] + s_n[2][1] + s_n[3][1];
    for (int q = 0; q < 5; ++q) o[2 + q] = sh.ired[0][q] + sh.ired[1][q] + sh.ired[2][q] + sh.ired[3][q];
    o[7] = n_windows;
    iou_sum[sess] = ((sh.wred[0] + sh.wred[1]) + sh.wred[2]) + sh.wred[3];
  }
}

// ---- identity -------------------------------------------------------------------------------------------------------------------------
struct IdShared { MotSide g, h; };

__global__ __launch_bounds__(256) void mot_id_counts_kernel(const float* __restrict__ gt_rows, const int* __restrict__ gt_track,
                                                            const int* __restrict__ gt_off, int n_gt_rows,
                                                            const float* __restrict__ hyp_rows, const int* __restrict__ hyp_track,
                                                            const int* __restrict__ hyp_off, int n_hyp_rows, int n_windows,
                                                            const int* __restrict__ gt_trk_off, const int* __restrict__ hyp_trk_off,
                                                            const long long* __restrict__ c_off, long long c_total, float iou_min,
                                                            int* __restrict__ C) {
  __shared__ IdShared sh;
  const int tid = threadIdx.x, w = blockIdx.x, sess = blockIdx.y;
  const long long k = (long long)sess * n_windows + w;
  int glo, ng, hlo, nh;
  mot_span(gt_off, k, n_gt_rows, glo, ng);
  mot_span(hyp_off, k, n_hyp_rows, hlo, nh);
  if (ng == 0 || nh == 0) return;                        // uniform
  const int G = gt_trk_off[sess + 1] - gt_trk_off[sess], H = hyp_trk_off[sess + 1] - hyp_trk_off[sess];
  const long long c0 = c_off[sess];
  if (G < 1 || H < 1 || c0 < 0 || c0 + (long long)G * H > c_total) return;      // the caller's tables are wrong: nothing is written
  mot_stage(sh.g, gt_rows, gt_track, glo, ng, G);
  mot_stage(sh.h, hyp_rows, hyp_track, hlo, nh, H);
  __syncthreads();
  // thread (i, j-phase): 256 threads over ng x nh pairs
  for (int q = tid; q < ng * nh; q += 256) {
    const int i = q / nh, j = q - i * nh;
    const int g = sh.g.trk[i], h = sh.h.trk[j];
    float iou;
    if (g >= 0 && h >= 0 && mot_allowed(sh.g, i, sh.h, j, iou_min, iou)) atomicAdd(&C[c0 + (long long)g * H + h], 1);
  }
}

__global__ __launch_bounds__(256) void mot_id_assign_kernel(const int* __restrict__ C, const long long* __restrict__ c_off,
                                                            long long c_total, const int* __restrict__ gt_trk_off,
                                                            const int* __restrict__ hyp_trk_off, long long* __restrict__ idtp) {
  __shared__ MotAssign<MOT_TMAX> as;
  __shared__ long long s_sum[4];
  const int tid = threadIdx.x, sess = blockIdx.x;
  const int G = gt_trk_off[sess + 1] - gt_trk_off[sess], H = hyp_trk_off[sess + 1] - hyp_trk_off[sess];
  const long long c0 = c_off[sess];
  if (G < 0 || H < 0 || G > MOT_TMAX || H > MOT_TMAX || c0 < 0 || c0 + (long long)G * H > c_total) {      // the caller's tables are wrong
    if (tid == 0) idtp[sess] = -1;
    return;
  }
  if (G == 0 || H == 0) {
    if (tid == 0) idtp[sess] = 0;
    return;
  }
  const int* Cs = C + c0;
  long long sum = 0;
  bool ok;
  if (G <= H) {               // rows g, columns h: the owned columns of a row are read coalesced
    ok = mot_assign<MOT_TMAX>(as, G, H, [&](int r, int c) -> double { return -(double)Cs[(size_t)r * H + c]; });
    if (ok)
      for (int c = tid; c < H; c += 256) {
        const int r = as.p[c + 1] - 1;
        if (r >= 0) sum += Cs[(size_t)r * H + c];
      }
  } else {                    // transposed: rows h, columns g (a strided read of C, which L2 holds)
    ok = mot_assign<MOT_TMAX>(as, H, G, [&](int r, int c) -> double { return -(double)Cs[(size_t)c * H + r]; });
    if (ok)
      for (int c = tid; c < G; c += 256) {
        const int r = as.p[c + 1] - 1;
        if (r >= 0) sum += Cs[(size_t)c * H + r];
      }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if ((tid & 63) == 0) s_sum[tid >> 6] = sum;
  __syncthreads();
  if (tid == 0) idtp[sess] = ok ? s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3] : -1;
}

// ---- C ABI ----------------------------------------------------------------------------------------------------------------------------
extern "C" int mmd_mot_clear_ws_bytes(long long n_gt_tracks) {
  if (n_gt_tracks < 0 || n_gt_tracks > 0x07ffffffll) return MMD_EINVAL;
  return (int)(n_gt_tracks * 8 + 16);
}

static bool mot_sizes_ok(long long n_gt_rows, long long n_hyp_rows, int n_sessions, int n_windows) {
  if (n_gt_rows < 0 || n_hyp_rows < 0 || n_gt_rows > 0x7fffffffll / 6 || n_hyp_rows > 0x7fffffffll / 6) return false;
  if (n_sessions < 1 || n_sessions > 65535 || n_windows < 1) return false;
  return (long long)n_sessions * n_windows < 0x7fffffffll;
}

extern "C" int mmd_mot_clear(const float* gt_rows, const int* gt_track, const int* gt_off, long long n_gt_rows, const float* hyp_rows,
                             const int* hyp_track, const int* hyp_off, long long n_hyp_rows, int n_sessions, int n_windows,
                             const int* gt_trk_off, long long n_gt_tracks, float iou_min, long long* counts, double* iou_sum, int* present,
                             int* matched, void* ws, hipStream_t stream) {
  if (!gt_off || !hyp_off || !gt_trk_off || !counts || !iou_sum || !present || !matched || !ws) return MMD_EINVAL;
  if (!mot_sizes_ok(n_gt_rows, n_hyp_rows, n_sessions, n_windows) || mmd_mot_clear_ws_bytes(n_gt_tracks) < 0) return MMD_EINVAL;
  if ((n_gt_rows > 0 && (!gt_rows || !gt_track)) || (n_hyp_rows > 0 && (!hyp_rows || !hyp_track))) return MMD_EINVAL;
  hipLaunchKernelGGL(mot_clear_kernel, dim3(n_sessions), dim3(256), 0, stream, gt_rows, gt_track, gt_off, (int)n_gt_rows, hyp_rows, hyp_track,
                     hyp_off, (int)n_hyp_rows, n_windows, gt_trk_off, (int)n_gt_tracks, iou_min, counts, iou_sum, present, matched, (int*)ws);
  return mmd_check_launch();
}

extern "C" int mmd_mot_id_counts(const float* gt_rows, const int* gt_track, const int* gt_off, long long n_gt_rows, const float* hyp_rows,
                                 const int* hyp_track, const int* hyp_off, long long n_hyp_rows, int n_sessions, int n_windows,
                                 const int* gt_trk_off, const int* hyp_trk_off, int max_tracks, const long long* c_off, long long c_total,
                                 float iou_min, int* C, hipStream_t stream) {
  if (!gt_off || !hyp_off || !gt_trk_off || !hyp_trk_off || !c_off || !C) return MMD_EINVAL;
  if (!mot_sizes_ok(n_gt_rows, n_hyp_rows, n_sessions, n_windows) || c_total < 1 || max_tracks < 1 || max_tracks > MOT_TMAX) return MMD_EINVAL;
  if ((n_gt_rows > 0 && (!gt_rows || !gt_track)) || (n_hyp_rows > 0 && (!hyp_rows || !hyp_track))) return MMD_EINVAL;
  hipLaunchKernelGGL(mot_id_counts_kernel, dim3(n_windows, n_sessions), dim3(256), 0, stream, gt_rows, gt_track, gt_off, (int)n_gt_rows,
                     hyp_rows, hyp_track, hyp_off, (int)n_hyp_rows, n_windows, gt_trk_off, hyp_trk_off, c_off, c_total, iou_min, C);
  return mmd_check_launch();
}

extern "C" int mmd_mot_id_assign(const int* C, const long long* c_off, long long c_total, const int* gt_trk_off, const int* hyp_trk_off,
                                 int n_sessions, int max_tracks, long long* idtp, hipStream_t stream) {
  if (!C || !c_off || !gt_trk_off || !hyp_trk_off || !idtp) return MMD_EINVAL;
  if (n_sessions < 1 || n_sessions > 65535 || c_total < 1 || max_tracks < 1 || max_tracks > MOT_TMAX) return MMD_EINVAL;
  hipLaunchKernelGGL(mot_id_assign_kernel, dim3(n_sessions), dim3(256), 0, stream, C, c_off, c_total, gt_trk_off, hyp_trk_off, idtp);
  return mmd_check_launch();
}

// ---- HOTA (Luiten et al. 2021) --------------------------------------------------------------------------------------------------------
// The rule is DESIGN.md's (tracking evaluation, HOTA); tests/hota_ref.py restates it.  Everything that is accumulated is an integer:
// q(x) = floor(x * 2^32 + 0.5) of a float32 IoU or of a float64 quotient in [0, 1], summed with integer atomics, so the order of arrival
// does not matter and two runs give the same bits.  No window needs another window's result inside a pass: one block per (window,
// session) in passes 1 and 2.  Hypothesis rows with track -1 (and rows whose id is outside the session's range) take no part.
#define HOTA_NA 19          // thresholds alpha_k = float32((k + 1) / 20)

__device__ __forceinline__ unsigned long long hota_q(double x) { return (unsigned long long)floor(x * 4294967296.0 + 0.5); }

// s(i, j): the IoU where both rows have a track and the labels are equal, else 0 (never NaN: `!(s > 0)` is "no similarity")
__device__ __forceinline__ float hota_sim(const MotSide& g, int i, const MotSide& h, int j) {
  if (g.trk[i] < 0 || h.trk[j] < 0 || !(g.label[i] == h.label[j])) return 0.f;
  const float s = mot_iou(g, i, h, j);
  return s > 0.f ? s : 0.f;
}
__device__ __forceinline__ unsigned long long hota_qsim(const MotSide& g, int i, const MotSide& h, int j) {
  const float s = hota_sim(g, i, h, j);
  return s > 0.f ? hota_q((double)s) : 0ull;
}
// the number of thresholds s passes; they nest, so these are the first `bins`
__device__ __forceinline__ int hota_bins(float s) {
  int b = 0;
#pragma unroll
  for (int k = 0; k < HOTA_NA; ++k) b += (s >= (float)((double)(k + 1) / 20.0)) ? 1 : 0;
  return b;
}
// gas(g, h) * s in float64, every operation rounded on its own (the restatement's bits): gas = P / (2^32 (gc + tc) - P)
__device__ __forceinline__ double hota_score(unsigned long long p, int gcount, int tcount, float s) {
#pragma clang fp contract(off)
  const double den = 4294967296.0 * (double)((long long)gcount + (long long)tcount) - (double)p;
  if (!(den > 0.0)) return 0.0;                          // the caller's counts are wrong
  return ((double)p / den) * (double)s;
}

// the session's part of the tables; false (uniform) when the caller's tables are wrong: nothing is read or written then
struct HotaSess { int G, H, g0, h0; long long c0; };
__device__ __forceinline__ bool hota_sess(const int* __restrict__ gt_trk_off, const int* __restrict__ hyp_trk_off,
                                          const long long* __restrict__ c_off, long long c_total, int sess, HotaSess& t) {
  t.g0 = gt_trk_off[sess]; t.h0 = hyp_trk_off[sess];
  t.G = gt_trk_off[sess + 1] - t.g0; t.H = hyp_trk_off[sess + 1] - t.h0;
  t.c0 = c_off[sess];
  return t.g0 >= 0 && t.h0 >= 0 && t.G >= 0 && t.H >= 0 && t.G <= MOT_TMAX && t.H <= MOT_TMAX && t.c0 >= 0 &&
         t.c0 + (long long)t.G * t.H <= c_total;
}

struct HotaAlignShared {
  MotSide g, h;
  unsigned long long R[MOT_RMAX], C[MOT_RMAX];           // row / column sums of q(s)
};

// pass 1: P[g][h] += q(q(s) / (R_i + C_j - q(s))) for every pair of the window with q(s) > 0
__global__ __launch_bounds__(256) void hota_align_kernel(const float* __restrict__ gt_rows, const int* __restrict__ gt_track,
                                                         const int* __restrict__ gt_off, int n_gt_rows, const float* __restrict__ hyp_rows,
                                                         const int* __restrict__ hyp_track, const int* __restrict__ hyp_off, int n_hyp_rows,
                                                         int n_windows, const int* __restrict__ gt_trk_off,
                                                         const int* __restrict__ hyp_trk_off, const long long* __restrict__ c_off,
                                                         long long c_total, unsigned long long* __restrict__ P) {
  __shared__ HotaAlignShared sh;
  const int tid = threadIdx.x, w = blockIdx.x, sess = blockIdx.y;
  const long long k = (long long)sess * n_windows + w;
  int glo, ng, hlo, nh;
  mot_span(gt_off, k, n_gt_rows, glo, ng);
  mot_span(hyp_off, k, n_hyp_rows, hlo, nh);
  if (ng == 0 || nh == 0) return;                        // uniform
  HotaSess t;
  if (!hota_sess(gt_trk_off, hyp_trk_off, c_off, c_total, sess, t) || t.G < 1 || t.H < 1) return;
  mot_stage(sh.g, gt_rows, gt_track, glo, ng, t.G);
  mot_stage(sh.h, hyp_rows, hyp_track, hlo, nh, t.H);
  __syncthreads();
  // thread i owns ground-truth row i, thread j hypothesis row j; the IoUs are recomputed below, not kept (256 x 256 floats)
  if (tid < ng) {
    unsigned long long r = 0;
    for (int j = 0; j < nh; ++j) r += hota_qsim(sh.g, tid, sh.h, j);
    sh.R[tid] = r;
  }
  if (tid < nh) {
    unsigned long long c = 0;
    for (int i = 0; i < ng; ++i) c += hota_qsim(sh.g, i, sh.h, tid);
    sh.C[tid] = c;
  }
  __syncthreads();
  for (int q = tid; q < ng * nh; q += 256) {
    const int i = q / nh, j = q - i * nh;
    const unsigned long long qs = hota_qsim(sh.g, i, sh.h, j);
    if (qs == 0) continue;
    const double c = (double)qs / (double)(sh.R[i] + sh.C[j] - qs);      // R_i and C_j both hold qs: the denominator is >= qs
    atomicAdd(&P[t.c0 + (long long)sh.g.trk[i] * t.H + sh.h.trk[j]], hota_q(c));
  }
}

struct HotaMatchShared {
  MotSide g, h;
  int glist[MOT_RMAX], hlist[MOT_RMAX];                  // the rows with a track
  int wsum[4];
  int cnt[HOTA_NA];                                      // the window's pairs with bins = b + 1 ..
  unsigned long long sum[HOTA_NA];                       // .. and the sum of their q(s)
  MotAssign<MOT_RMAX> as;
};

// pass 2: one maximum-score assignment per window, score = gas * s; the assigned pairs are counted per threshold
__global__ __launch_bounds__(256) void hota_match_kernel(const float* __restrict__ gt_rows, const int* __restrict__ gt_track,
                                                         const int* __restrict__ gt_off, int n_gt_rows, const float* __restrict__ hyp_rows,
                                                         const int* __restrict__ hyp_track, const int* __restrict__ hyp_off, int n_hyp_rows,
                                                         int n_windows, const int* __restrict__ gt_trk_off,
                                                         const int* __restrict__ hyp_trk_off, const long long* __restrict__ c_off,
                                                         long long c_total, const unsigned long long* __restrict__ P,
                                                         const int* __restrict__ gc, int n_gt_tracks, const int* __restrict__ tc,
                                                         int n_hyp_tracks, int* __restrict__ hist, long long* __restrict__ tp,
                                                         unsigned long long* __restrict__ loc) {
  __shared__ HotaMatchShared sh;
  const int tid = threadIdx.x, w = blockIdx.x, sess = blockIdx.y;
  const long long k = (long long)sess * n_windows + w;
  int glo, ng, hlo, nh;
  mot_span(gt_off, k, n_gt_rows, glo, ng);
  mot_span(hyp_off, k, n_hyp_rows, hlo, nh);
  if (ng == 0 || nh == 0) return;                        // uniform
  HotaSess t;
  if (!hota_sess(gt_trk_off, hyp_trk_off, c_off, c_total, sess, t) || t.G < 1 || t.H < 1) return;
  if ((long long)t.g0 + t.G > n_gt_tracks || (long long)t.h0 + t.H > n_hyp_tracks) return;
  mot_stage(sh.g, gt_rows, gt_track, glo, ng, t.G);
  mot_stage(sh.h, hyp_rows, hyp_track, hlo, nh, t.H);
  if (tid < HOTA_NA) { sh.cnt[tid] = 0; sh.sum[tid] = 0ull; }
  __syncthreads();
  const int nl = mot_compact(tid < ng && sh.g.trk[tid] >= 0, sh.glist, sh.wsum);
  const int ml = mot_compact(tid < nh && sh.h.trk[tid] >= 0, sh.hlist, sh.wsum);
  if (nl == 0 || ml == 0) return;                        // uniform
  const unsigned long long* Ps = P + t.c0;
  const int* gcs = gc + t.g0;
  const int* tcs = tc + t.h0;
  const int H = t.H;
  // hota_sim(g, h) is the expression's order in every use: the functor of the transposed problem swaps its indices back
  auto score = [&](int i, int j) -> double {
    const float s = hota_sim(sh.g, i, sh.h, j);
    if (!(s > 0.f)) return 0.0;
    const int g = sh.g.trk[i], h = sh.h.trk[j];
    return hota_score(Ps[(long long)g * H + h], gcs[g], tcs[h], s);
  };
  bool any = false;
  if (tid < nl) {
    const int i = sh.glist[tid];
    for (int c = 0; c < ml && !any; ++c) any = score(i, sh.hlist[c]) > 0.0;
  }
  if (!__syncthreads_or(any)) return;                    // no pair with a positive score: nothing to assign, nothing to count
  auto count = [&](int i, int j) {
    const float s = hota_sim(sh.g, i, sh.h, j);
    const int b = hota_bins(s);
    if (b < 1) return;
    atomicAdd(&hist[(t.c0 + (long long)sh.g.trk[i] * H + sh.h.trk[j]) * HOTA_NA + (b - 1)], 1);
    atomicAdd(&sh.cnt[b - 1], 1);
    atomicAdd(&sh.sum[b - 1], hota_q((double)s));
  };
  if (nl <= ml) {
    const bool ok = mot_assign<MOT_RMAX>(sh.as, nl, ml, [&](int r, int c) -> double { return -score(sh.glist[r], sh.hlist[c]); });
    if (ok)
      for (int c = tid; c < ml; c += 256) {
        const int r = sh.as.p[c + 1] - 1;
        if (r >= 0) count(sh.glist[r], sh.hlist[c]);
      }
  } else {
    const bool ok = mot_assign<MOT_RMAX>(sh.as, ml, nl, [&](int r, int c) -> double { return -score(sh.glist[c], sh.hlist[r]); });
    if (ok)
      for (int c = tid; c < nl; c += 256) {
        const int r = sh.as.p[c + 1] - 1;
        if (r >= 0) count(sh.glist[c], sh.hlist[r]);
      }
  }
  __syncthreads();
  if (tid < HOTA_NA) {                                   // threshold k counts the pairs with bins > k: a suffix sum
    long long n = 0;
    unsigned long long l = 0;
    for (int b = tid; b < HOTA_NA; ++b) { n += sh.cnt[b]; l += sh.sum[b]; }
    if (n > 0) {
      atomicAdd((unsigned long long*)&tp[(long long)sess * HOTA_NA + tid], (unsigned long long)n);
      atomicAdd(&loc[(long long)sess * HOTA_NA + tid], l);
    }
  }
}

// pass 3: per session and threshold, the three association numerators over the session's cells.  Thread t takes cells t, t + 256, ..;
// one butterfly per wave and a fixed order across the four waves: two runs give the same bits.
__global__ __launch_bounds__(256) void hota_assoc_kernel(const int* __restrict__ hist, const long long* __restrict__ c_off,
                                                         long long c_total, const int* __restrict__ gt_trk_off,
                                                         const int* __restrict__ hyp_trk_off, const int* __restrict__ gc, int n_gt_tracks,
                                                         const int* __restrict__ tc, int n_hyp_tracks, double* __restrict__ out) {
  __shared__ double red[4][HOTA_NA * 3];
  const int tid = threadIdx.x, sess = blockIdx.x;
  HotaSess t;
  bool ok = hota_sess(gt_trk_off, hyp_trk_off, c_off, c_total, sess, t);
  ok = ok && (long long)t.g0 + t.G <= n_gt_tracks && (long long)t.h0 + t.H <= n_hyp_tracks;
  double acc[HOTA_NA][3];
#pragma unroll
  for (int k = 0; k < HOTA_NA; ++k) { acc[k][0] = 0.0; acc[k][1] = 0.0; acc[k][2] = 0.0; }
  const int cells = ok ? t.G * t.H : 0;                  // a session whose tables are wrong reports zeros
  for (int cell = tid; cell < cells; cell += 256) {
    const int g = cell / t.H, h = cell - g * t.H;
    const int* hb = hist + (t.c0 + cell) * HOTA_NA;
    const long long a = gc[t.g0 + g], b = tc[t.h0 + h];
    long long mc = 0;
#pragma unroll
    for (int k = HOTA_NA - 1; k >= 0; --k) {
      mc += hb[k];
      if (mc > 0 && a > 0 && b > 0 && a + b - mc > 0) {
        const double m2 = (double)mc * (double)mc;
        acc[k][0] += m2 / (double)(a + b - mc);
        acc[k][1] += m2 / (double)a;
        acc[k][2] += m2 / (double)b;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < HOTA_NA; ++k) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const double v = wave_sum_d(acc[k][q]);
      if ((tid & 63) == 0) red[tid >> 6][k * 3 + q] = v;
    }
  }
  __syncthreads();
  if (tid < HOTA_NA * 3) out[(size_t)sess * (HOTA_NA * 3) + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

static bool hota_tables_ok(long long c_total, int max_tracks, long long n_gt_tracks, long long n_hyp_tracks) {
  if (c_total < 1 || c_total * HOTA_NA > (1ll << 28) || max_tracks < 1 || max_tracks > MOT_TMAX) return false;
  return n_gt_tracks >= 0 && n_hyp_tracks >= 0 && n_gt_tracks <= 0x07ffffffll && n_hyp_tracks <= 0x07ffffffll;
}

extern "C" int mmd_hota_align(const float* gt_rows, const int* gt_track, const int* gt_off, long long n_gt_rows, const float* hyp_rows,
                              const int* hyp_track, const int* hyp_off, long long n_hyp_rows, int n_sessions, int n_windows,
                              const int* gt_trk_off, const int* hyp_trk_off, int max_tracks, const long long* c_off, long long c_total,
                              unsigned long long* P, hipStream_t stream) {
  if (!gt_off || !hyp_off || !gt_trk_off || !hyp_trk_off || !c_off || !P) return MMD_EINVAL;
  if (!mot_sizes_ok(n_gt_rows, n_hyp_rows, n_sessions, n_windows) || n_windows > (1 << 20) || !hota_tables_ok(c_total, max_tracks, 0, 0))
    return MMD_EINVAL;
  if ((n_gt_rows > 0 && (!gt_rows || !gt_track)) || (n_hyp_rows > 0 && (!hyp_rows || !hyp_track))) return MMD_EINVAL;
  hipLaunchKernelGGL(hota_align_kernel, dim3(n_windows, n_sessions), dim3(256), 0, stream, gt_rows, gt_track, gt_off, (int)n_gt_rows,
                     hyp_rows, hyp_track, hyp_off, (int)n_hyp_rows, n_windows, gt_trk_off, hyp_trk_off, c_off, c_total, P);
  return mmd_check_launch();
}

extern "C" int mmd_hota_match(const float* gt_rows, const int* gt_track, const int* gt_off, long long n_gt_rows, const float* hyp_rows,
                              const int* hyp_track, const int* hyp_off, long long n_hyp_rows, int n_sessions, int n_windows,
                              const int* gt_trk_off, const int* hyp_trk_off, int max_tracks, const long long* c_off, long long c_total,
                              const unsigned long long* P, const int* gc, long long n_gt_tracks, const int* tc, long long n_hyp_tracks,
                              int* hist, long long* tp, unsigned long long* loc, hipStream_t stream) {
  if (!gt_off || !hyp_off || !gt_trk_off || !hyp_trk_off || !c_off || !P || !gc || !tc || !hist || !tp || !loc) return MMD_EINVAL;
  if (!mot_sizes_ok(n_gt_rows, n_hyp_rows, n_sessions, n_windows) || n_windows > (1 << 20) ||
      !hota_tables_ok(c_total, max_tracks, n_gt_tracks, n_hyp_tracks))
    return MMD_EINVAL;
  if ((n_gt_rows > 0 && (!gt_rows || !gt_track)) || (n_hyp_rows > 0 && (!hyp_rows || !hyp_track))) return MMD_EINVAL;
  hipLaunchKernelGGL(hota_match_kernel, dim3(n_windows, n_sessions), dim3(256), 0, stream, gt_rows, gt_track, gt_off, (int)n_gt_rows,
                     hyp_rows, hyp_track, hyp_off, (int)n_hyp_rows, n_windows, gt_trk_off, hyp_trk_off, c_off, c_total, P, gc,
                     (int)n_gt_tracks, tc, (int)n_hyp_tracks, hist, tp, loc);
  return mmd_check_launch();
}

extern "C" int mmd_hota_assoc(const int* hist, const long long* c_off, long long c_total, const int* gt_trk_off, const int* hyp_trk_off,
                              const int* gc, long long n_gt_tracks, const int* tc, long long n_hyp_tracks, int n_sessions, int max_tracks,
                              double* num, hipStream_t stream) {
  if (!hist || !c_off || !gt_trk_off || !hyp_trk_off || !gc || !tc || !num) return MMD_EINVAL;
  if (n_sessions < 1 || n_sessions > 65535 || !hota_tables_ok(c_total, max_tracks, n_gt_tracks, n_hyp_tracks)) return MMD_EINVAL;
  hipLaunchKernelGGL(hota_assoc_kernel, dim3(n_sessions), dim3(256), 0, stream, hist, c_off, c_total, gt_trk_off, hyp_trk_off, gc,
                     (int)n_gt_tracks, tc, (int)n_hyp_tracks, num);
  return mmd_check_launch();
}
