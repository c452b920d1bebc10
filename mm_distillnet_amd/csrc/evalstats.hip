// Device-side detection statistics of the evaluation (no per-batch host sync) — CDNA4 / gfx950.
//   get_batch_statistics ........ src/utils/utils.py:1058-1136 (prediction -> best ground-truth box, true positives per IoU threshold)
//   get_batch_central_distances . src/utils/utils.py:979-1055  (per ground-truth box the closest unused same-class prediction's extent)
//   bbox_iou (+1 pixel) ......... src/utils/utils.py:1139-1185
// as mm_distillnet_amd/metrics.py restates them; the results are meant to be bit-identical to that host path, so every fp32 operation is
// explicitly rounded (no FMA contraction, IEEE division) and keeps the reference's operation order, the 1e-16 of the denominator included
// (it is absorbed unless a1 + a2 - inter is exactly 0, where it turns 0 / 0 into 0).
//
// One 256-thread block per image:
//   phase 1, all threads, one prediction each: IoU against every box -> (best IoU, first best index), or index -1 when no box has the
//            prediction's class.  The match does not depend on the threshold, so it is computed once, not nine times.
//   phase 2, wave 0: the greedy walk over the predictions in their given order.  Lane k < 9 owns threshold k and its own "taken" bit set;
//            the nine walks run in lockstep, 64 predictions are fetched per step and handed round by __shfl, a __ballot collects the
//            9-bit mask.  (The reference's early stop - all boxes taken - changes no result: a taken box never matches again.  Here it
//            skips the rest of the walk once all nine thresholds are through.)
//            wave 1, at the same time: the central distances, boxes in order, lanes over the predictions, (distance, index) min by
//            __shfl_xor; each lane owns the "used" marks of its own predictions, so the marks need no cross-lane ordering.
// Images of up to EV_NP predictions and EV_NG boxes keep all of this in LDS (~30 KB); beyond that the same code runs on the caller's
// workspace (mmd_eval_ws_floats) and reads the boxes from global memory - correct for any count the arrays can hold, and slow: the walk
// and the distance search are sequential by definition (n and g * n / 64 steps of one wave).
//
// Record (caller-owned, device): rows (score, class) + 9-bit TP mask, appended in image then prediction order; per image
// (sum dx, sum dy, n_boxes); the flat list of ground-truth classes.  A batch's offsets are prefix sums over the images' counts on top of
// cursor[3] = {rows, images, classes}; a second one-block launch advances the cursor behind the batch (stream order, no atomics).
#include "common.h"
// hipcc's default is -ffp-contract=fast, and its __fmul_rn / __fadd_rn are inline operators that carry that default with them: the
// squared distance below, written with them, compiled to v_fmac_f32.  So contraction is off for this file and the arithmetic goes
// through local operators; `/` is the correctly rounded division (v_div_scale / v_div_fmas / v_div_fixup), hipcc's default for fp32.
#pragma clang fp contract(off)
__device__ __forceinline__ float ev_add(float x, float y) { return x + y; }
__device__ __forceinline__ float ev_sub(float x, float y) { return x - y; }
__device__ __forceinline__ float ev_mul(float x, float y) { return x * y; }
__device__ __forceinline__ float ev_div(float x, float y) { return x / y; }

#define EV_NP 1024         // predictions per image the LDS path holds
#define EV_NG 256           // ground-truth boxes per image the LDS path holds
#define EV_NT 9             // IoU thresholds 0.50 ... 0.90
#define EV_TW(g) (((g) + 31) >> 5)

// fp32(around(0.5 + 0.05 k, 2)): the double literal rounded to float, as numpy rounds the threshold metrics.py compares with
__device__ const float EV_THR[EV_NT] = {(float)0.5, (float)0.55, (float)0.6, (float)0.65, (float)0.7, (float)0.75, (float)0.8, (float)0.85, (float)0.9};

struct EvalArgs {
  const float* rows; const int* cnt; int cap;
  const float* boxes; const int* nbox; int G; int B;
  float* rec_rows; int* rec_tp; int max_rows;
  float* rec_cd; int max_images;
  float* rec_gt; int max_gt;
  int* cursor; float* ws; long long ws_stride; int* overflow;
};

__device__ __forceinline__ int ev_cnt(const int* c, int i, int cap) { return max(0, min(c[i], cap)); }
__device__ __forceinline__ int ev_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void eval_match_kernel(EvalArgs a) {
  __shared__ float s_box[EV_NG * 5];
  __shared__ float s_pred[EV_NP * 6];      // biou | bidx | pw | ph | pcl | used
  __shared__ unsigned s_taken[EV_NT * EV_TW(EV_NG)];
  __shared__ int s_base[2];
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int n = ev_cnt(a.cnt, b, a.cap), g = ev_cnt(a.nbox, b, a.G);
  // ---- where this image's rows and classes go: the counts of the images in front of it
  if (wave == 0) {
    int r0 = 0, g0 = 0;
    for (int i = lane; i < b; i += 64) {
      const int ni = ev_cnt(a.cnt, i, a.cap), gi = ev_cnt(a.nbox, i, a.G);
      if (ni > 0 && gi > 0) r0 += ni;
      g0 += gi;
    }
    r0 = ev_wave_sum(r0); g0 = ev_wave_sum(g0);
    if (lane == 0) { s_base[0] = r0; s_base[1] = g0; }
  }
  __syncthreads();
  const long long row0 = (long long)a.cursor[0] + s_base[0], gt0 = (long long)a.cursor[2] + s_base[1];
  const long long img = (long long)a.cursor[1] + b;
  const float* rows = a.rows + (size_t)b * a.cap * 6;
  const float* gbox = a.boxes + (size_t)b * a.G * 5;
  const bool match = n > 0 && g > 0;
  if (tid == 0 && ((match && row0 + n > a.max_rows) || gt0 + g > a.max_gt || img >= a.max_images)) *a.overflow = 1;
  for (int i = tid; i < g; i += 256)
    if (gt0 + i < a.max_gt) a.rec_gt[gt0 + i] = gbox[i * 5 + 4];
  if (g == 0) {           // no ground truth: no statistics, no distances; the image keeps its slot (n_boxes = 0)
    if (tid == 0 && img < a.max_images) { float* o = a.rec_cd + img * 3; o[0] = 0.f; o[1] = 0.f; o[2] = 0.f; }
    return;
  }
  // ---- LDS or workspace
  const bool lds = n <= EV_NP && g <= EV_NG;
  float* pw_ = lds ? s_pred : a.ws + (size_t)b * a.ws_stride;
  const int np = lds ? EV_NP : a.cap;
  float* biou = pw_; int* bidx = reinterpret_cast<int*>(pw_ + np);
  float* pw = pw_ + 2 * (size_t)np; float* ph = pw_ + 3 * (size_t)np; float* pcl = pw_ + 4 * (size_t)np;
  int* used = reinterpret_cast<int*>(pw_ + 5 * (size_t)np);
  unsigned* taken = lds ? s_taken : reinterpret_cast<unsigned*>(pw_ + 6 * (size_t)np);
  const int tw = EV_TW(g);
  const float* box = gbox;
  if (lds) {
    for (int e = tid; e < g * 5; e += 256) s_box[e] = gbox[e];
    box = s_box;
  }
  for (int e = tid; e < EV_NT * tw; e += 256) taken[e] = 0u;
  __syncthreads();
  // ---- phase 1: one prediction per thread
  for (int p = tid; p < n; p += 256) {
    const float* r = rows + (size_t)p * 6;
    const float x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3], pc = r[5];
    const float a1 = ev_mul(ev_add(ev_sub(x2, x1), 1.f), ev_add(ev_sub(y2, y1), 1.f));
    float best = -INFINITY; int bi = 0; bool has = false;
    for (int j = 0; j < g; ++j) {
      const float* q = box + j * 5;
      const float bx1 = q[0], by1 = q[1], bx2 = q[2], by2 = q[3];
      has |= (q[4] == pc);
      const float iw = fmaxf(ev_add(ev_sub(fminf(x2, bx2), fmaxf(x1, bx1)), 1.f), 0.f);
      const float ih = fmaxf(ev_add(ev_sub(fminf(y2, by2), fmaxf(y1, by1)), 1.f), 0.f);
      const float inter = ev_mul(iw, ih);
      const float a2 = ev_mul(ev_add(ev_sub(bx2, bx1), 1.f), ev_add(ev_sub(by2, by1), 1.f));
      const float iou = ev_div(inter, ev_add(ev_sub(ev_add(a1, a2), inter), 1e-16f));
      if (iou > best) { best = iou; bi = j; }      // strict: the first index wins ties
    }
    biou[p] = best; bidx[p] = has ? bi : -1;
    pw[p] = ev_sub(x2, x1); ph[p] = ev_sub(y2, y1); pcl[p] = pc; used[p] = 0;
    if (row0 + p < a.max_rows) { float* o = a.rec_rows + (row0 + p) * 2; o[0] = r[4]; o[1] = pc; }
  }
  __syncthreads();      // (orders the workspace path's global stores too: workgroup scope)
  // waves 2 and 3 are done: the walk and the distance search are one wave each, side by side
  if (wave == 0 && match) {
    // ---- phase 2: nine greedy walks in lockstep
    const float thr = EV_THR[lane < EV_NT ? lane : 0];
    unsigned* mine = taken + (lane < EV_NT ? lane : 0) * tw;
    int ntaken = 0;
    for (int p0 = 0; p0 < n; p0 += 64) {
      const int p = p0 + lane;
      int mask = 0;
      if (__ballot(lane < EV_NT && ntaken < g) != 0ull) {
        const float my_iou = p < n ? biou[p] : 0.f;
        const int my_bi = p < n ? bidx[p] : -1;
        const int m = min(64, n - p0);
        for (int j = 0; j < m; ++j) {
          const float iou = __shfl(my_iou, j, 64);
          const int bi = __shfl(my_bi, j, 64);
          bool tp = false;
          if (lane < EV_NT && bi >= 0 && iou >= thr) {
            const unsigned w = mine[bi >> 5], bit = 1u << (bi & 31);
            if (!(w & bit)) { mine[bi >> 5] = w | bit; ++ntaken; tp = true; }
          }
          const unsigned long long hits = __ballot(tp);
          if (lane == j) mask = (int)(hits & 0x1ffull);
        }
      }
      if (p < n && row0 + p < a.max_rows) a.rec_tp[row0 + p] = mask;
    }
  } else if (wave == 1) {
    // ---- central distances
    float sdx = 0.f, sdy = 0.f;
    for (int i = 0; i < g; ++i) {
      const float* q = box + i * 5;
      const float tx = ev_sub(q[2], q[0]), ty = ev_sub(q[3], q[1]), tc = q[4];
      float dx, dy;
      if (n == 0) {         // compared against zeros: as many class-0, zero-extent predictions as there are boxes
        dx = tc == 0.f ? fabsf(tx) : tx; dy = tc == 0.f ? fabsf(ty) : ty;
      } else {
        float bd = INFINITY; int bp = 0x7fffffff;
        for (int p = lane; p < n; p += 64) {
          if (used[p] || pcl[p] != tc) continue;
          const float ex = ev_sub(pw[p], tx), ey = ev_sub(ph[p], ty);
          const float d = ev_add(ev_mul(ex, ex), ev_mul(ey, ey));
          if (bp == 0x7fffffff || d < bd) { bd = d; bp = p; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const float od = __shfl_xor(bd, o, 64); const int op = __shfl_xor(bp, o, 64);
          if (op != 0x7fffffff && (bp == 0x7fffffff || od < bd || (od == bd && op < bp))) { bd = od; bp = op; }
        }
        if (bp == 0x7fffffff) { dx = tx; dy = ty; }      // no same-class prediction left: the box's own extent (signed, as upstream)
        else {
          dx = fabsf(ev_sub(tx, pw[bp])); dy = fabsf(ev_sub(ty, ph[bp]));
          if ((bp & 63) == lane) used[bp] = 1;
        }
      }
      sdx = ev_add(sdx, dx); sdy = ev_add(sdy, dy);
    }
    if (lane == 0 && img < a.max_images) { float* o = a.rec_cd + img * 3; o[0] = sdx; o[1] = sdy; o[2] = (float)g; }
  }
}

__global__ __launch_bounds__(64) void eval_advance_kernel(EvalArgs a) {
  const int lane = threadIdx.x;
  long long r = 0, g = 0;
  for (int i = lane; i < a.B; i += 64) {
    const int ni = ev_cnt(a.cnt, i, a.cap), gi = ev_cnt(a.nbox, i, a.G);
    if (ni > 0 && gi > 0) r += ni;
    g += gi;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { r += __shfl_xor(r, o, 64); g += __shfl_xor(g, o, 64); }
  if (lane == 0) {      // clamped: after an overflow the cursor stays at the capacity, later batches append nothing
    a.cursor[0] = (int)min((long long)a.max_rows, a.cursor[0] + r);
    a.cursor[1] = (int)min((long long)a.max_images, (long long)a.cursor[1] + a.B);
    a.cursor[2] = (int)min((long long)a.max_gt, a.cursor[2] + g);
  }
}

// floats of workspace PER IMAGE for arrays of cap predictions and G boxes per image (0: every image fits the LDS path); -22 when the
// size does not fit an int
extern "C" int mmd_eval_ws_floats(int cap, int G) {
  if (cap <= 0 || G <= 0) return MMD_EINVAL;
  if (cap <= EV_NP && G <= EV_NG) return 0;
  const long long n = (6ll * cap + (long long)EV_NT * EV_TW((long long)G) + 3) / 4 * 4;
  return n > 0x7fffffffll ? MMD_EINVAL : (int)n;
}
// which = 0: predictions, 1: boxes per image up to which an image stays on the LDS path
extern "C" int mmd_eval_lds_cap(int which) { return which == 0 ? EV_NP : (which == 1 ? EV_NG : MMD_EINVAL); }

extern "C" int mmd_eval_match(const float* rows, const int* cnt, int cap, const float* boxes, const int* nbox, int G, int B,
                              float* rec_rows, int* rec_tp, int max_rows, float* rec_cd, int max_images, float* rec_gt, int max_gt,
                              int* cursor, float* ws, int* overflow, hipStream_t stream) {
  if (!rows || !cnt || !boxes || !nbox || !rec_rows || !rec_tp || !rec_cd || !rec_gt || !cursor || !overflow) return MMD_EINVAL;
  if (B <= 0 || cap <= 0 || G <= 0 || max_rows <= 0 || max_images <= 0 || max_gt <= 0) return MMD_EINVAL;
  const int wsf = mmd_eval_ws_floats(cap, G);
  if (wsf < 0 || (wsf > 0 && !ws)) return MMD_EINVAL;
  EvalArgs a{rows, cnt, cap, boxes, nbox, G, B, rec_rows, rec_tp, max_rows, rec_cd, max_images, rec_gt, max_gt, cursor, ws, wsf, overflow};
  hipLaunchKernelGGL(eval_match_kernel, dim3(B), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(eval_advance_kernel, dim3(1), dim3(64), 0, stream, a);
  return mmd_check_launch();
}
