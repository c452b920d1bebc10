// The optimal assignment of the tracking evaluation (moteval.hip: CLEAR-MOT, identity, HOTA) and of the tracker's optimal association
// rule (track.hip, assign = 1): ONE routine, mot_assign, and the block-wide compaction its callers list their rows with.  Callers run
// one 256-thread block and keep a MotAssign<CAP> in LDS (CAP = 256: 9300 bytes).
#pragma once
#include "common.h"

#define MOT_INF 1.0e300

// ---- the assignment ------------------------------------------------------------------------------------------------------------------
template <int CAP>
struct MotAssign {
  double u[CAP + 1];          // row potentials, 1-based (u[0] unused)
  double v[CAP + 1];          // column potentials, 1-based
  double minv[CAP + 1];
  int way[CAP + 1];
  int p[CAP + 1];             // p[j]: the row matched to column j (1-based; 0: none); p[0]: the row being inserted
  int used[CAP + 1];
  double wv[4];               // the four waves' minima
  int wj[4];
};

// n x m, 1 <= n <= m <= CAP, cost(row, column) with 0-based indices, finite.  Called by all 256 threads; on return (behind a
// __syncthreads) L.p[1 .. m] holds the optimum.  Returns false - uniformly, and only for costs that are not finite - when a step
// finds no column: the matching in L.p is then not to be used.
template <int CAP, class Cost>
__device__ __forceinline__ bool mot_assign(MotAssign<CAP>& L, int n, int m, Cost cost) {
  const int tid = threadIdx.x;
  for (int j = tid; j <= m; j += 256) { L.u[j] = 0.0; L.v[j] = 0.0; L.p[j] = 0; }
  __syncthreads();
  for (int i = 1; i <= n; ++i) {
    if (tid == 0) L.p[0] = i;
    for (int j = 1 + tid; j <= m; j += 256) { L.minv[j] = MOT_INF; L.used[j] = 0; }
    int j0 = 0;
    __syncthreads();
    for (;;) {
      const int i0 = L.p[j0];
      const double ui0 = L.u[i0];
      double bv = MOT_INF;
      int bj = 0x7fffffff;
      for (int j = 1 + tid; j <= m; j += 256) {
        if (j == j0) L.used[j] = 1;                      // the owner marks the column that just joined the tree
        if (L.used[j]) continue;
        const double cur = cost(i0 - 1, j - 1) - ui0 - L.v[j];
        double mv = L.minv[j];
        if (cur < mv) { mv = cur; L.minv[j] = cur; L.way[j] = j0; }
        if (mv < bv) { bv = mv; bj = j; }                // own columns rise: the first minimum is the lowest column
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(bv, o, 64);
        const int oj = __shfl_xor(bj, o, 64);
        if (ov < bv || (ov == bv && oj < bj)) { bv = ov; bj = oj; }
      }
      if ((tid & 63) == 0) { L.wv[tid >> 6] = bv; L.wj[tid >> 6] = bj; }
      __syncthreads();
      double delta = L.wv[0];
      int j1 = L.wj[0];
#pragma unroll
      for (int w = 1; w < 4; ++w) {
        const double ov = L.wv[w];
        const int oj = L.wj[w];
        if (ov < delta || (ov == delta && oj < j1)) { delta = ov; j1 = oj; }
      }
      if (j1 > m) return false;                          // uniform: every thread read the same eight words
      for (int j = 1 + tid; j <= m; j += 256) {
        if (L.used[j]) { L.u[L.p[j]] += delta; L.v[j] -= delta; }      // the used columns' rows are distinct
        else L.minv[j] -= delta;
      }
      if (tid == 0) L.u[i] += delta;                     // column 0 of the tree: the row being inserted
      j0 = j1;
      __syncthreads();                                   // the potentials are visible, every thread is done with wv / wj
      if (L.p[j0] == 0) break;                           // uniform: a free column ends the path
    }
    if (tid == 0) {
      do {
        const int j1 = L.way[j0];
        L.p[j0] = L.p[j1];
        j0 = j1;
      } while (j0);
    }
    __syncthreads();
  }
  return true;
}

// The indices i < n with flag set, in rising order -> list[0 .. count-1]; returns count (uniform).  n <= 256.  Ends with a __syncthreads.
__device__ __forceinline__ int mot_compact(bool flag, int* __restrict__ list, int* __restrict__ wsum) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const unsigned long long b = __ballot(flag);
  const int before = __popcll(b & ((1ull << lane) - 1ull));
  if (lane == 0) wsum[w] = __popcll(b);
  __syncthreads();
  int base = 0, total = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = wsum[k];
    if (k < w) base += c;
    total += c;
  }
  if (flag) list[base + before] = tid;
  __syncthreads();
  return total;
}
