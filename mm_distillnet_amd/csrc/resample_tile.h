// The tile of the polyphase resampler, shared by mmd_resample_poly (resample.hip: a whole recording) and mmd_ring_resample (live.hip: a
// range of outputs from a ring of inputs into a ring of outputs).  Both plan their blocks with rs_plan and run the tap loop of
// rs_tile_taps on a staged input span, so for equal inputs they form equal fmaf chains: the same bits.  They differ only in how the
// span is staged (a linear row, or a ring that wraps) and where an output is stored.  The rule, the bank's layout and the shape of a
// block are described at the top of resample.hip.
#pragma once
#include "common.h"

#define RS_THREADS 256
#define RS_QT 4                                      // periods per thread
#define RS_PHMAX 64                                  // phases per block at most
#define RS_LDS_FLOATS 12288                          // staged input span at most (48 KB)
#define RS_FMAX 1024                                 // L, M at most
#define RS_TAPS_MAX 4096
#define RS_ROWS_MAX 65535                            // rows ride in gridDim.z

struct RsPlan { int PH, PS, QB, dbound, span; };

// dbound: phase_off[b] - phase_off[a] = floor(b M / L) - floor(a M / L) <= floor((b - a) M / L) + 1 for the PH phases of a tile.
// lds: floats the staged span may take, at least rs_min_span (mmd_ring_resample: no more than its input ring holds, so that the
// staging loads wrap once; the periods per block do not enter any output's sum).
static inline RsPlan rs_plan(int L, int M, int taps, long long n_periods, long long lds = RS_LDS_FLOATS) {
  RsPlan p;
  const int ntile = cdiv(L, RS_PHMAX);
  p.PH = cdiv(L, ntile);
  p.PS = RS_THREADS / p.PH;
  p.dbound = (int)(((long long)(p.PH - 1) * M) / L) + 1;
  long long qb = (lds - taps - p.dbound) / M + 1;                    // >= 1: taps + dbound <= 4096 + 1024 < RS_LDS_FLOATS
  if (qb > (long long)p.PS * RS_QT) qb = (long long)p.PS * RS_QT;
  if (qb > n_periods) qb = n_periods;
  p.QB = (int)qb;
  p.span = (p.QB - 1) * M + p.dbound + taps;
  return p;
}

// the span of a block of ONE period: the least a plan stages
static inline int rs_min_span(int L, int M, int taps) { return rs_plan(L, M, taps, 1).span; }

static inline bool rs_factors_ok(int L, int M, int taps) {
  return L >= 1 && L <= RS_FMAX && M >= 1 && M <= RS_FMAX && !(taps & 1) && taps >= 2 && taps <= RS_TAPS_MAX;
}

// Thread (ph, pq) = (tid % PH, tid / PH) of the block whose tile starts at output phase r0 (off0 = phase_off[r0]): acc[i] = the output
// of phase r0 + ph in the tile's period pq + i * PS, from s_x[0 .. pl.span) = the inputs from (first period) * M + off0 - taps / 2 + 1
// on.  acc = 0, then acc = fmaf(w, x, acc) over all taps in tap order.  The table is the caller's: its differences are clamped into
// the staged span (a bad table gives wrong samples, never a read outside the tile), idle threads read the tile's first taps.
// -> whether this thread's phase exists; output i exists where also pq + i * PS < pl.QB.
__device__ __forceinline__ bool rs_tile_taps(const float* s_x, const float* __restrict__ bank, const int* __restrict__ phase_off, int L, int M,
                                             int taps, const RsPlan& pl, int r0, int off0, float (&acc)[RS_QT]) {
  const int tid = threadIdx.x;
  const int ph = tid % pl.PH, pq = tid / pl.PH;
  const int r = min(r0 + ph, L - 1);
  const bool lane_ok = r0 + ph < L && pq < pl.PS;
  const int d = min(max(phase_off[r] - off0, 0), pl.dbound);
  int base[RS_QT];
#pragma unroll
  for (int i = 0; i < RS_QT; ++i) {
    const int qi = pq + i * pl.PS;
    base[i] = (lane_ok && qi < pl.QB) ? qi * M + d : 0;
    acc[i] = 0.f;
  }
  const float* b = bank + r;
#pragma unroll 4
  for (int j = 0; j < taps; ++j) {
    const float w = b[(size_t)j * L];
#pragma unroll
    for (int i = 0; i < RS_QT; ++i) acc[i] = fmaf(w, s_x[base[i] + j], acc[i]);
  }
  return lane_ok;
}
