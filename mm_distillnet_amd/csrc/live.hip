// Live streaming detection: the writers of the device sample ring that AudioDetector.open_stream's session reads its windows from.
//
// The ring is ring[channels, cap] float32 at a FIXED address: absolute sample p of the session (int64, counted from its start) of channel
// c lives at ring[c * cap + p % cap].  Chunks arrive a few milliseconds at a time (mmd_ring_push: float rows; mmd_ring_push_pcm: a WAV's
// interleaved frames as read), the front end reads whole windows back out of it across the wrap (mmd_melspec_windows_ring, melspec.hip),
// and because the address never changes one captured hipGraph of the detection chain serves every group of every session of one geometry.
//
// Both writers reduce pos modulo cap ONCE, on the host; a launch writes n <= cap consecutive positions, so a position wraps at most once:
// one compare and one subtract per store, no division on the device.  Lanes of a wave store consecutive floats; where the run crosses
// the ring's end the wave splits into two contiguous runs.  Plain vector stores, no atomics: nothing but the n slots per channel is
// touched, and which sample is overwritten is the caller's schedule (mm_distillnet_amd.audio.live_schedule).
//
// A session whose source is not at 44.1 kHz keeps a SECOND ring, of input-rate samples, in front of that one: the two writers fill it
// and mmd_ring_resample (below) computes the 44.1 kHz samples the schedule asks for from it into the first.
#include "common.h"
#include "pcm_tile.h"
#include "resample_tile.h"

#define RING_THREADS 256
#define RING_PER_THREAD 4
#define RING_MAX (1ll << 50)                         // cap and pos at most: pos + n stays far inside int64

// blockIdx.y = channel; a block owns 1024 consecutive samples, thread t samples t, t + 256, t + 512, t + 768 of them
__global__ __launch_bounds__(RING_THREADS) void ring_push_kernel(const float* __restrict__ src, long long src_stride, long long n,
                                                                 float* __restrict__ ring, long long cap, long long p0) {
  src += (size_t)blockIdx.y * (size_t)src_stride;
  ring += (size_t)blockIdx.y * (size_t)cap;
  const long long i0 = (long long)blockIdx.x * (RING_THREADS * RING_PER_THREAD) + threadIdx.x;
#pragma unroll
  for (int k = 0; k < RING_PER_THREAD; ++k) {
    const long long i = i0 + RING_THREADS * k;
    if (i < n) {
      long long d = p0 + i;                          // < 2 * cap: p0 < cap, i < n <= cap
      d = d >= cap ? d - cap : d;
      ring[d] = src[i];
    }
  }
}

extern "C" int mmd_ring_push(const float* src, long long src_stride, int channels, long long n, float* ring, long long cap, long long pos,
                             hipStream_t stream) {
  if (!src || !ring || channels < 1 || channels > 65535 || n < 1 || n > cap || cap > RING_MAX || pos < 0 || pos > RING_MAX ||
      src_stride < n)
    return MMD_EINVAL;
  const long long blocks = (n + RING_THREADS * RING_PER_THREAD - 1) / (RING_THREADS * RING_PER_THREAD);
  if (blocks > 0x7fffffffll) return MMD_EINVAL;
  hipLaunchKernelGGL(ring_push_kernel, dim3((unsigned)blocks, channels), dim3(RING_THREADS), 0, stream, src, src_stride, n, ring, cap,
                     pos % cap);
  return mmd_check_launch();
}

// mmd_pcm_to_float's tile (pcm_tile.h: the same staging and decoding, so the same floats) with row c = ring[c, :] and the column
// p0 + frame wrapped once
__global__ __launch_bounds__(PCM_THREADS) void ring_push_pcm_kernel(const unsigned char* __restrict__ pcm, long long frames, int channels,
                                                                    int width, int F, float* __restrict__ ring, long long cap,
                                                                    long long p0) {
  pcm_tile_to_rows(pcm, frames, channels, width, F, ring, cap, p0, cap);
}

extern "C" int mmd_ring_push_pcm(const unsigned char* pcm, long long frames, int channels, int width, float* ring, long long cap,
                                 long long pos, hipStream_t stream) {
  if (!pcm || !ring || frames < 1 || channels < 1 || (width != 2 && width != 3 && width != 4)) return MMD_EINVAL;
  if (frames > cap || cap > RING_MAX || pos < 0 || pos > RING_MAX) return MMD_EINVAL;
  const int F = pcm_tile_frames(channels, width);
  if (F < 1) return MMD_EINVAL;
  const long long blocks = (frames + F - 1) / F;
  if (blocks > 0x7fffffffll) return MMD_EINVAL;
  hipLaunchKernelGGL(ring_push_pcm_kernel, dim3((unsigned)blocks), dim3(PCM_THREADS), 0, stream, pcm, frames, channels, width, F, ring,
                     cap, pos % cap);
  return mmd_check_launch();
}

// ---- resampling from a ring into a ring: mmd_resample_poly's rule (resample.hip) for the outputs t_lo .. t_hi-1 of a recording of which
// only the last in_cap input samples are resident.  Output t = q * L + r needs the inputs q * M + phase_off[r] - half + 1 .. + half and
// nothing else, so a bounded history gives the offline kernel's sums: the block shape, the plan and the tap loop are that kernel's
// (resample_tile.h: one fmaf chain over all taps in tap order, zeros - multiplied, not skipped - outside 0 .. n_valid-1).
//
// What differs.  (1) [t_lo, t_hi) is not period-aligned: the grid covers the periods q_lo = t_lo / L .. (t_hi - 1) / L and the stores
// outside the range are masked.  (2) Staging reads the input ring, and a block stages no more than the ring holds
// (the plan's periods per block shrink with in_cap, down to one), so its loads wrap at most once.  The resident samples are the absolute positions v_lo .. n_valid-1
// with v_lo = max(0, n_valid - in_cap); the host reduces v_lo modulo in_cap ONCE, and a position g in that range lies d = g - v_lo <
// in_cap slots behind it: one compare and one subtract per load, and whatever is outside the range - before the recording, behind what
// was pushed, or overwritten - is staged as zero, so no load leaves the ring whatever range is asked for.  (3) Stores go to the output
// ring at (t_lo % out_cap) + (t - t_lo), t_lo % out_cap from the host and t - t_lo < out_cap: they wrap once.  Only q * M, q * L and
// the row offsets are 64-bit; nothing is divided on the device.
struct RingRs {
  long long q_lo;                                    // first period of the grid
  long long rel_lo, rel_hi;                          // t_lo - q_lo * L (< L), t_hi - q_lo * L: the range in outputs counted from q_lo * L
  long long v_lo, n_valid, s_lo;                     // resident inputs [v_lo, n_valid); s_lo = v_lo % in_cap
  long long in_cap, out_cap, o_lo;                   // o_lo = t_lo % out_cap
};

__global__ __launch_bounds__(RS_THREADS) void ring_resample_kernel(const float* __restrict__ in_ring, const float* __restrict__ bank,
                                                                   const int* __restrict__ phase_off, int L, int M, int taps,
                                                                   float* __restrict__ out_ring, RingRs a, RsPlan pl) {
  extern __shared__ float s_x[];                     // pl.span floats
  const int tid = threadIdx.x;
  const int r0 = blockIdx.y * pl.PH;                 // < L: gridDim.y = cdiv(L, PH)
  const long long qb0 = (long long)blockIdx.x * pl.QB;               // the tile's first period, counted from q_lo
  in_ring += (size_t)blockIdx.z * (size_t)a.in_cap;
  out_ring += (size_t)blockIdx.z * (size_t)a.out_cap;

  // ---- stage the tile's input span; s_x[i] = x[g0 + i], zero where g0 + i is not resident
  const int off0 = phase_off[r0];
  const long long g0 = (a.q_lo + qb0) * M + off0 - (taps >> 1) + 1;
  for (int i = tid; i < pl.span; i += RS_THREADS) {
    const long long g = g0 + i;
    float v = 0.f;
    if (g >= a.v_lo && g < a.n_valid) {
      long long s = a.s_lo + (g - a.v_lo);           // < 2 * in_cap: s_lo < in_cap, g - v_lo < n_valid - v_lo <= in_cap
      s = s >= a.in_cap ? s - a.in_cap : s;
      v = in_ring[s];
    }
    s_x[i] = v;
  }
  __syncthreads();

  float acc[RS_QT];
  const bool lane_ok = rs_tile_taps(s_x, bank, phase_off, L, M, taps, pl, r0, off0, acc);
  const int ph = tid % pl.PH, pq = tid / pl.PH;
#pragma unroll
  for (int i = 0; i < RS_QT; ++i) {
    const int qi = pq + i * pl.PS;
    const long long rel = (qb0 + qi) * L + r0 + ph;
    if (lane_ok && qi < pl.QB && rel >= a.rel_lo && rel < a.rel_hi) {
      long long o = a.o_lo + (rel - a.rel_lo);       // < 2 * out_cap: o_lo < out_cap, rel - rel_lo < t_hi - t_lo <= out_cap
      o = o >= a.out_cap ? o - a.out_cap : o;
      out_ring[o] = acc[i];
    }
  }
}

// the least input span a block stages (one period of a tile of phases): in_cap has to hold it
extern "C" int mmd_ring_resample_span(int L, int M, int taps) {
  if (!rs_factors_ok(L, M, taps)) return MMD_EINVAL;
  return rs_min_span(L, M, taps);
}

extern "C" int mmd_ring_resample(const float* in_ring, long long in_cap, int channels, long long n_valid, const float* bank,
                                 const int* phase_off, int L, int M, int taps, float* out_ring, long long out_cap, long long t_lo,
                                 long long t_hi, hipStream_t stream) {
  if (!in_ring || !bank || !phase_off || !out_ring || channels < 1 || channels > RS_ROWS_MAX) return MMD_EINVAL;
  if (!rs_factors_ok(L, M, taps)) return MMD_EINVAL;
  if (in_cap < 1 || in_cap > RING_MAX || out_cap < 1 || out_cap > RING_MAX || n_valid < 0 || n_valid > RING_MAX) return MMD_EINVAL;
  if (t_lo < 0 || t_hi <= t_lo || t_hi > RING_MAX || t_hi - t_lo > out_cap) return MMD_EINVAL;
  if (in_cap < rs_min_span(L, M, taps)) return MMD_EINVAL;
  if ((t_lo * M) / L - (taps >> 1) + 1 < n_valid - in_cap) return MMD_EINVAL;         // the oldest input is overwritten (t_lo * M < 2^60)
  RingRs a;
  a.q_lo = t_lo / L;
  const long long n_periods = (t_hi - 1) / L - a.q_lo + 1;
  a.rel_lo = t_lo - a.q_lo * L;
  a.rel_hi = t_hi - a.q_lo * L;
  a.v_lo = n_valid > in_cap ? n_valid - in_cap : 0;
  a.n_valid = n_valid;
  a.s_lo = a.v_lo % in_cap;
  a.in_cap = in_cap;
  a.out_cap = out_cap;
  a.o_lo = t_lo % out_cap;
  const RsPlan pl = rs_plan(L, M, taps, n_periods, in_cap < RS_LDS_FLOATS ? in_cap : RS_LDS_FLOATS);       // span <= in_cap
  const long long blocks = (n_periods + pl.QB - 1) / pl.QB;
  if (blocks > 0x7fffffffll) return MMD_EINVAL;
  const dim3 grid((unsigned)blocks, cdiv(L, pl.PH), channels);
  hipLaunchKernelGGL(ring_resample_kernel, grid, dim3(RS_THREADS), sizeof(float) * (size_t)pl.span, stream, in_ring, bank, phase_off, L, M,
                     taps, out_ring, a, pl);
  return mmd_check_launch();
}
