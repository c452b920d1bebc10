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
//
// A BANK of sessions (LiveBank.push_all) writes one round of chunks with mmd_rings_push and resamples it with mmd_rings_resample (at
// the end of this file): the same tiles, one launch for all sessions, driven by descriptor tables in device memory.
#include <cstring>
#include "common.h"
#include "pcm_tile.h"
#include "resample_tile.h"

#define RING_THREADS 256
#define RING_PER_THREAD 4
#define RING_MAX (1ll << 50)                         // cap and pos at most: pos + n stays far inside int64

// a block owns 1024 consecutive samples of one channel's row, thread t samples t, t + 256, t + 512, t + 768 of them (block: its index
// along the chunk); src and ring are that channel's rows
__device__ __forceinline__ void ring_push_tile(const float* __restrict__ src, long long n, float* __restrict__ ring, long long cap,
                                               long long p0, unsigned block) {
  const long long i0 = (long long)block * (RING_THREADS * RING_PER_THREAD) + threadIdx.x;
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

// blockIdx.y = channel
__global__ __launch_bounds__(RING_THREADS) void ring_push_kernel(const float* __restrict__ src, long long src_stride, long long n,
                                                                 float* __restrict__ ring, long long cap, long long p0) {
  ring_push_tile(src + (size_t)blockIdx.y * (size_t)src_stride, n, ring + (size_t)blockIdx.y * (size_t)cap, cap, p0, blockIdx.x);
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

// the block (bx, by) of the grid (blocks, cdiv(L, PH)) of one channel; in_ring and out_ring are that channel's rows
__device__ __forceinline__ void ring_resample_tile(const float* __restrict__ in_ring, const float* __restrict__ bank,
                                                   const int* __restrict__ phase_off, int L, int M, int taps, float* __restrict__ out_ring,
                                                   const RingRs& a, const RsPlan& pl, unsigned bx, unsigned by) {
  extern __shared__ float s_x[];                     // pl.span floats
  const int tid = threadIdx.x;
  const int r0 = by * pl.PH;                         // < L: by < cdiv(L, PH)
  const long long qb0 = (long long)bx * pl.QB;       // the tile's first period, counted from q_lo

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

// grid (blocks, cdiv(L, PH), channels)
__global__ __launch_bounds__(RS_THREADS) void ring_resample_kernel(const float* __restrict__ in_ring, const float* __restrict__ bank,
                                                                   const int* __restrict__ phase_off, int L, int M, int taps,
                                                                   float* __restrict__ out_ring, RingRs a, RsPlan pl) {
  ring_resample_tile(in_ring + (size_t)blockIdx.z * (size_t)a.in_cap, bank, phase_off, L, M, taps,
                     out_ring + (size_t)blockIdx.z * (size_t)a.out_cap, a, pl, blockIdx.x, blockIdx.y);
}

// the least input span a block stages (one period of a tile of phases): in_cap has to hold it
extern "C" int mmd_ring_resample_span(int L, int M, int taps) {
  if (!rs_factors_ok(L, M, taps)) return MMD_EINVAL;
  return rs_min_span(L, M, taps);
}

// mmd_ring_resample's refusals and its launch geometry, shared with the planner of mmd_rings_resample: -> 0 with a, pl and the grid's
// blocks and phase tiles filled, or MMD_EINVAL
static int ring_rs_plan(const void* in_ring, long long in_cap, int channels, long long n_valid, const void* bank, const void* phase_off,
                        int L, int M, int taps, const void* out_ring, long long out_cap, long long t_lo, long long t_hi, RingRs& a,
                        RsPlan& pl, long long& blocks, int& tiles) {
  if (!in_ring || !bank || !phase_off || !out_ring || channels < 1 || channels > RS_ROWS_MAX) return MMD_EINVAL;
  if (!rs_factors_ok(L, M, taps)) return MMD_EINVAL;
  if (in_cap < 1 || in_cap > RING_MAX || out_cap < 1 || out_cap > RING_MAX || n_valid < 0 || n_valid > RING_MAX) return MMD_EINVAL;
  if (t_lo < 0 || t_hi <= t_lo || t_hi > RING_MAX || t_hi - t_lo > out_cap) return MMD_EINVAL;
  if (in_cap < rs_min_span(L, M, taps)) return MMD_EINVAL;
  if ((t_lo * M) / L - (taps >> 1) + 1 < n_valid - in_cap) return MMD_EINVAL;         // the oldest input is overwritten (t_lo * M < 2^60)
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
  pl = rs_plan(L, M, taps, n_periods, in_cap < RS_LDS_FLOATS ? in_cap : RS_LDS_FLOATS);       // span <= in_cap
  blocks = (n_periods + pl.QB - 1) / pl.QB;
  if (blocks > 0x7fffffffll) return MMD_EINVAL;
  tiles = cdiv(L, pl.PH);
  return 0;
}

extern "C" int mmd_ring_resample(const float* in_ring, long long in_cap, int channels, long long n_valid, const float* bank,
                                 const int* phase_off, int L, int M, int taps, float* out_ring, long long out_cap, long long t_lo,
                                 long long t_hi, hipStream_t stream) {
  RingRs a;
  RsPlan pl;
  long long blocks;
  int tiles;
  if (ring_rs_plan(in_ring, in_cap, channels, n_valid, bank, phase_off, L, M, taps, out_ring, out_cap, t_lo, t_hi, a, pl, blocks, tiles))
    return MMD_EINVAL;
  const dim3 grid((unsigned)blocks, tiles, channels);
  hipLaunchKernelGGL(ring_resample_kernel, grid, dim3(RS_THREADS), sizeof(float) * (size_t)pl.span, stream, in_ring, bank, phase_off, L, M,
                     taps, out_ring, a, pl);
  return mmd_check_launch();
}

// ---- the batched forms (LiveBank.push_all): one launch for the ring writes of several sessions, one for their resamplings.  Each is
// driven by a table of descriptors in DEVICE memory - the number of entries varies per call, so they are no kernel arguments - of which
// the caller also hands over the HOST copy it uploaded: the wrappers check and size the launch from that one, the blocks read the other.
// blockIdx.z names the entry; the grid covers the largest entry, and a block outside its own entry's range returns before it touches
// memory or meets a barrier (the test is on blockIdx and the entry's words alone: the whole block decides alike).

// 64 bytes, all int64 so that a host fills it as a row of eight words
struct RingsPushDesc {
  long long src_off;                                 // the chunk, in bytes from the launch's src_base (float rows: a multiple of 4)
  long long src_stride;                              // float rows: floats between two channels' rows (>= n); PCM: unused
  long long n;                                       // samples per channel / frames, 1 .. cap
  long long kind;                                    // 0: float rows; 2, 3, 4: PCM frames of that width
  long long ring;                                    // the destination ring[channels, cap], as a device address
  long long cap;
  long long p0;                                      // pos % cap, reduced on the host
  long long pad;
};
static_assert(sizeof(RingsPushDesc) == 64, "RingsPushDesc is the 64-byte row include/mmdistill.h documents");

// float entries: ring_push_kernel's blocks (x: 1024 samples, y: channel).  PCM entries: ring_push_pcm_kernel's (x: F frames, all
// channels; y = 0 alone works).  RING_THREADS == PCM_THREADS.
__global__ __launch_bounds__(RING_THREADS) void rings_push_kernel(const unsigned char* __restrict__ src_base,
                                                                  const RingsPushDesc* __restrict__ desc, int channels) {
  const RingsPushDesc d = desc[blockIdx.z];
  float* ring = reinterpret_cast<float*>(d.ring);
  if (d.kind == 0) {
    if ((long long)blockIdx.x * (RING_THREADS * RING_PER_THREAD) >= d.n) return;
    const float* src = reinterpret_cast<const float*>(src_base + d.src_off);
    ring_push_tile(src + (size_t)blockIdx.y * (size_t)d.src_stride, d.n, ring + (size_t)blockIdx.y * (size_t)d.cap, d.cap, d.p0, blockIdx.x);
    return;
  }
  const int width = (int)d.kind, F = pcm_tile_frames(channels, width);
  if (blockIdx.y != 0 || (long long)blockIdx.x * F >= d.n) return;
  pcm_tile_to_rows(src_base + d.src_off, d.n, channels, width, F, ring, d.cap, d.p0, d.cap);
}

static_assert(RING_THREADS == PCM_THREADS, "rings_push_kernel runs both tiles in one block shape");

extern "C" int mmd_rings_push(const void* src_base, const void* h_desc, const void* d_desc, int n_desc, int channels, hipStream_t stream) {
  if (!src_base || !h_desc || !d_desc || n_desc < 1 || n_desc > 65535 || channels < 1 || channels > 65535) return MMD_EINVAL;
  const RingsPushDesc* h = static_cast<const RingsPushDesc*>(h_desc);
  long long most = 0;
  for (int e = 0; e < n_desc; ++e) {
    const RingsPushDesc& d = h[e];
    if (!d.ring || d.src_off < 0 || d.n < 1 || d.cap > RING_MAX || d.n > d.cap || d.p0 < 0 || d.p0 >= d.cap) return MMD_EINVAL;
    long long per;
    if (d.kind == 0) {
      if (d.src_stride < d.n || (d.src_off & 3) || (reinterpret_cast<uintptr_t>(src_base) & 3)) return MMD_EINVAL;
      per = RING_THREADS * RING_PER_THREAD;
    } else {
      if (d.kind != 2 && d.kind != 3 && d.kind != 4) return MMD_EINVAL;
      per = pcm_tile_frames(channels, (int)d.kind);
      if (per < 1) return MMD_EINVAL;
    }
    const long long blocks = (d.n + per - 1) / per;
    most = blocks > most ? blocks : most;
  }
  if (most > 0x7fffffffll) return MMD_EINVAL;
  hipLaunchKernelGGL(rings_push_kernel, dim3((unsigned)most, channels, n_desc), dim3(RING_THREADS), 0, stream,
                     static_cast<const unsigned char*>(src_base), static_cast<const RingsPushDesc*>(d_desc), channels);
  return mmd_check_launch();
}

// 192 bytes: what mmd_ring_resample takes for one session, and behind it what mmd_rings_resample_plan makes of that
struct RingsRsDesc {
  long long in_ring, bank, phase_off, out_ring;      // device addresses
  long long in_cap, n_valid, out_cap, t_lo, t_hi;
  int L, M, taps, tiles;                             // tiles = cdiv(L, PH): the entry's gridDim.y
  long long blocks;                                  // the entry's gridDim.x
  RingRs a;
  RsPlan pl;
  int pad;
};
static_assert(sizeof(RingsRsDesc) == 192, "RingsRsDesc is the 192-byte row include/mmdistill.h documents");

// fills the derived half of d from its arguments' half; MMD_EINVAL on what mmd_ring_resample refuses
static int rings_rs_fill(RingsRsDesc& d, int channels) {
  long long blocks;
  if (ring_rs_plan(reinterpret_cast<const void*>(d.in_ring), d.in_cap, channels, d.n_valid, reinterpret_cast<const void*>(d.bank),
                   reinterpret_cast<const void*>(d.phase_off), d.L, d.M, d.taps, reinterpret_cast<const void*>(d.out_ring), d.out_cap,
                   d.t_lo, d.t_hi, d.a, d.pl, blocks, d.tiles))
    return MMD_EINVAL;
  d.blocks = blocks;
  d.pad = 0;
  return 0;
}

extern "C" int mmd_rings_resample_plan(void* h_desc, int index, const float* in_ring, long long in_cap, int channels, long long n_valid,
                                       const float* bank, const int* phase_off, int L, int M, int taps, float* out_ring, long long out_cap,
                                       long long t_lo, long long t_hi) {
  if (!h_desc || index < 0 || index > 65534) return MMD_EINVAL;
  RingsRsDesc d;
  d.in_ring = (long long)reinterpret_cast<uintptr_t>(in_ring);
  d.bank = (long long)reinterpret_cast<uintptr_t>(bank);
  d.phase_off = (long long)reinterpret_cast<uintptr_t>(phase_off);
  d.out_ring = (long long)reinterpret_cast<uintptr_t>(out_ring);
  d.in_cap = in_cap, d.n_valid = n_valid, d.out_cap = out_cap, d.t_lo = t_lo, d.t_hi = t_hi;
  d.L = L, d.M = M, d.taps = taps;
  if (rings_rs_fill(d, channels)) return MMD_EINVAL;
  static_cast<RingsRsDesc*>(h_desc)[index] = d;
  return 0;
}

// grid (max blocks, max tiles, channels * n_desc); dynamic LDS: the largest span
__global__ __launch_bounds__(RS_THREADS) void rings_resample_kernel(const RingsRsDesc* __restrict__ desc, int channels) {
  const unsigned e = blockIdx.z / channels, c = blockIdx.z - e * channels;
  const RingsRsDesc& d = desc[e];
  if (blockIdx.x >= d.blocks || blockIdx.y >= (unsigned)d.tiles) return;         // in front of the first barrier, the whole block alike
  const RingRs a = d.a;
  const RsPlan pl = d.pl;
  ring_resample_tile(reinterpret_cast<const float*>(d.in_ring) + (size_t)c * (size_t)a.in_cap, reinterpret_cast<const float*>(d.bank),
                     reinterpret_cast<const int*>(d.phase_off), d.L, d.M, d.taps,
                     reinterpret_cast<float*>(d.out_ring) + (size_t)c * (size_t)a.out_cap, a, pl, blockIdx.x, blockIdx.y);
}

extern "C" int mmd_rings_resample(const void* h_desc, const void* d_desc, int n_desc, int channels, hipStream_t stream) {
  if (!h_desc || !d_desc || n_desc < 1 || n_desc > 65535 || channels < 1 || channels > RS_ROWS_MAX ||
      (long long)n_desc * channels > 65535)
    return MMD_EINVAL;
  const RingsRsDesc* h = static_cast<const RingsRsDesc*>(h_desc);
  long long blocks = 0;
  int tiles = 0, span = 0;
  for (int e = 0; e < n_desc; ++e) {
    RingsRsDesc d = h[e];                            // planned anew from the entry's arguments: the derived half must be the plan's
    if (rings_rs_fill(d, channels) || memcmp(&d, &h[e], sizeof(d))) return MMD_EINVAL;
    blocks = d.blocks > blocks ? d.blocks : blocks;
    tiles = d.tiles > tiles ? d.tiles : tiles;
    span = d.pl.span > span ? d.pl.span : span;
  }
  hipLaunchKernelGGL(rings_resample_kernel, dim3((unsigned)blocks, tiles, channels * n_desc), dim3(RS_THREADS),
                     sizeof(float) * (size_t)span, stream, static_cast<const RingsRsDesc*>(d_desc), channels);
  return mmd_check_launch();
}
