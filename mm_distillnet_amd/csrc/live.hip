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
#include "common.h"
#include "pcm_tile.h"

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
