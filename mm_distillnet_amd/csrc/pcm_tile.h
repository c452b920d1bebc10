// One tile of the PCM de-interleaving transpose, shared by mmd_pcm_to_float (resample.hip) and mmd_ring_push_pcm (live.hip): both
// decode through this one body, so their floats agree bit for bit.
//
// interleaved little-endian signed PCM [frames, channels] of 2, 3 or 4 bytes -> float rows, one per channel.
// A block owns F consecutive frames (F * channels * width <= 16 KB).  It copies their bytes to LDS as aligned 32-bit words, lane i word i
// (a word that straddles the tile's first or last byte is put together from byte loads, so nothing outside the tile is read, whatever
// the buffer's alignment), then thread idx = c * F + f decodes sample (f, c) from LDS bytes and stores it in row c: the lanes of a
// wave write consecutive floats.  In LDS they read channels * width bytes apart (16 bytes for eight 16-bit channels: every fourth bank,
// 4 lanes of a 32-lane half on each); one pad word behind every 32 spreads such power-of-two strides over all banks.
#pragma once
#include "common.h"

#define PCM_THREADS 256
#define PCM_TILE_BYTES 16384
#define PCM_FMAX 2048
#define PCM_LDS_WORDS ((PCM_TILE_BYTES + 4) / 4 + (PCM_TILE_BYTES + 4) / 128 + 2)

__device__ __forceinline__ int pcm_lds(int byte) { return (((byte >> 2) + (byte >> 7)) << 2) | (byte & 3); }

// frames per block, or 0 where channels * width is above the tile (host and device: mmd_rings_push's blocks work it out per entry)
__host__ __device__ static inline int pcm_tile_frames(int channels, int width) {
  if (channels < 1 || channels > PCM_TILE_BYTES / width) return 0;
  const int F = PCM_TILE_BYTES / (channels * width);
  return F > PCM_FMAX ? PCM_FMAX : F;
}

// Frame f0 + f of channel c goes to out[c * row_stride + col], col = col0 + f0 + f, less `wrap` once where col >= wrap (a ring of `wrap`
// slots per row with col0 < wrap and frames <= wrap; the linear transpose passes a wrap no column reaches).
__device__ __forceinline__ void pcm_tile_to_rows(const unsigned char* __restrict__ pcm, long long frames, int channels, int width, int F,
                                                 float* __restrict__ out, long long row_stride, long long col0, long long wrap) {
  __shared__ unsigned int s_w[PCM_LDS_WORDS];
  const unsigned char* s_b = reinterpret_cast<const unsigned char*>(s_w);
  const int tid = threadIdx.x;
  const long long f0 = (long long)blockIdx.x * F;
  const int nf = (int)(frames - f0 < F ? frames - f0 : F);
  const int fb = channels * width;
  const unsigned char* src = pcm + (size_t)f0 * fb;
  const int nbytes = nf * fb;                                        // <= PCM_TILE_BYTES
  const int lead = (int)(reinterpret_cast<uintptr_t>(src) & 3);      // LDS byte `lead + o` = src[o]
  const int nwords = (lead + nbytes + 3) >> 2;
  for (int i = tid; i < nwords; i += PCM_THREADS) {
    const int lo = 4 * i - lead;
    unsigned int v = 0;
    if (lo >= 0 && lo + 4 <= nbytes) {
      v = *reinterpret_cast<const unsigned int*>(src + lo);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (lo + k >= 0 && lo + k < nbytes) v |= (unsigned int)src[lo + k] << (8 * k);
    }
    s_w[i + (i >> 5)] = v;
  }
  __syncthreads();
  for (int idx = tid; idx < channels * nf; idx += PCM_THREADS) {
    const int c = idx / nf, f = idx - c * nf;
    const int at = lead + (f * channels + c) * width;
    const unsigned int b0 = s_b[pcm_lds(at)], b1 = s_b[pcm_lds(at + 1)];
    float v;
    if (width == 2) {
      v = (float)(short)(b0 | (b1 << 8)) * (1.f / 32768.f);
    } else if (width == 3) {
      const unsigned int b2 = s_b[pcm_lds(at + 2)];
      v = (float)((int)((b0 | (b1 << 8) | (b2 << 16)) << 8) >> 8) * (1.f / 8388608.f);
    } else {
      const unsigned int b2 = s_b[pcm_lds(at + 2)], b3 = s_b[pcm_lds(at + 3)];
      v = (float)(int)(b0 | (b1 << 8) | (b2 << 16) | (b3 << 24)) * (1.f / 2147483648.f);      // (float)i rounds to nearest; 2^-31 is exact
    }
    long long col = col0 + f0 + f;
    col = col >= wrap ? col - wrap : col;
    out[(size_t)c * (size_t)row_stride + (size_t)col] = v;
  }
}
