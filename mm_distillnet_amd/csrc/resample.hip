// Sample-rate conversion and PCM decoding: the first link of the waveform chain that melspec.hip restates.
//
//   Both of upstream's audio entry points call librosa.load(path, sr=44100) (mp3_to_pkl.py:31; MultimodalDetection.merge_audios,
//   src/datasets/MultimodalDetection.py:335-336), so upstream resamples whatever rate a file has (librosa 0.7.2 hands that to resampy's
//   `kaiser_best`) before the mel spectrogram.
//
// Neither library is part of the reference tree or installed with this project.  The rule below is the project's OWN: a band-limited
// windowed-sinc interpolator after the published design of `kaiser_best` (Z = 64 zero crossings, rolloff = 0.9475937167399596, Kaiser
// beta = 14.769656459379492), evaluated as an EXACT rational polyphase filter - resampy's linearly interpolated table is not used.  It is
// pinned to tests/resample_ref.py; parity with resampy / librosa themselves is UNPINNED.
//
//   L / M = sr_out / sr_in in lowest terms, scale = min(1, L / M), half = ceil(Z / scale), taps = 2 * half
//   h(tau) = scale * rolloff * sinc(scale * rolloff * tau) * w(tau * scale / Z)        tau in input samples, sinc(x) = sin(pi x) / (pi x)
//   w(u)   = I0(beta * sqrt(1 - u^2)) / I0(beta) for |u| < 1, else 0
//   n_out  = ceil(n_in * L / M)
//   y[t]   = sum_{k = -half+1 .. half} h(p / L - k) * x[n + k],   n = (t * M) // L,  p = (t * M) % L,   x = 0 outside 0 .. n_in - 1
//
// The host (mm_distillnet_amd.audio.resample_bank) evaluates h in float64 and rounds it once to float32; the kernel multiplies those
// values and accumulates in fp32 in tap order.
//
// Indexing.  t * M passes 2^31 within 77 s of 192 kHz audio (M = 640), and a 64-bit division per output is dear, so outputs are addressed
// as (period q, output phase r): t = q * L + r, 0 <= r < L.  Then n = q * M + phase_off[r] with phase_off[r] = (r * M) // L < M, and the
// filter phase is p = (r * M) % L - both depend on r alone.  Only q * M, q * L and the row offsets are 64-bit; nothing is divided.
//
// Bank layout (the `bank` argument): [taps, L], bank[j * L + r] = h(p(r) / L - k) at k = j - half + 1 - TRANSPOSED and with the columns in
// OUTPUT-phase order r, not filter-phase order p.  The lanes of a wave hold neighbouring r, so for a fixed tap they read neighbouring
// addresses; with the natural [L, taps] layout they would read `taps` floats apart.  The bank is 80 KB (48 k -> 44.1 k) to 320 KB
// (192 k -> 44.1 k) and every block walks all of it: it lives in L2.
//
// Shape.  A block owns ONE row, a tile of PH <= 64 consecutive output phases (L split into cdiv(L, 64) equal tiles: 3 x 49 for L = 147)
// and QB consecutive periods.  Thread (ph, pq) = (tid % PH, tid / PH) accumulates RS_QT = 4 outputs of its phase, periods pq, pq + PS,
// pq + 2 PS, pq + 3 PS with PS = 256 / PH: one bank value from L2 feeds four multiply-adds, and the threads of a wave write outputs that
// are consecutive in t within a period (consecutive across periods too when PH == L).  The tile's input span,
// (QB - 1) * M + (phase_off[last] - phase_off[first]) + taps samples (13 KB for 48 k -> 44.1 k with QB = 20; for 192 k QB shrinks from 20 to
// 19 and the span fills the 48 KB cap, three blocks per CU), is staged into LDS once with coalesced loads, zeros where the index leaves
// 0 .. n_in - 1: the tap loop has no bounds test.
// LDS reads are ds_read_b32 at (period offset + phase offset + j): within a 32-lane half the phase offsets rise by M / L per lane, so
// lanes land on distinct banks for M / L near 1, share an address (broadcast) for upsampling, and collide about M / L ways when
// downsampling from 96 k or 192 k - four LDS reads per global load either way.  Plain stores, no atomics, fixed summation order: y
// needs no zeroing and two launches give the same bits.
#include "common.h"
#include "pcm_tile.h"
#include "resample_tile.h"                           // the plan of a block and its tap loop, shared with mmd_ring_resample (live.hip)

__global__ __launch_bounds__(RS_THREADS) void resample_poly_kernel(const float* __restrict__ x, long long n_in, const float* __restrict__ bank,
                                                                   const int* __restrict__ phase_off, int L, int M, int taps,
                                                                   float* __restrict__ y, long long n_out, RsPlan pl) {
  extern __shared__ float s_x[];                     // pl.span floats
  const int tid = threadIdx.x;
  const int r0 = blockIdx.y * pl.PH;                 // < L: gridDim.y = cdiv(L, PH)
  const long long q0 = (long long)blockIdx.x * pl.QB;
  x += (size_t)blockIdx.z * (size_t)n_in;
  y += (size_t)blockIdx.z * (size_t)n_out;

  // ---- stage the tile's input span; s_x[i] = x[g0 + i], zero outside the row
  const int off0 = phase_off[r0];
  const long long g0 = q0 * M + off0 - (taps >> 1) + 1;
  for (int i = tid; i < pl.span; i += RS_THREADS) {
    const long long g = g0 + i;
    s_x[i] = (g >= 0 && g < n_in) ? x[g] : 0.f;
  }
  __syncthreads();

  // ---- thread (ph, pq): phase r0 + ph, periods q0 + pq + i * PS (resample_tile.h)
  float acc[RS_QT];
  const bool lane_ok = rs_tile_taps(s_x, bank, phase_off, L, M, taps, pl, r0, off0, acc);
  const int ph = tid % pl.PH, pq = tid / pl.PH;
#pragma unroll
  for (int i = 0; i < RS_QT; ++i) {
    const int qi = pq + i * pl.PS;
    const long long t = (q0 + qi) * L + r0 + ph;
    if (lane_ok && qi < pl.QB && t < n_out) y[t] = acc[i];
  }
}

extern "C" int mmd_resample_poly(const float* x, int rows, long long n_in, const float* bank, const int* phase_off, int L, int M, int taps,
                                 float* y, long long n_out, hipStream_t stream) {
  if (!x || !bank || !phase_off || !y || rows < 1 || rows > RS_ROWS_MAX || n_in < 1 || n_in > (1ll << 50)) return MMD_EINVAL;
  if (!rs_factors_ok(L, M, taps)) return MMD_EINVAL;
  if (n_out != (n_in * L + M - 1) / M) return MMD_EINVAL;
  const long long n_periods = (n_out + L - 1) / L;
  const RsPlan pl = rs_plan(L, M, taps, n_periods);
  const long long blocks = (n_periods + pl.QB - 1) / pl.QB;
  if (blocks > 0x7fffffffll) return MMD_EINVAL;
  const dim3 grid((unsigned)blocks, cdiv(L, pl.PH), rows);
  hipLaunchKernelGGL(resample_poly_kernel, grid, dim3(RS_THREADS), sizeof(float) * (size_t)pl.span, stream, x, n_in, bank, phase_off, L, M,
                     taps, y, n_out, pl);
  return mmd_check_launch();
}

// ---- interleaved little-endian signed PCM [frames, channels] of 2, 3 or 4 bytes -> float [channels, frames]: a transpose.  The tile
// body (LDS staging, decoding) is pcm_tile.h's, shared with the ring writer of live.hip; here row c is out[c, :] and nothing wraps.
__global__ __launch_bounds__(PCM_THREADS) void pcm_to_float_kernel(const unsigned char* __restrict__ pcm, long long frames, int channels,
                                                                   int width, int F, float* __restrict__ out) {
  pcm_tile_to_rows(pcm, frames, channels, width, F, out, frames, 0ll, 0x7fffffffffffffffll);
}

extern "C" int mmd_pcm_to_float(const unsigned char* pcm, long long frames, int channels, int width, float* out, hipStream_t stream) {
  if (!pcm || !out || frames < 1 || channels < 1 || (width != 2 && width != 3 && width != 4)) return MMD_EINVAL;
  if (channels > PCM_TILE_BYTES / width || frames > (1ll << 50)) return MMD_EINVAL;
  const int F = pcm_tile_frames(channels, width);
  const long long blocks = (frames + F - 1) / F;
  if (blocks > 0x7fffffffll) return MMD_EINVAL;
  hipLaunchKernelGGL(pcm_to_float_kernel, dim3((unsigned)blocks), dim3(PCM_THREADS), 0, stream, pcm, frames, channels, width, F, out);
  return mmd_check_launch();
}
