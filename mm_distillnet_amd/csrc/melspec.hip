// Waveform front end: power mel spectrograms of (optionally mixed) microphone waveforms in one launch.
//
//   MultimodalDetection.merge_audios (src/datasets/MultimodalDetection.py:329-353, per sample from yield_batch, :355-367) and
//   Audio2Spectogram (src/datasets/transformations.py:251-266): average two recordings' eight waveforms and run
//   librosa.feature.melspectrogram(sr=44100, n_fft=1024, hop_length=256, n_mels=80) on each channel.
//
// librosa (0.7.2 in requirements.txt) is a third-party dependency that is neither part of the reference tree nor installed with this
// project: the arithmetic below restates its published definition - y = (a + b) / 2 in fp32, reflect padding of n_fft / 2 samples
// (edge sample not repeated), frames of 1024 at hop 256 times the periodic Hann window, |rfft|^2, Slaney mel bank - and is pinned to
// tests/melspec_ref.py.  Parity with librosa itself is UNPINNED.  mmd_melspec_power has no power_to_db: merge_audios returns power.
//
// The student's ordinary input is the dB map of mp3_to_pkl.py:31-41: melspectrogram(...) then librosa.power_to_db(S, ref=np.max) per
// microphone.  mmd_melspec_batch (db = 1) and mmd_power_to_db restate that published rule - ls = 10 log10(max(1e-10, S)) -
// 10 log10(max(1e-10, max S)), then max(ls, max(ls) - 80) - pinned to tests/melspec_db_ref.py; parity with librosa's power_to_db itself
// is UNPINNED.  The maximum is per (sample, channel): each block's epilogue sends the maximum of what it stored to one word of a
// [B * C] workspace with an unsigned atomic max on the float's bits (power is >= +0, so the bit patterns order like the values; a
// maximum does not depend on arrival order, so two launches give the same bits), and a second, elementwise launch converts in place.
//
// Shape: a block owns ONE channel and MEL_FPB = 8 consecutive frames.  Frames overlap by 75 %, so the block stages the (8 + 3) * 256
// samples they cover in LDS once (mix and reflect index at that load; the index is clamped, never guarded: frames past the end compute
// on clamped samples and only their stores are masked).  Each of the 4 waves then transforms TWO real frames as one 1024-point complex
// FFT z = x0 + i x1 with 16 points per lane: radix-16, radix-16, radix-4 butterflies in registers, two exchanges through a wave-private
// LDS buffer whose rows of 16 complex values are padded to 17 (the 16- and 256-strided accesses of the exchanges otherwise land on one
// bank).  X0[k] = (Z[k] + conj Z[N-k]) / 2, X1[k] = (Z[k] - conj Z[N-k]) / 2i give the two power rows, which replace Z in LDS, and the
// mel projection reads them through the band form of the filter bank (each mel row is one contiguous run of at most ~50 bins; a dense
// 80 x 513 product would cost more than the FFT).  Twiddles and window are tables rounded once from double (melspec_tables.h).
// Plain stores, no atomics, fixed summation order: the output needs no zeroing and two launches give the same bits.
#include "common.h"
#include "melspec_tables.h"

#define MEL_NFFT 1024
#define MEL_HOP 256
#define MEL_NMEL 80
#define MEL_BINS 513
#define MEL_FPB 8                                   // frames per block: 4 waves x 2 frames
#define MEL_STAGE ((MEL_FPB + 3) * MEL_HOP)         // samples the block's frames cover
#define MEL_ZROW 1088                               // 1024 complex values in rows of 16 padded to 17
#define MEL_PROW 520                                // second power row's offset inside the (reused) exchange buffer
#define MEL_WMAX 4096                               // band weights kept in LDS: 80 * band_stride floats at most (stride <= 51)
#define MEL_DB_CMAX 1024                            // mmd_power_to_db: channels whose maxima one block keeps in LDS

__device__ __forceinline__ float2 mel_cmul(float2 a, float2 w) { return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }
__device__ __forceinline__ float2 mel_tw(int m) { return reinterpret_cast<const float2*>(mmd_mel_twiddle)[m]; }

// forward 4-point DFT (e^{-2 pi i nk/4}), in place
__device__ __forceinline__ void mel_dft4(float2& a0, float2& a1, float2& a2, float2& a3) {
  const float2 s0 = make_float2(a0.x + a2.x, a0.y + a2.y), s1 = make_float2(a0.x - a2.x, a0.y - a2.y);
  const float2 s2 = make_float2(a1.x + a3.x, a1.y + a3.y), s3 = make_float2(a1.x - a3.x, a1.y - a3.y);
  a0 = make_float2(s0.x + s2.x, s0.y + s2.y);
  a1 = make_float2(s1.x + s3.y, s1.y - s3.x);        // s1 - i s3
  a2 = make_float2(s0.x - s2.x, s0.y - s2.y);
  a3 = make_float2(s1.x - s3.y, s1.y + s3.x);        // s1 + i s3
}
// e^{-2 pi i m/16} for the products b*c of the 4 x 4 split (m in {0,1,2,3,4,6,9}); constants after unrolling
__device__ __forceinline__ float2 mel_w16(int m) {
  const float c1 = 0.92387953251128674f, s1 = 0.38268343236508977f, h = 0.70710678118654752f;
  switch (m) {
    case 1: return make_float2(c1, -s1);
    case 2: return make_float2(h, -h);
    case 3: return make_float2(s1, -c1);
    case 4: return make_float2(0.f, -1.f);
    case 6: return make_float2(-h, -h);
    case 9: return make_float2(-c1, s1);
    default: return make_float2(1.f, 0.f);
  }
}
// forward 16-point DFT in registers: n = 4a + b, k = c + 4d: DFT4 over a, times W16^{bc}, DFT4 over b
__device__ __forceinline__ void mel_dft16(float2 v[16]) {
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    mel_dft4(v[b], v[4 + b], v[8 + b], v[12 + b]);           // v[4c + b] = y[b][c]
#pragma unroll
    for (int c = 1; c < 4; ++c)
      if (b) v[4 * c + b] = mel_cmul(v[4 * c + b], mel_w16(b * c));
  }
  float2 o[16];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    mel_dft4(v[4 * c], v[4 * c + 1], v[4 * c + 2], v[4 * c + 3]);       // v[4c + d] = X[c + 4d]
#pragma unroll
    for (int d = 0; d < 4; ++d) o[c + 4 * d] = v[4 * c + d];
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = o[i];
}
__device__ __forceinline__ int mel_pad(int i) { return i + (i >> 4); }

// blockIdx.z = the sample of a batch ([B, C, N] waveforms -> [B, 80, T, C]); TRACK: also the block's maximum into mx_ws[sample * C + c]
// WIN = MEL_WIN_LINEAR (mmd_melspec_windows): sample b is the window wav_a[:, win_start[b] : win_start[b] + N] of ONE recording wav_a[C, n_total]; only
// the base pointer differs - every index below stays in window coordinates 0 .. N-1, so the reflection sees the window's own two ends
// and the bits are those of the materialised [B, C, N] stack.  The start is clamped into [0, n_total - N]: a bad table reads the wrong
// window, never outside the recording.
// WIN = MEL_WIN_RING (mmd_melspec_windows_ring): the recording is a ring wav_a[C, n_total] of n_total = cap slots per channel and
// win_start[b] an ABSOLUTE sample position: window sample s lives at slot (win_start[b] + s) % cap.  The start is reduced modulo cap
// once per block; s <= N - 1 < cap, so a slot wraps at most once: one compare and one subtract at the staging load, which is the only
// line that differs.  A negative start is clamped to 0; every slot read is inside the channel's row.
// WIN = MEL_WIN_RINGS (mmd_melspec_windows_rings): MEL_WIN_RING for wav_a[n_sess, C, n_total], the rings of a bank of sessions in one
// block of memory; sample b reads the ring of session win_sess[b].  Only the row base differs: (sess * C + c) * n_total.  The session is
// clamped into 0 .. n_sess-1: a bad table reads the wrong ring, never outside wav_a.
#define MEL_WIN_NONE 0
#define MEL_WIN_LINEAR 1
#define MEL_WIN_RING 2
#define MEL_WIN_RINGS 3
template <bool MIX, bool TRACK, int WIN>
__global__ __launch_bounds__(256) void melspec_power_kernel(const float* __restrict__ wav_a, const float* __restrict__ wav_b, long long N,
                                                            int T, int C, const int* __restrict__ band_start,
                                                            const int* __restrict__ band_len, const float* __restrict__ band_w,
                                                            int band_stride, float* __restrict__ out, unsigned int* __restrict__ mx_ws,
                                                            const long long* __restrict__ win_start, long long n_total,
                                                            const int* __restrict__ win_sess, int n_sess) {
  __shared__ float s_x[MEL_STAGE];
  __shared__ float2 s_z[4][MEL_ZROW];
  __shared__ float s_w[MEL_WMAX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = blockIdx.y, f0 = blockIdx.x * MEL_FPB;
  const size_t smp = blockIdx.z;
  const float* pa;
  long long r0 = 0;                                  // MEL_WIN_RING / MEL_WIN_RINGS: the window's first slot
  if (WIN == MEL_WIN_RINGS) {
    const long long w0 = win_start[smp];
    r0 = w0 < 0 ? 0 : w0 % n_total;
    int ss = win_sess[smp];
    ss = ss < 0 ? 0 : (ss > n_sess - 1 ? n_sess - 1 : ss);
    pa = wav_a + ((size_t)ss * C + c) * (size_t)n_total;
  } else if (WIN == MEL_WIN_RING) {
    const long long w0 = win_start[smp];
    r0 = w0 < 0 ? 0 : w0 % n_total;
    pa = wav_a + (size_t)c * (size_t)n_total;
  } else if (WIN == MEL_WIN_LINEAR) {
    long long w0 = win_start[smp];
    w0 = w0 < 0 ? 0 : (w0 > n_total - N ? n_total - N : w0);
    pa = wav_a + (size_t)c * (size_t)n_total + (size_t)w0;
  } else {
    pa = wav_a + (smp * C + c) * (size_t)N;
  }
  const float* pb = MIX ? wav_b + (smp * C + c) * (size_t)N : nullptr;
  out += smp * MEL_NMEL * (size_t)T * C;

  // ---- stage the block's samples: padded position p <-> sample p - 512, reflected at both ends, then clamped (frames >= T only);
  //      WIN: s is an index into the window (pa points at its first sample), so 0 <= s <= N - 1 keeps every read inside it
  const long long base = (long long)f0 * MEL_HOP - MEL_NFFT / 2;
#pragma unroll
  for (int it = 0; it < MEL_STAGE / 256; ++it) {
    const int i = tid + 256 * it;
    long long s = base + i;
    s = s < 0 ? -s : s;
    s = s >= N ? 2 * (N - 1) - s : s;
    s = s < 0 ? 0 : (s > N - 1 ? N - 1 : s);
    if (WIN == MEL_WIN_RING || WIN == MEL_WIN_RINGS) {
      s += r0;
      s = s >= n_total ? s - n_total : s;
    }
    float v = pa[s];
    if (MIX) v = (v + pb[s]) * 0.5f;
    s_x[i] = v;
  }
  for (int i = tid; i < MEL_NMEL * band_stride; i += 256) s_w[i] = band_w[i];
  __syncthreads();

  // The exchange buffer s_z[wave] is WAVE-PRIVATE: from here on no wave reads what another wrote.  The __syncthreads below only order
  // one wave's own LDS writes before its reads (and reads before the overwriting writes); they are block-wide for simplicity - all four
  // waves run the same straight-line code - not because the buffer is shared.
  // ---- pass 1: radix-16 over n = lane + 64 r (no twiddles), out[16 lane + r]
  float2* zb = s_z[wave];
  const float* x0 = s_x + wave * 2 * MEL_HOP;
  const float* x1 = x0 + MEL_HOP;
  float2 v[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int n = lane + 64 * r;
    const float w = mmd_mel_hann[n];
    v[r] = make_float2(w * x0[n], w * x1[n]);
  }
  mel_dft16(v);
#pragma unroll
  for (int r = 0; r < 16; ++r) zb[lane * 17 + r] = v[r];
  __syncthreads();

  // ---- pass 2: radix-16 over in[lane + 64 r] with twiddle W256^{r k}, k = lane % 16; out[256 (lane / 16) + k + 16 r]
  const int k16 = lane & 15;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    v[r] = zb[mel_pad(lane + 64 * r)];
    if (r) v[r] = mel_cmul(v[r], mel_tw((4 * r * k16) & (MEL_NFFT - 1)));
  }
  __syncthreads();
  mel_dft16(v);
#pragma unroll
  for (int r = 0; r < 16; ++r) zb[(lane >> 4) * 272 + k16 + 17 * r] = v[r];
  __syncthreads();

  // ---- pass 3: four radix-4 butterflies per lane over in[j + 256 r], j = lane + 64 q, twiddle W1024^{r j}; Z[j + 256 r] in place
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int j = lane + 64 * q;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      v[4 * q + r] = zb[mel_pad(j + 256 * r)];
      if (r) v[4 * q + r] = mel_cmul(v[4 * q + r], mel_tw(r * j));
    }
    mel_dft4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int r = 0; r < 4; ++r) zb[lane + 64 * q + 256 * r] = v[4 * q + r];         // natural order, unpadded
  __syncthreads();

  // ---- split the two real spectra, power of bins 0..512 (bin index clamped, store masked)
  float p0[9], p1[9];
#pragma unroll
  for (int m = 0; m < 9; ++m) {
    const int k = min(lane + 64 * m, MEL_BINS - 1);
    const float2 zk = zb[k], zn = zb[(MEL_NFFT - k) & (MEL_NFFT - 1)];
    const float ar = zk.x + zn.x, ai = zk.y - zn.y;          // 2 X0[k]
    const float br = zk.y + zn.y, bi = zk.x - zn.x;          // 2 X1[k] (up to the factor -i)
    p0[m] = 0.25f * (ar * ar + ai * ai);
    p1[m] = 0.25f * (br * br + bi * bi);
  }
  __syncthreads();
  float* pw = reinterpret_cast<float*>(zb);
#pragma unroll
  for (int m = 0; m < 9; ++m) {
    const int k = lane + 64 * m;
    if (k < MEL_BINS) { pw[k] = p0[m]; pw[MEL_PROW + k] = p1[m]; }
  }
  __syncthreads();

  // (The unoptimised part of the kernel, small against the FFT: per-lane trip counts of 2..50 diverge, 64 then 32 of 64 lanes work, and
  // lanes store T * C floats apart.  Follow-up together with batching the samples of a batch into one launch.)
  // ---- mel projection from the band form: mel rows 0..63 one per lane (both frames share the weight), rows 64..79 on lanes 0..31
  const int t0 = f0 + wave * 2;
  float mx = 0.f;                                    // TRACK: maximum of what this lane stores (frames >= T hold clamped samples: left out)
  {
    const int mel = lane;
    const int st = min(max(band_start[mel], 0), MEL_BINS - 1);
    const int ln = min(max(band_len[mel], 0), min(MEL_BINS - st, band_stride));
    const float* w = s_w + mel * band_stride;
    float a0 = 0.f, a1 = 0.f;
    for (int j = 0; j < ln; ++j) {
      a0 = fmaf(w[j], pw[st + j], a0);
      a1 = fmaf(w[j], pw[MEL_PROW + st + j], a1);
    }
    if (t0 < T) out[((size_t)mel * T + t0) * C + c] = a0;
    if (t0 + 1 < T) out[((size_t)mel * T + t0 + 1) * C + c] = a1;
    if (TRACK) mx = fmaxf(t0 < T ? a0 : 0.f, t0 + 1 < T ? a1 : 0.f);
  }
  {
    const int mel = 64 + (lane & 15), fr = (lane >> 4) & 1;
    const int st = min(max(band_start[mel], 0), MEL_BINS - 1);
    const int ln = lane < 32 ? min(max(band_len[mel], 0), min(MEL_BINS - st, band_stride)) : 0;
    const float* w = s_w + mel * band_stride;
    const float* p = pw + fr * MEL_PROW + st;
    float acc = 0.f;
    for (int j = 0; j < ln; ++j) acc = fmaf(w[j], p[j], acc);
    if (lane < 32 && t0 + fr < T) out[((size_t)mel * T + t0 + fr) * C + c] = acc;
    if (TRACK && lane < 32 && t0 + fr < T) mx = fmaxf(mx, acc);
  }
  if (TRACK) {
    // one atomic per block: waves through LDS (s_x was last read in pass 1, many barriers ago), then the bits of a value >= +0
    mx = wave_max(mx);
    if (lane == 0) s_x[wave] = mx;
    __syncthreads();
    if (tid == 0) {
      mx = fmaxf(fmaxf(s_x[0], s_x[1]), fmaxf(s_x[2], s_x[3]));
      atomicMax(mx_ws + smp * C + c, __float_as_uint(mx > 0.f ? mx : 0.f));
    }
  }
}

// ---- librosa.power_to_db(S, ref=np.max, amin=1e-10, top_db=80) per (sample, channel) map, as published:
//        ls = 10 log10(max(amin, S)) - 10 log10(max(amin, max S));  ls = max(ls, max(ls) - top_db)
// max(ls) is the value at the map's maximum, 10 log10(m) - 10 log10(m) = +0 exactly (log10f is monotone), so the floor is -80.
// Each product and the difference are rounded on their own like numpy's three array operations (contraction is off), and both
// entry points convert through this one function: their bits agree.
#define MEL_AMIN 1e-10f
#define MEL_TOPDB 80.f
__device__ __forceinline__ float mel_power_to_db(float s, float ref) {
#pragma clang fp contract(off)      // a fused 10 * a - (10 * b) leaves the product's rounding error, not 0, at the maximum (s == ref)
  const float a = 10.f * log10f(fmaxf(MEL_AMIN, s));
  const float b = 10.f * log10f(fmaxf(MEL_AMIN, ref));
  const float ls = a - b;
  return fmaxf(ls, 0.f - MEL_TOPDB);
}

// x[B, P, C] in place; mx_ws[B * C] = the bits of each map's maximum.  blockIdx.y = sample.
__global__ __launch_bounds__(256) void power_to_db_kernel(float* __restrict__ x, size_t per_sample, int C,
                                                          const unsigned int* __restrict__ mx_ws) {
  const size_t b = blockIdx.y;
  float* xs = x + b * per_sample;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < per_sample; i += (size_t)gridDim.x * 256)
    xs[i] = mel_power_to_db(xs[i], __uint_as_float(mx_ws[b * C + (int)(i % C)]));
}

// mx_ws[b * C + c] = max(mx_ws[..], bits of max(0, x[b, :, c])): values below +0 (none in a power map) count as 0, like max(amin, S)
__global__ __launch_bounds__(256) void power_max_kernel(const float* __restrict__ x, size_t per_sample, int C,
                                                        unsigned int* __restrict__ mx_ws) {
  __shared__ unsigned int s_m[MEL_DB_CMAX];
  const size_t b = blockIdx.y;
  const float* xs = x + b * per_sample;
  for (int i = threadIdx.x; i < C; i += 256) s_m[i] = 0u;
  __syncthreads();
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < per_sample; i += (size_t)gridDim.x * 256) {
    const float v = xs[i];
    if (v > 0.f) atomicMax(&s_m[(int)(i % C)], __float_as_uint(v));
  }
  __syncthreads();
  for (int i = threadIdx.x; i < C; i += 256)
    if (s_m[i]) atomicMax(mx_ws + b * C + i, s_m[i]);
}

// 1 + n_samples / 256 frames (center=True), or MMD_EINVAL: reflect padding of 512 needs more than 512 samples
extern "C" int mmd_melspec_frames(long long n_samples) {
  if (n_samples <= MEL_NFFT / 2 || n_samples / MEL_HOP >= 0x7fffffffLL) return MMD_EINVAL;
  return (int)(1 + n_samples / MEL_HOP);
}

// The maxima workspace is cleared by the project's zero-fill KERNEL (mmd_zero_bytes, optim.hip), not by hipMemsetAsync: a memset node
// recorded by stream capture is not reliably executed on later replays of the graph (optim.hip found the same on the accumulator arenas).
// Seen here as: from the second replay of AudioDetector's waveform graph on, max_ws held stale or foreign words in front of the
// atomicMax, the dB reference was wrong and detect() returned other rows than the eager run on the same clip.
static int mel_zero_max(unsigned int* mx, int batch, int channels, hipStream_t stream) {
  return mmd_zero_bytes(mx, sizeof(unsigned int) * (size_t)batch * channels, stream);
}

static void power_to_db_launch(float* x, int batch, size_t per_sample, int C, const unsigned int* mx_ws, hipStream_t stream) {
  const size_t blocks = (per_sample + 255) / 256;
  const dim3 grid((unsigned)(blocks < 4096 ? blocks : 4096), batch);
  hipLaunchKernelGGL(power_to_db_kernel, grid, dim3(256), 0, stream, x, per_sample, C, mx_ws);
}

// The launch sequence of the five entry points below: [zero max_ws ->] melspec_power_kernel<MIX = wav_b, TRACK = db, WIN = win> [-> dB pass].
// n_samples: the length of one sample (a window's, in the window modes).  win = MEL_WIN_LINEAR / MEL_WIN_RING: win_start[batch] into ONE
// recording / ring wav_a[channels, extent], no wav_b; MEL_WIN_NONE: wav_a (+ wav_b) [batch, channels, n_samples], no win_start.
// MEL_WIN_RINGS: MEL_WIN_RING with wav_a[n_sess, channels, extent] and win_sess[batch]; the other modes pass no win_sess.
static int melspec_launch(int win, const float* wav_a, const float* wav_b, int batch, int channels, long long n_samples,
                          const long long* win_start, long long extent, const int* band_start, const int* band_len, const float* band_w,
                          int band_stride, int db, float* max_ws, float* out, hipStream_t stream, const int* win_sess = nullptr,
                          int n_sess = 0) {
  if (!wav_a || !band_start || !band_len || !band_w || !out || channels <= 0 || channels > 65535 || batch <= 0 || batch > 65535)
    return MMD_EINVAL;
  if (band_stride <= 0 || band_stride * MEL_NMEL > MEL_WMAX || (db != 0 && db != 1) || (db && !max_ws)) return MMD_EINVAL;
  const int T = mmd_melspec_frames(n_samples);
  if (T < 0 || (win != MEL_WIN_NONE && (!win_start || n_samples > extent))) return MMD_EINVAL;
  if (win == MEL_WIN_RINGS && (!win_sess || n_sess < 1)) return MMD_EINVAL;
  const dim3 grid(cdiv(T, MEL_FPB), channels, batch), block(256);
  unsigned int* mx = db ? reinterpret_cast<unsigned int*>(max_ws) : nullptr;
  if (db && mel_zero_max(mx, batch, channels, stream) != MMD_OK) return MMD_ELAUNCH;
#define MEL_LAUNCH(MIX, TRACK, WIN)                                                                                                  \
  hipLaunchKernelGGL((melspec_power_kernel<MIX, TRACK, WIN>), grid, block, 0, stream, wav_a, wav_b, n_samples, T, channels, band_start, \
                     band_len, band_w, band_stride, out, mx, win_start, extent, win_sess, n_sess)
  // (named in the order the code object has always held the first eight instantiations; the two of MEL_WIN_RINGS come behind them)
  if (win == MEL_WIN_NONE && !db) {
    if (wav_b) MEL_LAUNCH(true, false, MEL_WIN_NONE); else MEL_LAUNCH(false, false, MEL_WIN_NONE);
  } else if (win == MEL_WIN_NONE) {
    if (wav_b) MEL_LAUNCH(true, true, MEL_WIN_NONE); else MEL_LAUNCH(false, true, MEL_WIN_NONE);
  } else if (win == MEL_WIN_LINEAR) {
    if (db) MEL_LAUNCH(false, true, MEL_WIN_LINEAR); else MEL_LAUNCH(false, false, MEL_WIN_LINEAR);
  } else if (win == MEL_WIN_RING) {
    if (db) MEL_LAUNCH(false, true, MEL_WIN_RING); else MEL_LAUNCH(false, false, MEL_WIN_RING);
  } else {
    if (db) MEL_LAUNCH(false, true, MEL_WIN_RINGS); else MEL_LAUNCH(false, false, MEL_WIN_RINGS);
  }
#undef MEL_LAUNCH
  if (db) power_to_db_launch(out, batch, (size_t)MEL_NMEL * T * channels, channels, mx, stream);
  return mmd_check_launch();
}

// one sample's power map: mmd_melspec_batch at batch 1, db 0
extern "C" int mmd_melspec_power(const float* wav_a, const float* wav_b, int channels, long long n_samples, const int* band_start,
                                 const int* band_len, const float* band_w, int band_stride, float* out, hipStream_t stream) {
  return melspec_launch(MEL_WIN_NONE, wav_a, wav_b, 1, channels, n_samples, nullptr, 0ll, band_start, band_len, band_w, band_stride, 0,
                        nullptr, out, stream);
}

extern "C" int mmd_melspec_batch(const float* wav_a, const float* wav_b, int batch, int channels, long long n_samples,
                                 const int* band_start, const int* band_len, const float* band_w, int band_stride, int db, float* max_ws,
                                 float* out, hipStream_t stream) {
  return melspec_launch(MEL_WIN_NONE, wav_a, wav_b, batch, channels, n_samples, nullptr, 0ll, band_start, band_len, band_w, band_stride,
                        db, max_ws, out, stream);
}

extern "C" int mmd_melspec_windows(const float* wav, int channels, long long n_total, const long long* win_start, int batch,
                                   long long win_len, const int* band_start, const int* band_len, const float* band_w, int band_stride,
                                   int db, float* max_ws, float* out, hipStream_t stream) {
  return melspec_launch(MEL_WIN_LINEAR, wav, nullptr, batch, channels, win_len, win_start, n_total, band_start, band_len, band_w,
                        band_stride, db, max_ws, out, stream);
}

// the ring mode of mmd_melspec_windows: cap in n_total's place
extern "C" int mmd_melspec_windows_ring(const float* ring, int channels, long long cap, const long long* win_start, int batch,
                                        long long win_len, const int* band_start, const int* band_len, const float* band_w,
                                        int band_stride, int db, float* max_ws, float* out, hipStream_t stream) {
  return melspec_launch(MEL_WIN_RING, ring, nullptr, batch, channels, win_len, win_start, cap, band_start, band_len, band_w,
                        band_stride, db, max_ws, out, stream);
}

// the rings of a bank of sessions: window b out of the ring of session win_sess[b]
extern "C" int mmd_melspec_windows_rings(const float* rings, int n_sessions, int channels, long long cap, const int* win_sess,
                                         const long long* win_start, int batch, long long win_len, const int* band_start,
                                         const int* band_len, const float* band_w, int band_stride, int db, float* max_ws, float* out,
                                         hipStream_t stream) {
  return melspec_launch(MEL_WIN_RINGS, rings, nullptr, batch, channels, win_len, win_start, cap, band_start, band_len, band_w,
                        band_stride, db, max_ws, out, stream, win_sess, n_sessions);
}

extern "C" int mmd_power_to_db(float* x, int batch, int h, int w, int channels, float* max_ws, hipStream_t stream) {
  if (!x || !max_ws || batch <= 0 || batch > 65535 || h <= 0 || w <= 0 || channels <= 0 || channels > MEL_DB_CMAX) return MMD_EINVAL;
  const size_t per_sample = (size_t)h * w * channels;
  unsigned int* mx = reinterpret_cast<unsigned int*>(max_ws);
  if (mel_zero_max(mx, batch, channels, stream) != MMD_OK) return MMD_ELAUNCH;
  const size_t blocks = (per_sample + 255) / 256;
  const dim3 grid((unsigned)(blocks < 1024 ? blocks : 1024), batch);
  hipLaunchKernelGGL(power_max_kernel, grid, dim3(256), 0, stream, x, per_sample, channels, mx);
  power_to_db_launch(x, batch, per_sample, channels, mx, stream);
  return mmd_check_launch();
}
