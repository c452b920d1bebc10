"""Helper (not a test): float64 numpy restatement of the waveform front end that csrc/melspec.hip computes.

`MultimodalDetection.merge_audios` (src/datasets/MultimodalDetection.py:329-353) and `Audio2Spectogram`
(src/datasets/transformations.py:251-266) call librosa 0.7.2's `feature.melspectrogram(sr=44100, n_fft=1024, hop_length=256,
n_mels=80)`.  librosa is neither part of the reference tree nor installed here, so this file restates the published arithmetic:

  y = (a + b) / 2 in float32 when two recordings are mixed
  reflect-pad n_fft / 2 samples at both ends (the edge sample is not repeated)
  frame t = padded[hop * t : hop * t + n_fft] * periodic Hann (0.5 - 0.5 cos(2 pi n / n_fft))
  real FFT, power re^2 + im^2 of bins 0..n_fft/2
  Slaney mel bank (htk=False, fmin=0, fmax=sr/2, area-normalised triangles), weights rounded to float32

PARITY UNPINNED against librosa itself; pinned by the closed forms in tests/test_melspec_cpu.py.  `dtype=np.float32` runs the
same chain in single precision (scipy.fft keeps float32 -> complex64), which is what librosa 0.7.2 itself computes (complex64
STFT, float32 bank): its distance from the float64 run is the yardstick of tests/test_gpu_melspec.py."""
import numpy as np

SR, N_FFT, HOP, N_MELS = 44100, 1024, 256, 80


def hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    lin = f / (200.0 / 3.0)
    log = 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0)
    return np.where(f >= 1000.0, log, lin)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), (200.0 / 3.0) * m)


def mel_frequencies(sr=SR, n_mels=N_MELS):
    """n_mels + 2 band edges in Hz, evenly spaced on the Slaney mel scale between 0 and sr / 2."""
    return mel_to_hz(np.linspace(hz_to_mel(0.0), hz_to_mel(sr / 2.0), n_mels + 2))


def mel_bank64(sr=SR, n_fft=N_FFT, n_mels=N_MELS):
    """[n_mels, 1 + n_fft/2] float64: row i = the triangle over [f[i], f[i+2]] peaking at f[i+1] with height 2 / (f[i+2] - f[i]),
    sampled at the FFT bin frequencies."""
    f = mel_frequencies(sr, n_mels)
    bins = np.linspace(0.0, sr / 2.0, 1 + n_fft // 2)
    w = np.zeros((n_mels, bins.size))
    for i in range(n_mels):
        lo, pk, hi = f[i], f[i + 1], f[i + 2]
        up = (bins - lo) / (pk - lo)              # 0 at lo, 1 at the peak
        down = (hi - bins) / (hi - pk)            # 1 at the peak, 0 at hi
        w[i] = np.maximum(np.minimum(up, down), 0.0) * (2.0 / (hi - lo))
    return w


def mel_bank32(sr=SR, n_fft=N_FFT, n_mels=N_MELS):
    return mel_bank64(sr, n_fft, n_mels).astype(np.float32)


def hann(n_fft=N_FFT, dtype=np.float64):
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)).astype(dtype)


def frames(y, n_fft=N_FFT, hop=HOP):
    """[T, n_fft] windows of the reflect-padded signal, T = 1 + len(y) // hop."""
    p = np.pad(y, n_fft // 2, mode="reflect")
    T = 1 + (p.size - n_fft) // hop
    idx = hop * np.arange(T)[:, None] + np.arange(n_fft)[None, :]
    return p[idx]


def mix(y_a, y_b=None):
    y = np.asarray(y_a, dtype=np.float32)
    if y_b is not None:
        y = (y + np.asarray(y_b, dtype=np.float32)) / np.float32(2.0)         # float32 arrays upstream: the mix is an fp32 operation
    return y


def power_spectrum(y, dtype=np.float64):
    """[1 + n_fft/2, T] |STFT|^2 of one channel."""
    import scipy.fft
    fr = frames(np.asarray(y, dtype=dtype)) * hann(dtype=dtype)[None, :]
    z = scipy.fft.rfft(fr, axis=1)                 # float32 in -> complex64 out
    assert z.dtype == (np.complex128 if dtype == np.float64 else np.complex64)
    return (z.real ** 2 + z.imag ** 2).T


def melspec_ref(y_a, y_b=None, dtype=np.float64):
    """One channel: float32 waveform(s) [N] -> power mel spectrogram [80, T] in `dtype` arithmetic."""
    bank = mel_bank32().astype(dtype)
    return bank @ power_spectrum(mix(y_a, y_b), dtype)
