"""Reading a recording from disk, whole or a chunk at a time: `.npy` waveforms and 8-channel PCM `.wav` files.  Only numpy and `wave`:
nothing here touches torch or the device.  What a `LiveSession` or `LiveBank` is fed from a file comes from `open_chunks`."""
import os
import wave

import numpy as np

CHANNELS, SAMPLE_RATE = 8, 44100


def _check_npy(path: str, a, one: bool = False):
    """The rules of a `.npy`: float32 [8, N] or [B, 8, N] -> [B, 8, N], a view of `a`; one: ONE recording, B = 1"""
    if a.dtype != np.float32:
        raise ValueError(f"{path}: waveforms must be float32, found {a.dtype}")
    b = a[None] if a.ndim == 2 else a
    if b.ndim == 3 and b.shape[1] == CHANNELS and (b.shape[0] == 1 or not one):
        return b
    if not one:
        raise ValueError(f"{path}: expected [{CHANNELS}, N] or [B, {CHANNELS}, N] waveforms, found shape {b.shape}")
    raise ValueError(f"{path}: --window_s takes ONE recording (a .wav, or a .npy of shape [{CHANNELS}, N]), "
                     f"found shape {(b[0] if b.ndim == 3 and b.shape[0] == 1 else b).shape}")


def _check_wav(path: str, w, any_rate: bool):
    """The header rules of an open `wave` reader -> (bytes per sample, rate in Hz).  any_rate False: 8 channels of 16-bit PCM at 44.1 kHz,
    what the front end takes as it is; True: 8 channels of 16-, 24- or 32-bit PCM at any rate, what the device decodes and resamples."""
    width, rate, channels = w.getsampwidth(), w.getframerate(), w.getnchannels()
    if not any_rate and rate != SAMPLE_RATE:
        raise ValueError(f"{path}: sample rate {rate} Hz is not supported (the front end is built for {SAMPLE_RATE} Hz; resample first)")
    if w.getcomptype() != "NONE" or width not in ((2, 3, 4) if any_rate else (2,)):
        bits = "16-, 24- or 32-bit" if any_rate else "16-bit"
        raise ValueError(f"{path}: only {bits} PCM is supported, found {8 * width}-bit {w.getcomptype()}")
    if channels != CHANNELS:
        raise ValueError(f"{path}: expected {CHANNELS} microphone channels, found {channels}")
    if rate < 1:
        raise ValueError(f"{path}: sample rate {rate} Hz")
    return width, rate


def _read_frames(path: str, any_rate: bool):
    """-> (all frames of a `.wav` as they are in the file, bytes per sample, rate in Hz)"""
    with wave.open(path, "rb") as w:
        width, rate = _check_wav(path, w, any_rate)
        return w.readframes(w.getnframes()), width, rate


def read_npy(path: str) -> np.ndarray:
    return np.ascontiguousarray(_check_npy(path, np.load(path, allow_pickle=False)))


def read_wav(path: str) -> np.ndarray:
    pcm = np.frombuffer(_read_frames(path, any_rate=False)[0], dtype="<i2").reshape(-1, CHANNELS)
    return np.ascontiguousarray((pcm.astype(np.float32) / np.float32(32768.0)).T)[None]


def read_input(path: str) -> np.ndarray:
    """-> float32 [B, 8, N]"""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npy":
        return read_npy(path)
    if ext == ".wav":
        return read_wav(path)
    raise ValueError(f"{path}: unsupported input (a .npy of float32 waveforms or an 8-channel 16-bit PCM .wav at 44.1 kHz)")


def read_recording(path: str):
    """A PCM `.wav` of 8 channels at ANY rate, 16-, 24- or 32-bit -> (its frames as a uint8 array, just as they are in the file:
    interleaved little-endian signed samples; frames; channels; bytes per sample; rate in Hz).  Nothing is decoded on the host:
    `Resampler.pcm_to_float` and `Resampler.resample` take it from there."""
    raw, width, rate = _read_frames(path, any_rate=True)
    raw = np.frombuffer(raw, dtype=np.uint8)
    frames = raw.size // (CHANNELS * width)
    if frames < 1:
        raise ValueError(f"{path}: no frames")
    return raw[:frames * CHANNELS * width].copy(), frames, CHANNELS, width, rate


def _wav_chunks(w, chunk: int, width: int):
    """(raw whole frames, bytes per sample) of an open `wave` reader, `chunk` frames at a time; closes the reader behind the last"""
    with w:
        while True:
            raw = w.readframes(chunk)
            if len(raw) < width * CHANNELS:
                return
            yield raw[:len(raw) - len(raw) % (width * CHANNELS)], width


def open_chunks(path: str, seconds: float, any_rate: bool, sample_rate=None):
    """-> (n_frames, rate, chunks): the recording's length in frames at its own rate in Hz and an iterator over it round(seconds * rate)
    frames at a time - (raw frames, bytes per sample) of a `.wav` (for `push_pcm`), (float32 [8, n], None) of a `.npy` of ONE recording
    read through a memory map (for `push`).  any_rate False: a 16-bit `.wav` at 44.1 kHz, `read_wav`'s checks; True: 16-, 24- or 32-bit
    PCM at the rate in its header, `read_recording`'s checks.  A `.npy` is taken to be at sample_rate (default 44100).  Only one chunk
    is in host memory at a time; a refused `.wav` is closed before the refusal is raised."""
    if os.path.splitext(path)[1].lower() == ".wav":
        w = wave.open(path, "rb")
        try:
            width, rate = _check_wav(path, w, any_rate)
            chunk = int(round(seconds * rate))
            if chunk < 1:
                raise ValueError(f"--live_s {seconds}: a positive number of seconds (at least one frame at {rate} Hz)")
        except ValueError:
            w.close()
            raise
        return w.getnframes(), rate, _wav_chunks(w, chunk, width)
    rate = SAMPLE_RATE if sample_rate is None else int(sample_rate)
    m, chunk = _check_npy(path, np.load(path, mmap_mode="r", allow_pickle=False), one=True)[0], int(round(seconds * rate))
    return m.shape[1], rate, ((np.ascontiguousarray(m[:, i:i + chunk]), None) for i in range(0, m.shape[1], chunk))
