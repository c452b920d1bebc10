#!/usr/bin/env python3
"""Figures of profiles/resample_notes.md, section "Time": 60 s of 8-channel audio through `mmd_resample_poly` per input rate, the
48 kHz recording's `mmd_pcm_to_float` per sample width, and that recording's `detect_stream` beside decode + resample.

The detector is the set-up of profiles/stream_detect_notes.md: D2 student with synthetic weights (classifier bias tuned to about 40
candidates per window), S = 512, window 1.0 s, hop 0.1 s, batch 8.  Run on the GPU: `python tools/dev/resample_figures.py`.
"""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import make_state  # noqa: E402
from mm_distillnet_amd.audio import MelFrontEnd, Resampler  # noqa: E402
from mm_distillnet_amd.data import synthetic_waveforms  # noqa: E402
from mm_distillnet_amd.detector import AudioDetector  # noqa: E402
from mm_distillnet_amd.synth import tune_teacher_bias  # noqa: E402

DEV = "cuda:0"
S, SECONDS, CHANNELS = 512, 60, 8
RATES = (48000, 16000, 22050, 96000, 192000)


def say(*a):
    print(*a, flush=True)


def fmt(ts, digits=3):
    return " ".join("%.*f" % (digits, t) for t in ts)


def event_ms(fn, reps=20, warm=3):
    """ms per call between two device events, five windows of `reps` calls after a warm-up"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / reps)
    return ts


def wall_s(fn, n=5):
    """host clock around a call that ends in a device synchronise"""
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts


def pcm_frames(wav, width):
    """[8, N] floats -> (interleaved little-endian signed PCM of `width` bytes as uint8, frames)"""
    s16 = np.clip(np.rint(wav * 0.5 * 32768.0), -32768, 32767).astype(np.int64).T
    s = s16 << (8 * (width - 2))
    le = s.astype("<i8").view(np.uint8).reshape(s.shape[0], s.shape[1], 8)[:, :, :width]
    return np.ascontiguousarray(le).reshape(-1), s.shape[0]


def time_resample(rs):
    rec48 = None
    for sr in RATES:
        n = SECONDS * sr
        if sr == 48000:
            w = synthetic_waveforms(24, 3, n, sr=sr)
        else:
            w = torch.randn(CHANNELS, n, generator=torch.Generator().manual_seed(sr)) * 0.3
        wd = w.to(DEV)
        ts = event_ms(lambda: rs.resample(wd, sr))
        L, M, taps, _, _ = rs._bank(sr, 44100)
        n_out = -((-n * L) // M)
        med = statistics.median(ts)
        say("resample %6d -> 44100, 8 x %d samples, L/M %d/%d taps %d: ms per call %s  median %.3f  %.0f GFLOP/s (2 * taps per output)" %
            (sr, n, L, M, taps, fmt(ts), med, 2.0 * CHANNELS * n_out * taps / med / 1e6))
        if sr == 48000:
            rec48 = w.numpy()
        del wd
    return rec48


def time_pcm(rs, rec48):
    raw16 = None
    for width in (2, 3, 4):
        raw, frames = pcm_frames(rec48, width)
        rd = torch.from_numpy(raw).to(DEV)
        ts = event_ms(lambda: rs.pcm_to_float(rd, frames, CHANNELS, width))
        med = statistics.median(ts)
        say("pcm_to_float %d-bit, %d frames x 8: ms per call %s  median %.3f  %.0f GB/s (bytes in + floats out)" %
            (8 * width, frames, fmt(ts), med, (raw.size + 4.0 * frames * CHANNELS) / med / 1e6))
        if width == 2:
            raw16 = rd
    return raw16, rec48.shape[1]


def time_stream(rs, raw16, frames):
    def decode_and_resample():
        return rs.resample(rs.pcm_to_float(raw16, frames, CHANNELS, 2), 48000)

    wav44 = decode_and_resample()
    spec, st = make_state(2, 8, 13, "audio")
    windows = torch.stack([wav44[:, k * 44100:(k + 1) * 44100] for k in range(8)]).contiguous()
    tune_teacher_bias(spec, st, MelFrontEnd(DEV).student_input(windows, None, S, db=True).cpu(), DEV, 40)
    det = AudioDetector(spec, DEV, image_size=S)
    det.load(st)
    rows, win = det.detect_stream(wav44, 44100, 4410, batch=8)            # captures the graph
    say("detect_stream on %s: %d windows, %d rows" % (tuple(wav44.shape), int(win.max()) + 1 if len(win) else 0, len(rows)))
    ts = wall_s(lambda: det.detect_stream(wav44, 44100, 4410, batch=8))
    tw = wall_s(decode_and_resample)
    a, b = statistics.median(tw), statistics.median(ts)
    say("detect_stream, s per recording: %s  median %.4f" % (fmt(ts, 4), b))
    say("pcm_to_float (16-bit) + resample, s per recording: %s  median %.5f" % (fmt(tw, 5), a))
    say("share of decode + resample in (decode + resample + detect_stream): %.2f %%" % (100.0 * a / (a + b)))


def main():
    torch.cuda.set_device(0)
    rs = Resampler(DEV)
    rec48 = time_resample(rs)
    raw16, frames = time_pcm(rs, rec48)
    time_stream(rs, raw16, frames)


if __name__ == "__main__":
    main()
