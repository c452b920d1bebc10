#!/usr/bin/env python3
"""Figures of profiles/live_resample_notes.md: what one `push` of a 0.1 s host chunk costs a live session (`AudioDetector.open_stream`)
at 44.1 kHz - no resampling: the launches of the session before `sample_rate` existed - and at 48 kHz and 192 kHz, where the chunk goes
through the input ring and `mmd_ring_resample`; split into pushes that complete no group and pushes that complete one.

The detector is the set-up of profiles/live_session_notes.md: D2 student with synthetic weights (classifier bias tuned to about 40
candidates per window), S = 512, window 1.0 s, hop 0.1 s, batch 8, cand_cap = 4096.  Run on the GPU:
`python tools/dev/live_resample_figures.py [--seconds 20] [--rounds 3] [--rates 44100,48000,192000]`; under a kernel trace give
`--rounds 1` and read `ring_resample_kernel` out of the trace's statistics.
"""
import argparse
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
from mm_distillnet_amd.audio import MelFrontEnd  # noqa: E402
from mm_distillnet_amd.data import synthetic_waveforms  # noqa: E402
from mm_distillnet_amd.detector import AudioDetector  # noqa: E402
from mm_distillnet_amd.synth import tune_teacher_bias  # noqa: E402

DEV = "cuda:0"
S, WIN, HOP, BATCH = 512, 44100, 4410, 8


def say(*a):
    print(*a, flush=True)


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))]


def one_recording(session, chunks):
    """-> (wall s of the whole recording, [(host s of the call, s until the device is idle, groups completed)] per push, rows)"""
    session.reset()
    per_push, rows = [], 0
    torch.cuda.synchronize()
    start = time.perf_counter()
    for c in chunks:
        g0 = session.group
        t0 = time.perf_counter()
        out = session.push(c)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        per_push.append((t1 - t0, t2 - t0, session.group - g0))
        rows += len(out[0])
    rows += len(session.flush()[0])
    torch.cuda.synchronize()
    return time.perf_counter() - start, per_push, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rates", type=str, default="44100,48000,192000")
    a = ap.parse_args()
    rates = [int(r) for r in a.rates.split(",")]
    torch.cuda.set_device(0)
    spec, st = make_state(2, 8, 13, "audio")
    w44 = synthetic_waveforms(24, 11, a.seconds * 44100).to(DEV)
    windows = torch.stack([w44[:, k * WIN:(k + 1) * WIN] for k in range(8)]).contiguous()
    tune_teacher_bias(spec, st, MelFrontEnd(DEV).student_input(windows, None, S, db=True).cpu(), DEV, 40)
    det = AudioDetector(spec, DEV, image_size=S, cand_cap=4096)
    det.load(st)
    chunks = {}
    for r in rates:                                                                  # the same tones written down at each rate
        w = synthetic_waveforms(24, 11, a.seconds * r, sr=r).numpy()
        chunks[r] = [np.ascontiguousarray(w[:, i:i + r // 10]) for i in range(0, w.shape[1], r // 10)]
    figures = {r: dict(wall=[], idle=[], group=[], host_idle=[], host_group=[]) for r in rates}
    for rnd in range(a.rounds + 1):                                                  # round 0 warms up: a new session captures its graph
        for r in rates:                                                              # the rates alternate within a round
            session = det.open_stream(WIN, HOP, batch=BATCH, sample_rate=r)
            one_recording(session, chunks[r][:30])
            wall, per_push, rows = one_recording(session, chunks[r])
            session.close()
            if rnd == 0:
                say("%6d Hz: %d chunks of %d samples, %d rows, input ring %s" % (r, len(chunks[r]), r // 10, rows, session.in_ring_len))
                continue
            f = figures[r]
            f["wall"].append(wall)
            f["host_idle"] += [h for h, _, g in per_push if g == 0]
            f["idle"] += [d for _, d, g in per_push if g == 0]
            f["host_group"] += [h for h, _, g in per_push if g == 1]
            f["group"] += [d for _, d, g in per_push if g == 1]
    for r in rates:
        f = figures[r]
        say("%6d Hz  recording of %d s in 0.1 s host chunks, wall s per round: %s" % (r, a.seconds, " ".join("%.4f" % t for t in f["wall"])))
        for name, what in (("idle", "push completing NO group, call + wait until the device is idle"),
                           ("host_idle", "push completing NO group, host time of the call alone"),
                           ("group", "push completing a group, call + wait"), ("host_group", "push completing a group, the call alone")):
            xs = f[name]
            say("%6d Hz  %-68s n %4d  median %8.1f us  p90 %8.1f us  max %8.1f us" %
                (r, what, len(xs), 1e6 * statistics.median(xs), 1e6 * pct(xs, 0.9), 1e6 * max(xs)))


if __name__ == "__main__":
    main()
