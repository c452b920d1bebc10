"""Latency of the waveform front end and of the audio-only detector (figures of profiles/melspec_db_notes.md).

    python tools/dev/time_audio_detector.py [--reps 200] [--warmup 20]

Front end, B = 8, C = 8, N = 44100, S = 512: the batched path (mmd_melspec_batch + mmd_resize_cubic_batch) with db = 0 and db = 1 against
the per-sample path of the previous front end (8 x mmd_melspec_power + 8 x mmd_resize_cubic), device events around each repetition, medians.
Detector, D2 at 512 x 512, B = 1 and B = 8, waveform to rows on the host: eager launches against graph replay, host wall time per call
(the call ends with the synchronize and the device-to-host copy of the rows), medians."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from mm_distillnet_amd import _lib  # noqa: E402
from mm_distillnet_amd.arch import make_spec  # noqa: E402
from mm_distillnet_amd.audio import MelFrontEnd  # noqa: E402
from mm_distillnet_amd.data import synthetic_waveforms  # noqa: E402
from mm_distillnet_amd.detector import AudioDetector  # noqa: E402
from mm_distillnet_amd.synth import synth_state  # noqa: E402

DEV = "cuda:0"


def events(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out), min(out), max(out)


def wall(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        t = time.perf_counter(); fn(); out.append((time.perf_counter() - t) * 1e6)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    print("device:", torch.cuda.get_device_name(0))
    B, C, N, S = 8, 8, 44100, 512
    fe = MelFrontEnd(DEV)
    wav = torch.stack([synthetic_waveforms(24, i, N) for i in range(B)]).to(DEV)
    T = fe.n_frames(N)
    mel, out = torch.empty(B, 80, T, C, device=DEV), torch.empty(B, C, S, S, device=DEV)

    def per_sample():
        for b in range(B):
            _lib.call("mmd_melspec_power", wav[b], None, C, N, fe.start, fe.length, fe.band, fe.stride, mel[b])
        for b in range(B):
            _lib.call("mmd_resize_cubic", mel[b], 80, T, C, S, out[b])

    for order in range(2):          # twice, alternating: the second pass shows whether the order mattered
        for name, fn in (("per-sample power (16 launches)", per_sample),
                         ("batched db=0 (student_input)", lambda: fe.student_input(wav, None, S)),
                         ("batched db=1 (student_input)", lambda: fe.student_input(wav, None, S, db=True))):
            print("front end pass %d %-34s median %.1f us (min %.1f, max %.1f)" % ((order, name) + events(fn, a.reps, a.warmup)))

    spec = make_spec(2, 8)
    state = synth_state(spec, seed=7, cls_bias=-2.0)
    for batch in (1, 8):
        w = wav[:batch].contiguous()
        for graph in (False, True):
            det = AudioDetector(spec, DEV, image_size=S)
            det.load(state)
            det.use_graph = graph
            rows = det.detect(w)
            med, lo, hi = wall(lambda: det.detect(w), max(20, a.reps // 4), 5)
            print("detector B=%d %-6s waveform -> rows: median %.0f us (min %.0f, max %.0f); %d boxes; replays %d"
                  % (batch, "graph" if graph else "eager", med, lo, hi, sum(len(r) for r in rows), det.graph_replays))
            det.check_overflow()


if __name__ == "__main__":
    main()
