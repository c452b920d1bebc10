"""Host time per tick of a live session bank against a single live session at the same batch size (figures of
profiles/live_bank_notes.md).

    python tools/dev/time_live_bank.py --leg bank   [--sessions 8] [--batch 8] [--seconds 6] [--root DIR]
    python tools/dev/time_live_bank.py --leg single [--batch 8]    [--seconds 6] [--root DIR]

D2 at 512 x 512 with hash weights (tools/dev/time_audio_detector.py's detector), one-second windows every 0.1 s, host chunks of 0.1 s
from `synthetic_waveforms`.  bank: `--sessions` recordings pushed in round robin through `AudioDetector.open_bank`; single: one
recording through `AudioDetector.open_stream`.  Timed: the wall time of every push that completed a tick / group (it ends with the
rows on the host), and - bank - the wall time from the start of the round's first push to the end of the push that ran the round's
tick: the delay of the window that waited longest.  --root: the checkout whose package is imported (default: this one), so the single
leg runs unchanged on an older commit.  One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--leg", choices=("bank", "single"), required=True)
ap.add_argument("--sessions", type=int, default=8)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--seconds", type=float, default=6.0)
ap.add_argument("--warmup", type=int, default=5, help="ticks / groups left out of the figures")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
a = ap.parse_args()
sys.path.insert(0, a.root)

import torch  # noqa: E402

from mm_distillnet_amd.arch import make_spec  # noqa: E402
from mm_distillnet_amd.data import synthetic_waveforms  # noqa: E402
from mm_distillnet_amd.detector import AudioDetector  # noqa: E402
from mm_distillnet_amd.synth import synth_state  # noqa: E402

DEV, SR, S = "cuda:0", 44100, 512
WIN, HOP, CHUNK = SR, SR // 10, SR // 10


def med(v):
    v = v[a.warmup:]
    return dict(n=len(v), median_us=round(statistics.median(v), 1), min_us=round(min(v), 1), max_us=round(max(v), 1))


def main():
    torch.cuda.set_device(0)
    spec = make_spec(2, 8)
    det = AudioDetector(spec, DEV, image_size=S)
    det.load(synth_state(spec, seed=7, cls_bias=-2.0))
    n = int(a.seconds * SR)
    out = dict(leg=a.leg, batch=a.batch, device=torch.cuda.get_device_name(0), root=a.root)
    if a.leg == "single":
        w = synthetic_waveforms(24, 0, n)
        session = det.open_stream(WIN, HOP, batch=a.batch)
        group, rows = [], 0
        for lo in range(0, n, CHUNK):
            t = time.perf_counter()
            got = session.push(w[:, lo:lo + CHUNK])
            dt = (time.perf_counter() - t) * 1e6
            if session.group > len(group):
                group.append(dt)
                rows += len(got[0])
        session.close()
        out.update(group=med(group), rows=rows, replays=det.live_replays)
    else:
        w = [synthetic_waveforms(24, i, n) for i in range(a.sessions)]
        bank = det.open_bank(a.sessions, WIN, HOP, batch=a.batch)
        tick, delay, rows = [], [], 0
        for lo in range(0, n, CHUNK):
            t0 = time.perf_counter()
            for s in range(a.sessions):
                before = len(bank.ticks)
                t = time.perf_counter()
                got = bank.push(s, w[s][:, lo:lo + CHUNK])
                end = time.perf_counter()
                if len(bank.ticks) > before:
                    tick.append((end - t) * 1e6)
                    delay.append((end - t0) * 1e6)
                    rows += len(got[0])
        bank.close()
        out.update(sessions=a.sessions, tick=med(tick), delay=med(delay), rows=rows, replays=det.bank_replays)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
