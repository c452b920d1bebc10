"""Host time of the live pushes that complete NO group / tick - one staging copy, one ring write (at 48 kHz also a resampling launch), the
schedule - for a session and for a bank of 4 sessions, at 44.1 and at 48 kHz (figures of profiles/live_host_path_notes.md).

    python tools/dev/time_live_idle_push.py [--seconds 20] [--root DIR]

D2 at 128 x 128 with hash weights (the forward pass is not what is timed), one-second windows every 0.1 s at batch 8, host chunks of
0.01 s from `synthetic_waveforms`; the first 200 such pushes of every case are left out.  --root: the checkout whose package is imported
(default: this one), so an older commit runs unchanged.  One JSON line: per case the count, the median and the first decile in us."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
ap.add_argument("--seconds", type=float, default=20.0)
a = ap.parse_args()
sys.path.insert(0, a.root)

import torch  # noqa: E402

from mm_distillnet_amd.arch import make_spec  # noqa: E402
from mm_distillnet_amd.data import synthetic_waveforms  # noqa: E402
from mm_distillnet_amd.detector import AudioDetector  # noqa: E402
from mm_distillnet_amd.synth import synth_state  # noqa: E402

SR = 44100
WIN, HOP, CHUNK = SR, SR // 10, SR // 100
torch.cuda.set_device(0)
spec = make_spec(2, 8)
det = AudioDetector(spec, "cuda:0", image_size=128)
det.load(synth_state(spec, seed=7, cls_bias=-2.0))
n = int(a.seconds * SR)
out = dict(root=a.root)
for leg, sessions in (("single", 1), ("bank", 4)):
    w = [synthetic_waveforms(24, i, n) for i in range(sessions)]
    for rate in (None, 48000):
        if leg == "single":
            obj = det.open_stream(WIN, HOP, batch=8, sample_rate=rate)
            push = lambda s, c: obj.push(c)
            done = lambda: obj.group
        else:
            obj = det.open_bank(sessions, WIN, HOP, batch=8, sample_rates=None if rate is None else [rate] * sessions)
            push = lambda s, c: obj.push(s, c)
            done = lambda: len(obj.ticks)
        idle = []
        for lo in range(0, n, CHUNK):
            for s in range(sessions):
                before = done()
                c = w[s][:, lo:lo + CHUNK]
                t = time.perf_counter()
                push(s, c)
                dt = (time.perf_counter() - t) * 1e6
                if done() == before:
                    idle.append(dt)
            if lo % (50 * CHUNK) == 0:
                torch.cuda.synchronize()      # keep the queue short: the idle pushes never wait for the device themselves
        torch.cuda.synchronize()
        obj.close()
        idle = idle[200:]
        out["%s_%s" % (leg, rate or 44100)] = dict(n=len(idle), median_us=round(statistics.median(idle), 2),
                                                   p10_us=round(statistics.quantiles(idle, n=10)[0], 2))
print(json.dumps(out))
