#!/usr/bin/env python3
"""Times `mot.hota_metrics` (csrc/moteval.hip: mmd_hota_align, mmd_hota_match, mmd_hota_assoc) against tests/hota_ref.py, the numpy / scipy
restatement on the host, on the workload of profiles/mot_eval_notes.md: --windows windows per session (36 000), five lanes, a vehicle
crosses a lane in 400 windows, 5 % of its detections are missing and each lane is empty for five windows between two vehicles.  Ground
truth: the detections tracked by `tracker.track_rows` with TrackConfig(max_age=8); hypothesis: 90 % of the rows, every edge jittered
with sigma 1.5 px, tracked with the default TrackConfig().  Sessions are seeds of the same generator stacked with a session column.

A host clock around the whole call (host preparation, upload, three launches, synchronise, copy back), the median of --reps calls after
one warm-up call; then ONE call with a synchronise behind every launch, which gives the three launches apart; `mot.mot_metrics` (the
CLEAR walk and the identity measures) on the same input beside it; the restatement once (--no_ref leaves it out).  The figures of the
two must agree within the tests' bound; the script reports whether they do (the input is not checked for tied matchings).

    python tools/dev/time_hota.py [--sessions 1 16] [--windows 36000] [--reps 3] [--no_ref] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from mm_distillnet_amd import mot  # noqa: E402
from mm_distillnet_amd.tracker import TrackConfig, track_rows  # noqa: E402

DEV = "cuda:0"


def session(seed, W, lanes=5, cross=400, gap=5):
    """-> (gt, hyp): (rows, window, track) each"""
    r = np.random.RandomState(seed)
    w = np.repeat(np.arange(W), lanes)
    k = np.tile(np.arange(lanes), W)
    t = (w + 81 * k) % (cross + gap)                      # the vehicle's age on its lane; the last `gap` windows of a period are empty
    keep = (t < cross) & (r.rand(len(w)) >= 0.05)
    w, k, t = w[keep], k[keep], t[keep]
    x, y = 0.5 * t, 40.0 * k
    rows = np.stack([x, y, x + 30.0, y + 20.0, np.full(len(w), 0.9), np.where(k % 2, 6.0, 14.0)], axis=1).astype(np.float32)
    gt_ids = track_rows(rows, w, W, TrackConfig(max_age=8), DEV)
    assert (gt_ids >= 0).all()
    sel = r.rand(len(w)) < 0.9
    noisy = rows[sel].copy()
    noisy[:, :4] += r.normal(0, 1.5, (int(sel.sum()), 4)).astype(np.float32)
    hyp_ids = track_rows(noisy, w[sel], W, TrackConfig(), DEV)
    return (rows, w, gt_ids.astype(np.int64)), (noisy, w[sel], hyp_ids.astype(np.int64))


def stack(parts):
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3)) + (np.concatenate([np.full(len(p[0]), s, np.int64) for s, p in enumerate(parts)]),)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--windows", type=int, default=36000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no_ref", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    made = [session(100 + s, a.windows) for s in range(max(a.sessions))]
    res = []
    for S in a.sessions:
        gt, hyp = stack([m[0] for m in made[:S]]), stack([m[1] for m in made[:S]])
        whole, clear = [], []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            got = mot.hota_metrics(gt, hyp, a.windows, DEV)
            t1 = time.perf_counter()
            mot.mot_metrics(gt, hyp, a.windows, DEV)
            t2 = time.perf_counter()
            if rep:              # rep 0 warms both up (code objects, allocator)
                whole.append(t1 - t0); clear.append(t2 - t1)
        t0 = time.perf_counter()
        prep = mot.hota_prepare(gt, hyp, a.windows)
        t_prep = time.perf_counter() - t0
        parts = {}
        mot.hota_run_device(prep, DEV, times=parts)
        row = {"sessions": S, "windows": a.windows, "rows_gt": len(gt[0]), "rows_hyp": len(hyp[0]),
               "tracks_gt": int(np.diff(prep["gt"]["trk_off"]).max()), "tracks_hyp": int(np.diff(prep["hyp"]["trk_off"]).max()),
               "cells": int(prep["c_off"][-1]), "reps": a.reps,
               "hota_s_median": float(np.median(whole)), "hota_s_min": float(np.min(whole)), "hota_s_max": float(np.max(whole)),
               "mot_metrics_s_median": float(np.median(clear)), "prepare_s": t_prep, **{k + "_s": float(v) for k, v in parts.items()},
               **{k: got["overall"][k] for k in mot.HOTA_KEYS}}
        if not a.no_ref:
            import hota_ref
            t0 = time.perf_counter()
            ref = hota_ref.evaluate(gt, hyp, a.windows)
            row["hota_ref_s"] = time.perf_counter() - t0
            bound = (max(ref["cells"]) + 10) * 2.0 ** -52
            row["largest_relative_difference"] = max(abs(got["overall"][k] - ref["overall"][k]) / abs(ref["overall"][k]) for k in mot.HOTA_KEYS)
            row["agrees_with_hota_ref"] = bool(row["largest_relative_difference"] <= bound
                                               and np.array_equal(got["alphas"]["overall"]["tp"], ref["alphas"]["overall"]["tp"]))
        print(json.dumps(row), flush=True)
        res.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
