#!/usr/bin/env python3
"""Times the tracker's two association rules (csrc/track.hip; TrackConfig(assign="greedy" | "optimal")) for profiles/track_assign_notes.md.

`tracker.track_rows` - a host clock around the whole call (packing, upload, one launch per group, synchronise, copy back), the median
of --reps calls after one warm-up call - on two workloads:
  sparse  --windows windows (36 000) of five lanes, the scale and the generator of profiles/mot_eval_notes.md (tools/dev/time_hota.py):
          a vehicle crosses a lane in 400 windows, 5 % of its detections are missing, every edge jittered with sigma 1.5 px
  dense   2 000 windows of 64 vehicles on an 8 x 8 grid of pitch 12 px, boxes of 30 px (each may pair with its neighbours), drifting and
          jittered with sigma 1.5 px, 5 % of the detections missing
Then the update kernel alone: --launches launches of ONE group back to back between two events, on a fresh copy of a state that the
same group left (so every launch does the association work of live tracks): a group of 8 windows of the dense workload, one of the
sparse workload, and - once, a single launch - the worst case, one window of 256 boxes on 256 live tracks in which every pair is allowed.

--root DIR imports the package from another tree (the parent commit's, with its own library): the rules that tree does not know are
left out.

    python tools/dev/time_track_assign.py [--root DIR] [--windows 36000] [--reps 3] [--launches 200] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

DEV = "cuda:0"


def sparse(seed, W, lanes=5, cross=400, gap=5):
    r = np.random.RandomState(seed)
    w = np.repeat(np.arange(W), lanes)
    k = np.tile(np.arange(lanes), W)
    t = (w + 81 * k) % (cross + gap)
    keep = (t < cross) & (r.rand(len(w)) >= 0.05)
    w, k, t = w[keep], k[keep], t[keep]
    x, y = 0.5 * t, 40.0 * k
    rows = np.stack([x, y, x + 30.0, y + 20.0, np.full(len(w), 0.9), np.where(k % 2, 6.0, 14.0)], axis=1).astype(np.float32)
    rows[:, :4] += r.normal(0, 1.5, (len(w), 4)).astype(np.float32)
    return rows, w


def dense(seed, W, side=8, pitch=12.0, size=30.0):
    r = np.random.RandomState(seed)
    n = side * side
    w = np.repeat(np.arange(W), n)
    k = np.tile(np.arange(n), W)
    keep = r.rand(len(w)) >= 0.05
    w, k = w[keep], k[keep]
    x, y = pitch * (k % side) + 0.25 * (w % 40), pitch * (k // side) + 0.1 * (w % 40)
    rows = np.stack([x, y, x + size, y + size, np.full(len(w), 0.9), np.full(len(w), 6.0)], axis=1).astype(np.float32)
    rows[:, :4] += r.normal(0, 1.5, (len(w), 4)).astype(np.float32)
    return rows, w


def full(n=256):
    """two windows of n nearly coincident boxes: every pair of the second window is allowed"""
    r = np.random.RandomState(1)
    rows = np.tile(np.array([[10.0, 10.0, 110.0, 110.0, 0.9, 6.0]], np.float32), (2 * n, 1))
    rows[:, :4] += r.uniform(-2, 2, (2 * n, 4)).astype(np.float32)
    return rows, np.repeat(np.arange(2), n)


def kernel_alone(tracker, rows, window, first, group, cfg, launches):
    """us per launch of the group of windows first .. first + group - 1, the state being what the windows before AND that group left"""
    sel = window < first + group
    state = tracker.new_state(DEV, cfg)
    tracker.track_rows(rows[sel], window[sel], first + group, cfg, DEV, group=group, state=state)
    m = (window >= first) & (window < first + group)
    counts = np.bincount(window[m] - first, minlength=group)
    cap = max(1, int(counts.max()))
    packed = np.zeros((group, cap, 6), np.float32)
    at = np.concatenate([[0], np.cumsum(counts)])
    packed[window[m] - first, np.arange(int(m.sum())) - at[window[m] - first]] = rows[m]
    packed_d, cnt_d = torch.from_numpy(packed).to(DEV), torch.from_numpy(counts.astype(np.int32)).to(DEV)
    ctl = torch.tensor([group, first], dtype=torch.int32, device=DEV)
    rec_count = torch.zeros(1, dtype=torch.int32, device=DEV)
    rec_track = torch.full((max(1, int(m.sum())),), -1, dtype=torch.int32, device=DEV)
    keep = [t.clone() for t in state]
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(4):
        for t, k in zip(state, keep):
            t.copy_(k)
        torch.cuda.synchronize()
        a.record()
        for _ in range(launches):
            tracker.update(packed_d, cnt_d, ctl, rec_count, len(rec_track), rec_track, state, cfg)
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / launches)
    return {"rows_in_group": int(m.sum()), "live_tracks": int((keep[0][:, 0] != 0).sum()), "us_per_launch": out[1:], "overflow": int(state[1][1].item())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--windows", type=int, default=36000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    sys.path.insert(0, os.path.abspath(a.root))
    from mm_distillnet_amd import tracker
    rules = ["greedy", "optimal"] if "assign" in tracker.TrackConfig.__dataclass_fields__ else [None]
    res = {"root": os.path.abspath(a.root), "rules": rules}
    for name, (rows, window), W, slots in (("sparse", sparse(100, a.windows), a.windows, 64), ("dense", dense(100, 2000), 2000, 256)):
        ids = {}
        for rule in rules:
            cfg = tracker.TrackConfig(max_tracks=slots, **({} if rule is None else {"assign": rule}))
            for group in (8, 1024):
                times = []
                for rep in range(a.reps + 1):
                    t0 = time.perf_counter()
                    ids[rule] = tracker.track_rows(rows, window, W, cfg, DEV, group=group)
                    times.append(time.perf_counter() - t0)
                res["%s/%s/group%d" % (name, rule, group)] = {"rows": len(rows), "windows": W, "tracks": int(ids[rule].max()) + 1,
                                                             "s_median": float(np.median(times[1:])), "s_all": times[1:]}
            res["%s/%s/kernel_group8" % (name, rule)] = kernel_alone(tracker, rows, window, 800, 8, cfg, a.launches)
        if len(rules) == 2:
            res[name + "/rows_whose_id_differs"] = int((ids["greedy"] != ids["optimal"]).sum())
    rows, window = full()
    for rule in rules:
        cfg = tracker.TrackConfig(max_tracks=256, iou_min=0.3, **({} if rule is None else {"assign": rule}))
        res["full256/%s/kernel_one_window" % rule] = kernel_alone(tracker, rows, window, 1, 1, cfg, 1)
    print(json.dumps(res, indent=1), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
