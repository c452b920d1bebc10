#!/usr/bin/env python3
"""Times the end of an evaluation both ways on synthetic records that lie on the device, as begin_eval lays them out:
    host  : DistillEngine.end_eval() (the bulk copy) + metrics.table_from_stats (numpy)
    device: DistillEngine.end_eval_table() (csrc/evaltable.hip, 2064 doubles copied)
A host clock around each call; both end in a device-to-host copy, i.e. synchronised.  The two run alternately, --reps times each after one
warm-up; scores are distinct, so the two tables must agree and the script checks that they do.

    python tools/dev/time_eval_table.py [--rows 65536 1048576] [--classes 1 20] [--reps 5] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from mm_distillnet_amd import metrics as M  # noqa: E402
from mm_distillnet_amd.step import DistillEngine  # noqa: E402

S = 512


def fill(eng, n, n_cls, n_img, seed):
    """a full record of n rows: distinct scores, labels and ground truth over n_cls classes, random 9-bit masks"""
    rng = np.random.default_rng(seed)
    eng.begin_eval(n_img, n, n)
    ev = eng._eval
    rows = np.stack([rng.permutation(n).astype(np.float32) / np.float32(n), rng.integers(0, n_cls, n).astype(np.float32)], axis=1)
    ev.rows.copy_(torch.from_numpy(rows.reshape(-1)))
    ev.tp.copy_(torch.from_numpy(rng.integers(0, 512, n).astype(np.int32)))
    ev.cd.copy_(torch.from_numpy(np.stack([rng.random(n_img) * 300, rng.random(n_img) * 200, rng.integers(1, 9, n_img)], 1)
                                    .astype(np.float32).reshape(-1)))
    ev.gt.copy_(torch.from_numpy(rng.integers(0, n_cls, n).astype(np.float32)))
    ev.cursor.copy_(torch.tensor([n, n_img, n], dtype=torch.int32))
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[65536, 1048576])
    ap.add_argument("--classes", type=int, nargs="+", default=[1, 20])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    # the record and its two ends need nothing of the networks: an engine without them
    eng = DistillEngine.__new__(DistillEngine)
    eng.device, eng._eval, eng.overflow = "cuda:0", None, torch.zeros(1, dtype=torch.int32, device="cuda:0")
    res = []
    for n in a.rows:
        for n_cls in a.classes:
            t = {"host": [], "device": []}
            for rep in range(a.reps + 1):
                fill(eng, n, n_cls, max(1, n // 16), seed=n_cls)
                t0 = time.perf_counter()
                host = M.table_from_stats(eng.end_eval(), S)
                t1 = time.perf_counter()
                fill(eng, n, n_cls, max(1, n // 16), seed=n_cls)
                t2 = time.perf_counter()
                dev = eng.end_eval_table(S)
                t3 = time.perf_counter()
                if rep:          # rep 0 warms both up (code objects, allocator)
                    t["host"].append((t1 - t0) * 1e3); t["device"].append((t3 - t2) * 1e3)
            for k in ("AP@Ave", "AP@0.5", "AP@0.75"):
                assert abs(host[k] - dev[k]) <= 1e-7, (k, host[k], dev[k])
            for k in ("CDx", "CDy"):
                assert abs(host[k] - dev[k]) <= 1e-5 * abs(host[k]), (k, host[k], dev[k])
            row = {"rows": n, "classes": n_cls, "reps": a.reps, "AP@Ave": dev["AP@Ave"],
                   **{f"{k}_ms_{s}": float(f(v)) for k, v in t.items() for s, f in (("median", np.median), ("min", np.min), ("max", np.max))}}
            print(json.dumps(row), flush=True)
            res.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
