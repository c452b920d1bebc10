#!/usr/bin/env python3
"""Evaluation entry point with the reference's CLI (evaluate.py:51-170 upstream):

    python evaluate.py --config_file F --checkpoint P [--overwrite JSON] [--ema]

--ema: the checkpoint's averaged weights (`state_dict_ema`, written by a run with cfg ema_decay) instead of its raw ones (`state_dict`).

The student's detections (score > conf_threshold, class filter, NMS — the same device kernels that make the
teachers' pseudo-labels) are scored against the merged multi-teacher pseudo ground truth with the reference's
AP@0.5 / AP@0.75 / AP@Ave / CDx / CDy definitions (mm_distillnet_amd/metrics.py, pinned by the reference's evaluate() through
tests/golden/metrics_eval.npz) and written to <exp>/results.<rank>.csv with the reference's columns.
"""
import argparse
import os
import sys

import numpy as np

# Hardware queues (opt-in): the step's graph has six concurrent branches (main chain, three teachers, weight gradients,
# regressor head); the HIP runtime multiplexes a process' streams onto GPU_MAX_HW_QUEUES hardware queues (default 4).
# MMD_HW_QUEUES=8 measured 21.35 ms/step (mean of 12 runs) against 21.73 with the default; left off by default because the
# runtime proved fragile away from its default (2 queues: 40.7 ms/step or a segfault inside graph replay) - profiles/r01_notes.md.
# Must be in the environment before the HIP runtime initialises, i.e. before torch is imported.
if os.environ.get("MMD_HW_QUEUES"):
    os.environ.setdefault("GPU_MAX_HW_QUEUES", os.environ["MMD_HW_QUEUES"])
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import train as T  # noqa: E402
from mm_distillnet_amd.data import SyntheticMultimodalDetection, collate  # noqa: E402
from mm_distillnet_amd.metrics import evaluate_table, table_from_stats  # noqa: E402
from mm_distillnet_amd.step import DistillEngine  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config_file", required=True)
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--overwrite", type=str, default=None)
    ap.add_argument("--just_plot", action="store_true")
    ap.add_argument("--ema", action="store_true", help="evaluate the checkpoint's averaged weights (state_dict_ema: cfg ema_decay)")
    a = ap.parse_args(argv)
    cfg, _ = T.parse_config(["--config_file", a.config_file] + (["--overwrite", a.overwrite] if a.overwrite else []))
    ckpt_state = None
    if a.ema:
        # refused on the host, before the device is touched: no checkpoint, or one without averaged weights
        if not a.checkpoint:
            raise ValueError("--ema reads the averaged weights of a checkpoint: it needs --checkpoint")
        ckpt_state = T.TR.checkpoint_student_state(torch.load(a.checkpoint, map_location="cpu", weights_only=False), True, a.checkpoint)
    torch.cuda.set_device(0)
    dev = "cuda:0"
    sspec, sstate, tspecs, tstates = T.load_states(cfg, int(cfg.get("compound_coef", 2)))
    if ckpt_state is not None:
        sstate = ckpt_state
    elif a.checkpoint:
        c = torch.load(a.checkpoint, map_location="cpu", weights_only=False)
        sstate = c["state_dict"] if "state_dict" in c else c
    eng = DistillEngine(sspec, tspecs, dev, T.step_config(cfg))
    eng.load(sstate, tstates)
    test_set = SyntheticMultimodalDetection(cfg, "test")
    loader = torch.utils.data.DataLoader(test_set, batch_size=cfg.getint("batch_size"), shuffle=False, collate_fn=collate)
    # evaluate() (src/utils/utils.py:2018-2181): one row per testing point; 'ALL' when the three teachers are in use
    mods = [m for m in ("rgb", "depth", "thermal") if cfg.getboolean(f"use_{m}", True)]
    modality = "ALL" if len(mods) == 3 else ",".join(mods)
    mode = cfg.get("eval_metrics", "host")      # host until the device path is timed against it: profiles/eval_metrics_notes.md
    if mode not in ("device", "device_table", "host"):
        raise Exception(f"Unsupported eval_metrics {mode} (device | device_table | host)")
    per_class = None
    if mode in ("device", "device_table"):
        # the matching and the central distances run on the device behind every batch (csrc/evalstats.hip): no per-batch synchronize,
        # the record is copied once, at the end.  Record capacity: cfg eval_record_rows (predictions of images with ground truth, and
        # ground-truth boxes, over the whole test set); exceeded -> end_eval raises, nothing is truncated silently
        rows = cfg.getint("eval_record_rows", 0) or max(1 << 16, 256 * len(test_set))
        eng.begin_eval(len(test_set), rows)
        for i, (rgb, thermal, depth, audio, _, ids) in enumerate(loader):
            eng.eval_batch({"rgb": rgb.to(dev), "thermal": thermal.to(dev), "depth": depth.to(dev), "audio": audio.to(dev)})
            if i % 64 == 63:
                eng.check_overflow()      # a record that is too small ends the run here, not after the last batch
        if mode == "device_table":
            # the table too is computed on the device, on the record where it lies (csrc/evaltable.hip): what comes back is the row below
            # and the per-class table upstream logs at IoU 0.5 (src/utils/utils.py:1393-1401); equal scores rank in record order
            table = eng.end_eval_table(cfg.getint("image_size"))
            per_class = table.pop("per_class")
        else:
            table = table_from_stats(eng.end_eval(), cfg.getint("image_size"))
    else:
        # get_predictions_multiteacher (src/utils/utils.py:1720-1830): per batch the student's detections and the merged teacher
        # pseudo ground truth, plus the flat list of ground-truth class ids
        all_pred, all_lab, labels = [], [], []
        for rgb, thermal, depth, audio, _, ids in loader:
            batch = {"rgb": rgb.to(dev), "thermal": thermal.to(dev), "depth": depth.to(dev), "audio": audio.to(dev)}
            p, l = eng.predict(batch)
            all_pred.append(p); all_lab.append(l)
            labels += [float(r[4]) for t in l for r in np.asarray(t, np.float32).reshape(-1, 5)]
        eng.check_overflow()
        table = evaluate_table(all_pred, all_lab, labels, cfg.getint("image_size"))
    print({k: round(v, 3) for k, v in table.items()})
    if per_class is not None:
        print("%8s %10s %10s %10s %10s" % ("class", "precision", "recal", "AP", "F1"))
        for c, _, _, p, r, ap, f1 in per_class:
            print("%8d %10.4f %10.4f %10.4f %10.4f" % (int(c), p, r, ap, f1))
    if os.path.exists(cfg["exp_name"]):
        import pandas as pd
        pd.DataFrame([dict(exp_name=cfg["exp_name"], modality=modality, **table)]).to_csv(
            f"{cfg['exp_name']}/results.{cfg['rank']}.csv", index=False)
    return table


if __name__ == "__main__":
    main()
