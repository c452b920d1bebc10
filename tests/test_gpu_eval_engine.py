"""GPU: DistillEngine.begin_eval / eval_batch / end_eval + metrics.table_from_stats against the host path (predict +
metrics.evaluate_table) on the D2 / 256^2 engine and inputs of the validate golden (test_gpu_model.py): the same table, value for value,
and the same (tp, score, label) rows at every IoU threshold."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mm_distillnet_amd import metrics as M
from mm_distillnet_amd.synth import synth_inputs

DEV = "cuda"


def test_device_record_equals_host_path(golden_dir):
    from mm_distillnet_amd.arch import make_spec
    from mm_distillnet_amd.step import DistillEngine, StepConfig
    from test_oracle_golden import val_states
    g = np.load(os.path.join(golden_dir, "validate_d2_256.npz"))
    S, N, B = int(g["image_size"]), int(g["n"]), int(g["batch"])
    tstates, spec, st_s = val_states()
    eng = DistillEngine(spec, {"rgb": make_spec(2, 3), "depth": make_spec(2, 3), "thermal": make_spec(2, 1)}, DEV, StepConfig(image_size=S))
    eng.load(st_s, tstates)
    data = synth_inputs(N, S, seed=61)
    batches = [{k: v[b * B:(b + 1) * B].to(DEV) for k, v in data.items()} for b in range(N // B)]
    # host path
    all_pred, all_lab = [], []
    for batch in batches:
        p, l = eng.predict(batch)
        all_pred.append(p); all_lab.append(l)
    labels = [float(r[4]) for bl in all_lab for t in bl for r in np.asarray(t, np.float32).reshape(-1, 5)]
    want = M.evaluate_table(all_pred, all_lab, labels, S)
    n_pred, n_gt = sum(len(p) for bp in all_pred for p in bp), len(labels)
    assert n_pred > 0 and n_gt > 0 and want["AP@0.5"] > 0, "the comparison needs detections and pseudo ground truth"
    # device path, record exactly as large as it has to be
    host = M.stats_from_lists(all_pred, all_lab)
    eng.begin_eval(N, max(1, len(host["tp"])), n_gt)
    for batch in batches:
        eng.eval_batch(batch)
    eng.check_overflow()
    stats = eng.end_eval()
    for k in ("tp", "score", "label", "cd", "gt"):
        np.testing.assert_array_equal(stats[k], host[k], err_msg=k)
    for k, iou in enumerate(np.around(np.arange(0.5, 0.95, 0.05), 2)):      # the host path's concatenated rows, threshold by threshold
        sm = [m for bp, bl in zip(all_pred, all_lab) for m in M.get_batch_statistics(bp, bl, iou)]
        tp, sc, lb = [np.concatenate(x, 0) for x in zip(*sm)]
        np.testing.assert_array_equal(((stats["tp"] >> k) & 1).astype(np.float64), tp)
        np.testing.assert_array_equal(stats["score"], sc); np.testing.assert_array_equal(stats["label"], lb)
    got = M.table_from_stats(stats, S)
    assert got.keys() == want.keys()
    for k in want:
        assert got[k] == want[k], (k, got[k], want[k])
    # a record one row too small raises, and an evaluation cannot end twice
    eng.begin_eval(N, max(1, len(host["tp"]) - 1), n_gt)
    for batch in batches:
        eng.eval_batch(batch)
    with pytest.raises(RuntimeError, match="evaluation record capacity exceeded"):
        eng.check_overflow()
    with pytest.raises(RuntimeError, match="evaluation record capacity exceeded"):
        eng.end_eval()
    with pytest.raises(RuntimeError, match="without begin_eval"):
        eng.end_eval()
