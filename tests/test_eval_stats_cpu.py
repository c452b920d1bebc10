"""CPU: metrics.table_from_stats builds evaluate_table's dict from an evaluation record (what DistillEngine.end_eval returns), value
for value.  The record is built on the host by metrics.get_batch_statistics / get_batch_central_distances (metrics.stats_from_lists)
over the reference-made detections of tests/golden/metrics_eval.npz: 20 images, 49 predictions, 40 boxes."""
import os

import numpy as np

from mm_distillnet_amd import metrics as M


def _ragged(rows, counts, cols):
    out, o = [], 0
    for c in counts:
        out.append(rows[o:o + c].reshape(-1, cols)); o += c
    return out


def golden_lists(golden_dir, bs=4):
    g = np.load(os.path.join(golden_dir, "metrics_eval.npz"))
    preds = _ragged(g["pred_rows"], g["pred_counts"], 6)
    labs = _ragged(g["lab_rows"], g["lab_counts"], 5)
    all_pred = [preds[i:i + bs] for i in range(0, len(preds), bs)]
    all_lab = [labs[i:i + bs] for i in range(0, len(labs), bs)]
    labels = [float(r[4]) for l in labs for r in l]
    return g, all_pred, all_lab, labels, int(g["image_size"])


def test_table_from_stats_equals_evaluate_table(golden_dir):
    g, all_pred, all_lab, labels, S = golden_lists(golden_dir)
    stats = M.stats_from_lists(all_pred, all_lab)
    # the record itself: the reference's own per-threshold outputs
    for iou, k in ((0.5, 0), (0.75, 5), (0.9, 8)):
        np.testing.assert_array_equal(((stats["tp"] >> k) & 1).astype(np.float64), g[f"tp@{iou}"])
        np.testing.assert_array_equal(stats["score"], g[f"score@{iou}"])
        np.testing.assert_array_equal(stats["label"], g[f"label@{iou}"])
    cd = stats["cd"][stats["cd"][:, 2] > 0]
    np.testing.assert_array_equal((cd[:, 0] / cd[:, 2] / S).astype(np.float64), g["cd_x"])
    np.testing.assert_array_equal((cd[:, 1] / cd[:, 2] / S).astype(np.float64), g["cd_y"])
    np.testing.assert_array_equal(stats["gt"], np.asarray(labels, np.float32))
    assert stats["cd"].shape == (20, 3) and stats["tp"].dtype == np.int32
    want = M.evaluate_table(all_pred, all_lab, labels, S)
    got = M.table_from_stats(stats, S)
    assert got.keys() == want.keys()
    for k in want:
        assert got[k] == want[k], (k, got[k], want[k])
    assert got["AP@0.5"] > 0 and 0 < got["CDx"] < 10000


def test_table_from_stats_batching_does_not_matter(golden_dir):
    _, all_pred, all_lab, labels, S = golden_lists(golden_dir, bs=4)
    _, one_pred, one_lab, _, _ = golden_lists(golden_dir, bs=20)
    a, b = M.stats_from_lists(all_pred, all_lab), M.stats_from_lists(one_pred, one_lab)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])


def test_table_from_stats_sentinel_row(golden_dir):
    """no image with both predictions and ground truth: AP 0 and CDx = CDy = 100 * 100, as evaluate_table"""
    _, _, all_lab, _, S = golden_lists(golden_dir)
    lab = [l for bl in all_lab for l in bl if len(l)][0]
    cases = [([[np.zeros((0, 6), np.float32)]], [[lab]]),                                      # ground truth, nothing predicted
             ([[np.zeros((0, 6), np.float32), np.array([[1, 2, 30, 40, 0.9, 6]], np.float32)]],
              [[lab, np.zeros((0, 5), np.float32)]])]                                          # predictions only where there is no ground truth
    for preds, labs in cases:
        labels = [float(r[4]) for bl in labs for t in bl for r in t]
        want = M.evaluate_table(preds, labs, labels, S)
        got = M.table_from_stats(M.stats_from_lists(preds, labs), S)
        assert got == want
        assert got["AP@0.5"] == 0.0 and got["AP@Ave"] == 0.0 and got["CDx"] == 10000.0 and got["CDy"] == 10000.0
