"""Helper (not a test): float64 restatements of what csrc/evaltable.hip is held to, written from the contract in include/mmdistill.h and
from mm_distillnet_amd/metrics.py, not from the kernels.

  sort_order(key, cls) ... the permutation of mmd_sort_desc_f32: class ascending, key descending, index ascending; -0.0 = +0.0, +-inf
                           are numbers, NaN keys last within their class in input order.
  table_ref(stats, S) .... metrics.table_from_stats with that stable tie rule in place of np.argsort(-conf), plus the per-class rows
                           (class, n_gt, n_pred, precision, recall, AP, F1) at IoU 0.5 and the nine mean APs.
  records() .............. the evaluation records of tests/test_gpu_eval_table.py, by name.
"""
import numpy as np


def canon(key):
    k = np.array(key, np.float32)
    k[k == 0] = 0.0          # -0.0 -> +0.0
    return k


def sort_order(key, cls=None):
    with np.errstate(invalid="ignore"):          # a signalling NaN key is still a NaN in float64
        k = canon(key).astype(np.float64)
    nan = np.isnan(k)
    keys = [np.arange(k.size), np.where(nan, 0.0, -k), nan]      # last key is the most significant
    if cls is not None:
        keys.append(np.asarray(cls, np.float64))
    return np.lexsort(tuple(keys))


def table_ref(stats, image_size):
    sc, lb = np.asarray(stats["score"], np.float32), np.asarray(stats["label"], np.float32)
    mask, gt = np.asarray(stats["tp"]).astype(np.int64), np.asarray(stats["gt"], np.float64)
    cd = np.asarray(stats["cd"], np.float32).reshape(-1, 3)
    classes, n_obj = np.unique(gt, return_counts=True)
    per = np.zeros((classes.size, 7))
    per[:, 0], per[:, 1] = classes, n_obj
    if sc.size == 0:
        return {"AP@Ave": 0.0, "AP@0.5": 0.0, "AP@0.75": 0.0, "CDx": 10000.0, "CDy": 10000.0, "per_class": per, "mean_ap": np.zeros(9)}
    order = sort_order(sc, lb)
    ap = np.zeros((classes.size, 9))
    for ci, (c, n_c) in enumerate(zip(classes, n_obj)):
        seg = order[lb[order] == c]          # the class's predictions, ranked
        per[ci, 2] = seg.size
        if seg.size == 0:
            continue
        for k in range(9):
            tp = ((mask[seg] >> k) & 1).astype(np.float64)
            hits = np.cumsum(tp)
            p = hits / (np.arange(seg.size) + 1.0)
            r = hits / (n_c + 1e-16)
            env = np.maximum.accumulate(p[::-1])[::-1]
            step = r - np.r_[0.0, r[:-1]]
            ap[ci, k] = np.sum((step * env)[tp > 0])
            if k == 0:
                per[ci, 3], per[ci, 4] = p[-1], r[-1]
    per[:, 5] = ap[:, 0]
    per[:, 6] = 2 * per[:, 3] * per[:, 4] / (per[:, 3] + per[:, 4] + 1e-16)
    mean = ap.mean(axis=0) if classes.size else np.full(9, np.nan)
    has = cd[cd[:, 2] > 0]
    S = np.float32(image_size)
    qx = (has[:, 0] / has[:, 2] / S).astype(np.float64)       # the float32 quotients, averaged in float64
    qy = (has[:, 1] / has[:, 2] / S).astype(np.float64)
    return {"AP@Ave": float(np.mean(mean)) * 100, "AP@0.5": float(mean[0]) * 100, "AP@0.75": float(mean[5]) * 100,
            "CDx": float(np.mean(qx)) * 100 if qx.size else float("nan"), "CDy": float(np.mean(qy)) * 100 if qy.size else float("nan"),
            "per_class": per, "mean_ap": mean}


def _record(rng, n, classes, gt_classes, n_img=7, ties=False, masks="random"):
    """n predictions over `classes`, ground truth over `gt_classes` (class -> count)"""
    score = rng.choice(np.array([0.2, 0.5, 0.5000001, 0.9], np.float32), n) if ties else rng.permutation(n).astype(np.float32) / np.float32(n + 1)
    label = rng.choice(np.asarray(classes, np.float32), n).astype(np.float32)
    tp = {"random": rng.integers(0, 512, n), "all": np.full(n, 511), "none": np.zeros(n)}[masks].astype(np.int32)
    gt = np.concatenate([np.full(m, c, np.float32) for c, m in gt_classes.items()])
    cd = np.stack([rng.random(n_img) * 300, rng.random(n_img) * 200, rng.integers(1, 9, n_img)], axis=1).astype(np.float32)
    return {"score": score, "label": label, "tp": tp, "cd": cd, "gt": rng.permutation(gt)}


def records(tile, seed=5):
    """name -> (record, tie_free)"""
    rng = np.random.default_rng(seed)
    out = {}
    out["empty"] = ({"score": np.zeros(0, np.float32), "label": np.zeros(0, np.float32), "tp": np.zeros(0, np.int32),
                     "cd": np.array([[3, 4, 2], [0, 0, 0]], np.float32), "gt": np.array([6, 6, 2], np.float32)}, True)
    out["one_class_all_tp"] = (_record(rng, 37, [6], {6: 50}, masks="all"), True)
    out["one_class_all_fp"] = (_record(rng, 37, [6], {6: 11}, masks="none"), True)
    out["missing_and_extra_class"] = (_record(rng, 300, [1, 4, 200], {1: 40, 4: 9, 7: 5}), True)      # 7: never predicted; 200: not in the ground truth
    out["random_masks"] = (_record(rng, 1000, [0, 3, 6, 255], {0: 300, 3: 100, 6: 17, 255: 60}), True)
    out["two_classes_across_tiles"] = (_record(rng, 2 * tile + 5, [2, 9], {2: tile, 9: 700}), True)
    r = _record(rng, 200, [5, 6], {5: 30, 6: 80}, n_img=9)
    r["cd"][[0, 4, 8]] = 0          # images without ground truth keep a zero row
    out["images_without_boxes"] = (r, True)
    out["heavy_ties"] = (_record(rng, tile + 300, [0, 1, 2], {0: 500, 1: 20, 2: 300}, ties=True), False)
    return out
