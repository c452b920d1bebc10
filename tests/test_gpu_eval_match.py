"""GPU: mmd_eval_match (csrc/evalstats.hip) against the host metrics (mm_distillnet_amd/metrics.py, itself pinned to the reference by
tests/golden/metrics_eval.npz), bit for bit: the 9-bit true-positive masks at all nine IoU thresholds, scores, classes, the central
distance sums, the ground-truth class list, the cursor and the overflow flag.

Every call runs under the two rules of tests/test_gpu_pseudo_labels.py (guarded tails behind every buffer; once on zeroed buffers and
once on dirty ones - here the record and the workspace are filled with 0xFF bytes and the input rows behind the counts with NaN - with
bit-identical results), and the part of the record behind the cursor must still hold its 0xFF bytes afterwards."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mm_distillnet_amd import _lib
from mm_distillnet_amd import metrics as M
from test_gpu_pseudo_labels import Harness, both, eq, i32, r5, r6

call = _lib.call


def lds_cap(which):
    return int(_lib.LIB.load().mmd_eval_lds_cap(which))


def ws_floats(cap, G):
    return int(_lib.LIB.load().mmd_eval_ws_floats(cap, G))


def run_match(h, batches, cap, G, max_rows, max_images, max_gt):
    """batches: [(predictions per image, boxes per image)] -> the record after one mmd_eval_match call per batch"""
    rec_rows = h.buf((max_rows, 2)); rec_tp = h.buf((max_rows,), torch.int32)
    rec_cd = h.buf((max_images, 3)); rec_gt = h.buf((max_gt,))
    record = [rec_rows, rec_tp, rec_cd, rec_gt]
    if h.dirty:
        for t in record:
            t.view(torch.int32).fill_(-1)
    cursor = h.buf((3,), torch.int32); cursor.zero_()      # the caller zeroes the cursor and the sticky flag
    ovf = h.flag()
    n = ws_floats(cap, G)
    assert n >= 0
    for preds, boxes in batches:
        B = len(preds)
        ws = None
        if n:
            ws = h.buf((B * n,))
            if h.dirty:
                ws.view(torch.int32).fill_(-1)
        call("mmd_eval_match", h.rows(preds, cap, 6), i32(len(p) for p in preds), cap, h.rows(boxes, G, 5), i32(len(b) for b in boxes),
             G, B, rec_rows, rec_tp, max_rows, rec_cd, max_images, rec_gt, max_gt, cursor, ws, ovf)
    torch.cuda.synchronize()
    cur = cursor.cpu().numpy()
    assert 0 <= cur[0] <= max_rows and 0 <= cur[1] <= max_images and 0 <= cur[2] <= max_gt
    if h.dirty:           # behind the cursor nothing was touched
        for t, c in zip(record, (cur[0], cur[0], cur[1], cur[2])):
            assert bool((t[int(c):].contiguous().view(torch.int32) == -1).all())
    nr, ni, ng = (int(c) for c in cur)
    return {"score": rec_rows[:nr, 0].cpu().numpy(), "label": rec_rows[:nr, 1].cpu().numpy(), "tp": rec_tp[:nr].cpu().numpy(),
            "cd": rec_cd[:ni].cpu().numpy(), "gt": rec_gt[:ng].cpu().numpy(), "cursor": cur, "overflow": int(ovf.item())}


def host_stats(batches):
    return M.stats_from_lists([b[0] for b in batches], [b[1] for b in batches])


def check(batches, cap=None, G=None, slack=3):
    """device record == host record for `batches`, all nine thresholds; -> the host record"""
    want = host_stats(batches)
    cap = cap or max(1, max(len(p) for b in batches for p in b[0]))
    G = G or max(1, max(len(x) for b in batches for x in b[1]))
    n_img = sum(len(b[0]) for b in batches)
    got = both(run_match, batches, cap, G, len(want["tp"]) + slack, n_img + slack, len(want["gt"]) + slack)
    assert got["overflow"] == 0
    for k in ("score", "label", "tp", "cd", "gt"):
        eq(got[k], want[k], k)
    assert list(got["cursor"]) == [len(want["tp"]), n_img, len(want["gt"])]
    return want


# ---------------------------------------------------------------------------------------------------------------------
def _ragged(rows, counts, cols):
    out, o = [], 0
    for c in counts:
        out.append(rows[o:o + c].reshape(-1, cols)); o += c
    return out


def test_reference_golden_in_batches_of_four(golden_dir):
    g = np.load(os.path.join(golden_dir, "metrics_eval.npz"))
    S = int(g["image_size"])
    preds, labs = _ragged(g["pred_rows"], g["pred_counts"], 6), _ragged(g["lab_rows"], g["lab_counts"], 5)
    batches = [(preds[i:i + 4], labs[i:i + 4]) for i in range(0, 20, 4)]
    got = both(run_match, batches, 8, 6, 64, 24, 48)
    assert got["overflow"] == 0 and list(got["cursor"]) == [43, 20, 40]
    for iou, k in ((0.5, 0), (0.75, 5), (0.9, 8)):
        np.testing.assert_array_equal(((got["tp"] >> k) & 1).astype(np.float64), g[f"tp@{iou}"])
        np.testing.assert_array_equal(got["score"], g[f"score@{iou}"])
        np.testing.assert_array_equal(got["label"], g[f"label@{iou}"])
    cd = got["cd"][got["cd"][:, 2] > 0]
    np.testing.assert_array_equal((cd[:, 0] / cd[:, 2] / S).astype(np.float64), g["cd_x"])
    np.testing.assert_array_equal((cd[:, 1] / cd[:, 2] / S).astype(np.float64), g["cd_y"])
    labels = [float(r[4]) for l in labs for r in l]
    np.testing.assert_array_equal(got["gt"], np.asarray(labels, np.float32))
    want = M.evaluate_table([b[0] for b in batches], [b[1] for b in batches], labels, S)
    table = M.table_from_stats(got, S)
    for k in want:
        assert table[k] == want[k], (k, table[k], want[k])
    assert any(r[2] < r[0] for pr in preds for r in pr)      # the golden's degenerate row (x2 < x1) took part


PAIRS = [(1, 2), (11, 20), (3, 5), (13, 20), (7, 10), (3, 4), (4, 5), (17, 20), (9, 10)]      # inter / union = threshold k


def test_iou_exactly_on_and_one_pixel_short_of_every_threshold():
    """Nested boxes with the +1 convention: prediction [0, I-1] x [0, fy-1] inside box [0, U-1] x [0, fy-1] -> inter = I fy, union = U fy.
    One image per (threshold, scale, exact | one pixel short); every image also holds a second prediction that must not steal the box."""
    images, expect = [], []
    for k, (i, u) in enumerate(PAIRS):
        for fx, fy in ((2, 1), (5, 3), (16, 7)):
            I, U = i * fx, u * fx
            for short in (0, 1):
                box = r5([[0, 0, U - 1, fy - 1, 6]])
                pred = r6([[0, 0, I - 1 - short, fy - 1, 0.5, 6], [0, 0, I - 1 - short, fy - 1, 0.9, 6]])
                images.append((pred, box)); expect.append((k, short))
    want = check([([p for p, _ in images], [b for _, b in images])])
    for j, (k, short) in enumerate(expect):      # the premise: the first prediction of image j sits on / just under threshold k
        m = int(want["tp"][2 * j])
        assert (m >> k) & 1 == 1 - short and m & (m + 1) == 0 and (short or m == (1 << (k + 1)) - 1), (j, k, short, m)
        assert int(want["tp"][2 * j + 1]) == 0      # the box is taken


def _random_image(rng, n, g, classes=(1, 6, 14), size=256):
    """g integer boxes; predictions: jittered copies of boxes (so that IoUs spread over 0.3 .. 1), exact copies, strangers; shuffled"""
    x1 = rng.integers(0, size - 40, g); y1 = rng.integers(0, size - 40, g)
    w = rng.integers(4, 40, g); hgt = rng.integers(4, 40, g)
    boxes = np.stack([x1, y1, x1 + w, y1 + hgt, rng.choice(classes, g)], 1).astype(np.float32)
    rows = []
    for _ in range(n):
        kind = rng.integers(0, 10)
        if g and kind < 7:
            b = boxes[rng.integers(0, g)]
            j = rng.integers(-3, 4, 4) if kind < 6 else np.zeros(4)
            rows.append([b[0] + j[0], b[1] + j[1], b[2] + j[2], b[3] + j[3], 0, b[4] if kind else rng.choice(classes)])
        else:
            x, y = rng.integers(0, size - 40, 2)
            rows.append([x, y, x + rng.integers(4, 40), y + rng.integers(4, 40), 0, rng.choice(classes)])
    rows = np.asarray(rows, np.float32).reshape(-1, 6)
    rows[:, 4] = rng.permutation(n).astype(np.float32) / max(n, 1)      # distinct scores, NOT sorted
    return rows, boxes


def test_constructed_images_one_batch_of_five_and_batches_of_one():
    b1, b2 = [10, 10, 29, 29, 6], [100, 100, 139, 119, 6]
    images = [
        # duplicate boxes and duplicate predictions: the first index wins
        (r6([[10, 10, 29, 29, .9, 6], [10, 10, 29, 29, .9, 6], [10, 10, 29, 29, .8, 6], [11, 10, 29, 29, .7, 6]]), r5([b1, b1, b2, b1])),
        # a class no box has, unsorted scores, more predictions than boxes: the boxes run out at different points per threshold
        # (IoU 0.7 then 1.0 on the second box, 0.8 then 1.0 then 0.95 on the first: the exact copies are true positives only above those)
        (r6([[10, 10, 29, 29, .2, 3], [100, 100, 139, 113, .3, 6], [14, 10, 29, 29, .9, 6], [10, 10, 29, 29, .1, 6],
             [100, 100, 139, 119, .5, 6], [100, 101, 139, 119, .4, 6], [10, 11, 29, 29, .6, 6]]), r5([b1, b2])),
        # a degenerate box (x2 < x1) and a degenerate prediction
        (r6([[50, 10, 40, 30, .9, 6], [48, 10, 60, 30, .8, 6], [10, 10, 29, 29, .7, 1]]), r5([[50, 10, 40, 30, 6], b1, [5, 5, 4, 4, 1]])),
        (np.zeros((0, 6), np.float32), r5([b1, [0, 0, 9, 4, 0], [30, 30, 20, 35, 0]])),      # no predictions: compared against zeros
        (r6([[10, 10, 29, 29, .9, 6]]), np.zeros((0, 5), np.float32)),                       # no boxes
    ]
    neither = (np.zeros((0, 6), np.float32), np.zeros((0, 5), np.float32))
    want = check([([p for p, _ in images], [b for _, b in images])])                         # B = 5
    assert [int(m) for m in want["tp"][4:11]] == [0, 0x1f, 0x7f, 0x180, 0x1e0, 0, 0]
    check([([p], [b]) for p, b in images + [neither]])                                       # B = 1, appended call after call
    check([([neither[0], images[0][0], neither[0]], [neither[1], images[0][1], neither[1]])])


@pytest.mark.parametrize("counts", [[(63, 63), (64, 64), (65, 65)], [(130, 70), (7, 65), (65, 3)]])
def test_counts_across_one_wavefront(counts):
    rng = np.random.default_rng(sum(n * 131 + g for n, g in counts))
    images = [_random_image(rng, n, g) for n, g in counts]
    want = check([([p for p, _ in images], [b for _, b in images])])
    assert 0 < int((want["tp"] & 1).sum()) < len(want["tp"]) and len({int(m) for m in want["tp"]}) > 3


def test_lds_bound_and_workspace_path():
    """counts at the LDS bound stay in LDS, one above (predictions, boxes, both) runs through the workspace: same results"""
    NP, NG = lds_cap(0), lds_cap(1)
    assert ws_floats(NP, NG) == 0 and ws_floats(NP + 1, NG) >= 6 * (NP + 1) + 9 * ((NG + 31) // 32) and ws_floats(NP, NG + 1) > 0
    rng = np.random.default_rng(5)
    images = [_random_image(rng, n, g) for n, g in ((NP, NG), (NP + 1, 9), (9, NG + 1), (NP + 1, NG + 1), (3, 2))]
    want = check([([p for p, _ in images], [b for _, b in images])], cap=NP + 1, G=NG + 1)
    assert int((want["tp"] & 1).sum()) > NG


def test_two_calls_append_and_a_record_one_row_too_small():
    rng = np.random.default_rng(11)
    a = [_random_image(rng, n, g) for n, g in ((5, 4), (0, 3), (9, 6))]
    b = [_random_image(rng, n, g) for n, g in ((4, 0), (8, 8))]
    batches = [([p for p, _ in a], [x for _, x in a]), ([p for p, _ in b], [x for _, x in b])]
    want = check(batches, cap=12, G=9, slack=0)            # exactly full: no overflow
    nr, ng = len(want["tp"]), len(want["gt"])
    assert nr == 5 + 9 + 8 and ng == 4 + 3 + 6 + 8
    # one row too small: flagged, the rows in front of the missing one intact, the cursor at the capacity
    got = both(run_match, batches, 12, 9, nr - 1, 5, ng)
    assert got["overflow"] == 1 and list(got["cursor"]) == [nr - 1, 5, ng]
    for k in ("score", "label", "tp"):
        eq(got[k], want[k][:nr - 1], k)
    eq(got["cd"], want["cd"]); eq(got["gt"], want["gt"])
    # too small for the FIRST call's rows: the second call appends nothing, the first rows stay
    got = both(run_match, batches, 12, 9, 7, 5, ng)
    assert got["overflow"] == 1 and got["cursor"][0] == 7
    for k in ("score", "label", "tp"):
        eq(got[k], want[k][:7], k)
    # one class and one image too few
    got = both(run_match, batches, 12, 9, nr, 4, ng - 1)
    assert got["overflow"] == 1 and list(got["cursor"]) == [nr, 4, ng - 1]
    eq(got["gt"], want["gt"][:ng - 1]); eq(got["cd"], want["cd"][:4]); eq(got["tp"], want["tp"])


def test_bad_arguments():
    dll = _lib.LIB.load()
    t = torch.zeros(64, device="cuda"); ti = torch.zeros(64, dtype=torch.int32, device="cuda")
    p, pi = t.data_ptr(), ti.data_ptr()
    ok = [p, pi, 4, p, pi, 2, 1, p, pi, 4, p, 2, p, 4, pi, None, pi, None]
    assert dll.mmd_eval_match(*ok) == 0
    for i in (0, 1, 3, 4, 7, 8, 10, 12, 14, 16):
        bad = list(ok); bad[i] = None
        assert dll.mmd_eval_match(*bad) == -22, i
    for i in (2, 5, 6, 9, 11, 13):
        bad = list(ok); bad[i] = 0
        assert dll.mmd_eval_match(*bad) == -22, i
    big = list(ok); big[2] = lds_cap(0) + 1      # needs a workspace, none given
    assert dll.mmd_eval_match(*big) == -22
    assert ws_floats(0, 1) == -22 and ws_floats(1, 0) == -22
    torch.cuda.synchronize()
