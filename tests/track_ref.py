"""Helper (not a test): numpy float32 restatement of the streaming tracker that csrc/track.hip computes (mmd_track_update).

The reference tree ships no tracker; the rule is this project's own (streaming tracking): a greedy IoU tracker with a
constant-velocity alpha-beta model, alpha = 1.  Every operation below is a float32 operation rounded on its own, in the order the kernel
does them with __fadd_rn / __fsub_rn / __fmul_rn / __fdiv_rn, so track ids AND the final state are compared bit for bit.  min / max are
np.fmin / np.fmax (fminf / fmaxf: the non-NaN operand wins), comparisons are false for NaN.

Per window, in window order (empty windows age the tracks):
  1. predict: every live slot's box moves by its velocity
  2. candidates: (slot, detection) with equal labels and iou >= iou_min; only the first 256 detections of a window take part
  3. greedy: the largest IoU among unmatched slots and detections, ties to the lowest slot, then to the lowest detection
  4. matched slot: v += beta * (centre of the detection - centre of the prediction); box and score become the detection's
  5. unmatched live slot: keeps the prediction, misses += 1, freed (zeroed) once misses > max_age - before the births
  6. unmatched detection with score >= birth_score, in detection order: lowest free slot, id = next_id++; no slot: -1 and overflow
  7. every other row: -1

State layout (what `new_state` of mm_distillnet_amd/tracker.py allocates): slots int32 [max_tracks, 16], words
  0 live  1 id  2..5 x1 y1 x2 y2 (float bits)  6 vx  7 vy  8 label (float bits)  9 score  10 hits  11 misses  12 last_window
  13..15 unused (never read, never written); glob int32 [2] = {next_id, overflow}."""
import numpy as np

WORDS, DET_MAX = 16, 256
F = np.float32


def iou_matrix(tb, db):
    """tb [T, 4], db [n, 4] float32 -> [T, n] float32, as the NMS computes it (areas without +1), 0 where the boxes do not overlap"""
    tx1, ty1, tx2, ty2 = (tb[:, k][:, None] for k in range(4))
    dx1, dy1, dx2, dy2 = (db[:, k][None, :] for k in range(4))
    with np.errstate(all="ignore"):
        ta = (tx2 - tx1) * (ty2 - ty1)
        da = (dx2 - dx1) * (dy2 - dy1)
        ww = np.fmin(tx2, dx2) - np.fmax(tx1, dx1)
        hh = np.fmin(ty2, dy2) - np.fmax(ty1, dy1)
        inter = ww * hh
        u = (ta + da) - inter
        iou = np.where(u > 0, inter / np.where(u > 0, u, F(1)), F(0))
        iou = np.where((ww <= 0) | (hh <= 0), F(0), iou)
    assert iou.dtype == np.float32
    return iou


def track(rows, window, n_windows, cfg, slots=None, glob=None):
    """rows [R, 6] (x1, y1, x2, y2, score, label), window [R] non-decreasing, windows 0 .. n_windows-1
    -> (track int32 [R], slots int32 [max_tracks, 16], glob int32 [2]); slots / glob: the state to go on from (default: reset)"""
    rows = np.asarray(rows, np.float32).reshape(-1, 6)
    window = np.asarray(window, np.int64).reshape(-1)
    assert len(window) == len(rows) and (np.diff(window) >= 0).all()
    M = int(cfg.max_tracks)
    iou_min, beta, birth = F(cfg.iou_min), F(cfg.beta), F(cfg.birth_score)
    slots = np.zeros((M, WORDS), np.int32) if slots is None else np.array(slots, np.int32).reshape(M, WORDS)
    glob = np.zeros(2, np.int32) if glob is None else np.array(glob, np.int32).reshape(2)
    live = slots[:, 0] != 0
    fl = slots.view(np.float32)
    ids = np.where(live, slots[:, 1], 0).astype(np.int32)
    box = np.where(live[:, None], fl[:, 2:6], F(0)).astype(np.float32)
    vel = np.where(live[:, None], fl[:, 6:8], F(0)).astype(np.float32)
    label = np.where(live, fl[:, 8], F(0)).astype(np.float32)
    score = np.where(live, fl[:, 9], F(0)).astype(np.float32)
    hits = np.where(live, slots[:, 10], 0).astype(np.int32)
    misses = np.where(live, slots[:, 11], 0).astype(np.int32)
    last = np.where(live, slots[:, 12], 0).astype(np.int32)
    next_id, over = int(glob[0]), int(glob[1])
    out = np.full(len(rows), -1, np.int32)
    lo_hi = np.searchsorted(window, np.arange(n_windows + 1))

    for w in range(n_windows):
        lo, hi = int(lo_hi[w]), int(lo_hi[w + 1])
        if hi - lo > DET_MAX:
            over = 1
        det = rows[lo:min(hi, lo + DET_MAX)]
        n = len(det)
        # 1. predict
        with np.errstate(all="ignore"):
            box[live, 0] += vel[live, 0]
            box[live, 2] += vel[live, 0]
            box[live, 1] += vel[live, 1]
            box[live, 3] += vel[live, 1]
        T = np.nonzero(live)[0]                                   # rising slot order
        matched = np.zeros(M, bool)
        used = np.zeros(n, bool)
        if len(T) and n:
            iou = iou_matrix(box[T], det[:, :4])
            with np.errstate(invalid="ignore"):
                cand = (label[T][:, None] == det[:, 5][None, :]) & (iou >= iou_min)
            # 2. / 3. greedy: argmax of the row-major matrix returns the first maximum = lowest slot, then lowest detection
            while cand.any():
                k = int(np.argmax(np.where(cand, iou, F(-1))))
                ti, d = divmod(k, n)
                t = int(T[ti])
                # 4. matched slot
                with np.errstate(all="ignore"):
                    rx = (det[d, 0] + det[d, 2]) * F(0.5) - (box[t, 0] + box[t, 2]) * F(0.5)
                    ry = (det[d, 1] + det[d, 3]) * F(0.5) - (box[t, 1] + box[t, 3]) * F(0.5)
                    vel[t, 0] = vel[t, 0] + beta * rx
                    vel[t, 1] = vel[t, 1] + beta * ry
                box[t] = det[d, :4]
                score[t] = det[d, 4]
                hits[t] += 1
                misses[t] = 0
                last[t] = w
                out[lo + d] = ids[t]
                matched[t] = True
                used[d] = True
                cand[ti, :] = False
                cand[:, d] = False
        # 5. unmatched live slots age; freeing comes before the births
        for t in T:
            if not matched[t]:
                misses[t] += 1
                if misses[t] > cfg.max_age:
                    live[t] = False
                    ids[t] = hits[t] = misses[t] = last[t] = 0
                    box[t] = 0
                    vel[t] = 0
                    label[t] = score[t] = 0
        # 6. births
        for d in range(n):
            if used[d] or not (det[d, 4] >= birth):
                continue
            free = np.nonzero(~live)[0]
            if len(free) == 0:
                over = 1
                continue
            t = int(free[0])
            live[t] = True
            ids[t] = next_id
            out[lo + d] = next_id
            next_id += 1
            box[t] = det[d, :4]
            vel[t] = 0
            label[t], score[t] = det[d, 5], det[d, 4]
            hits[t], misses[t], last[t] = 1, 0, w

    new = slots.copy()
    nf = new.view(np.float32)
    new[:, 0], new[:, 1] = live.astype(np.int32), ids
    nf[:, 2:6], nf[:, 6:8], nf[:, 8], nf[:, 9] = box, vel, label, score
    new[:, 10], new[:, 11], new[:, 12] = hits, misses, last
    return out, new, np.array([next_id, over], np.int32)
