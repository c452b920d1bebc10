"""Helper (not a test): numpy / scipy restatement of the tracker's OPTIMAL association rule (TrackConfig(assign="optimal"),
mmd_track_update_assign with assign = 1; DESIGN.md, tracking evaluation: the tracker's optimal rule).

`track` has the interface and the state layout of tests/track_ref.track and differs from it only in steps 2 - 3:
  2. T = the live slots in rising order after the predict step, D = the first 256 detections; iou = track_ref.iou_matrix (float32); a
     pair is allowed when the labels are equal and iou >= float32(iou_min) (false for NaN); W = float64(iou) on allowed pairs, 0 elsewhere
  3. scipy.optimize.linear_sum_assignment(W, maximize=True) on the FULL matrix; the pairs that are not allowed are dropped; every pair
     left is a match (step 4: all matched slots update from their own prediction, so the order does not matter)
Steps 1 and 4 - 7 are track_ref.track's, operation for operation.

It also returns the smallest MARGIN over the call's windows.  The margin of a window is the optimum weight minus the best weight that
can be reached with any single chosen pair forbidden (its weight set to 0, i.e. the pair dropped; re-solved per pair); +inf for a window
without a pair.  Any other matching lacks at least one chosen pair or is a strict subset of the optimum - and a strict subset is among
the matchings a re-solve may take - so the margin bounds the runner-up: a solver whose float64 sums err by less than the margin must
find the same pairs.  (Forbidding a pair changes nothing outside the connected component of the allowed-pair graph it lies in, so the
re-solve runs on that component alone; the difference of the two optima is the same.)"""
import numpy as np
from scipy.optimize import linear_sum_assignment
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components

from track_ref import DET_MAX, WORDS, F, iou_matrix


def box(x, y=0, size=20, score=0.9, label=6):
    return (x, y, x + size, y + size, score, label)


# Scenes of two windows, shared by the CPU and the GPU tests.
# DIFFERS: A at x = 0 and B at x = 15, then two boxes: IoU(A, first) = 17 / 23, the largest of the window; IoU(A, second) = 15 / 25;
# IoU(B, first) = 8 / 32; B only touches the second box.  Greedy pairs (A, first) and leaves B without an allowed box; the optimum is
# (A, second) + (B, first): 0.85 against 0.739.  iou_min = 0.2 lets the pair of 0.25 in.
DIFFERS = ([box(0), box(15)], [box(3), box(-5)])
DIFFERS_KW = dict(iou_min=0.2)
# WEIGHT: A at x = 0 and B at x = 10.25, then two boxes: IoU(A, first) = 19 / 21; IoU(A, second) = 10.5 / 29.5 and IoU(B, first) =
# 10.75 / 29.25, both allowed at iou_min = 0.3; B only touches the second box.  One pair (0.905) beats the two (0.723) that a
# maximum-cardinality matching takes.
WEIGHT = ([box(0), box(10.25)], [box(1), box(-9.5)])
# A fast vehicle (about 9 px per window) overtakes a slow one in its lane, the boxes jitter by a few pixels; the rows swap places
# every other window.  Ground-truth ids: 0 the fast, 1 the slow vehicle.
CROSS_FAST = [13, 20, 30, 35, 50, 56, 65, 76, 80, 93]
CROSS_SLOW = [61, 59, 60, 55, 58, 58, 53, 51, 53, 49]


def crossing():
    """-> (windows, ground-truth id per row)"""
    windows, gt = [], []
    for w, (xa, xb) in enumerate(zip(CROSS_FAST, CROSS_SLOW)):
        windows.append([box(xa, 40), box(xb, 40)][::-1 if w % 2 else 1])
        gt += [1, 0] if w % 2 else [0, 1]
    return windows, np.asarray(gt, np.int32)


def weights(tb, tlabel, det, iou_min):
    """tb [T, 4] predicted boxes, tlabel [T], det [n, 6] -> (W float64 [T, n], allowed bool [T, n])"""
    iou = iou_matrix(np.asarray(tb, np.float32).reshape(-1, 4), det[:, :4])
    with np.errstate(invalid="ignore"):
        allowed = (np.asarray(tlabel, np.float32)[:, None] == det[:, 5][None, :]) & (iou >= F(iou_min))
    return np.where(allowed, iou.astype(np.float64), 0.0), allowed


def solve(W, allowed):
    """-> (pairs [(t, d)] of the maximum-weight matching, the not allowed ones dropped; its weight)"""
    if W.size == 0 or not allowed.any():
        return [], 0.0
    r, c = linear_sum_assignment(W, maximize=True)
    pairs = [(int(i), int(j)) for i, j in zip(r, c) if allowed[i, j]]
    return pairs, float(sum(W[i, j] for i, j in pairs))


def margin(W, allowed, pairs):
    """the loss of the best matching that lacks one of `pairs` (the optimum of W); inf without a pair"""
    if not pairs:
        return np.inf
    T, n = W.shape
    graph = csr_matrix((np.ones(int(allowed.sum())), (np.nonzero(allowed)[0], T + np.nonzero(allowed)[1])), shape=(T + n, T + n))
    comp = connected_components(graph, directed=False)[1]
    best = np.inf
    for t, d in pairs:
        ts, ds = np.nonzero(comp[:T] == comp[t])[0], np.nonzero(comp[T:] == comp[t])[0]
        sub, ok = W[np.ix_(ts, ds)].copy(), allowed[np.ix_(ts, ds)].copy()
        full = solve(sub, ok)[1]
        i, j = int(np.searchsorted(ts, t)), int(np.searchsorted(ds, d))
        sub[i, j], ok[i, j] = 0.0, False
        best = min(best, full - solve(sub, ok)[1])
    return best


def track(rows, window, n_windows, cfg, slots=None, glob=None):
    """as track_ref.track -> (track int32 [R], slots int32 [max_tracks, 16], glob int32 [2], margin: the smallest over the windows)"""
    rows = np.asarray(rows, np.float32).reshape(-1, 6)
    window = np.asarray(window, np.int64).reshape(-1)
    assert len(window) == len(rows) and (np.diff(window) >= 0).all()
    M = int(cfg.max_tracks)
    beta, birth = F(cfg.beta), F(cfg.birth_score)
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
    smallest = np.inf

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
            # 2. / 3. the matching of maximum weight on the full matrix
            W, allowed = weights(box[T], label[T], det, cfg.iou_min)
            pairs, _ = solve(W, allowed)
            smallest = min(smallest, margin(W, allowed, pairs))
            pred = box.copy()                                     # every matched slot updates from its own prediction
            for ti, d in pairs:
                t = int(T[ti])
                # 4. matched slot
                with np.errstate(all="ignore"):
                    rx = (det[d, 0] + det[d, 2]) * F(0.5) - (pred[t, 0] + pred[t, 2]) * F(0.5)
                    ry = (det[d, 1] + det[d, 3]) * F(0.5) - (pred[t, 1] + pred[t, 3]) * F(0.5)
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
    return out, new, np.array([next_id, over], np.int32), float(smallest)
