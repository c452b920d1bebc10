"""Helper (not a test): the hand-built and the random inputs of the tracking-evaluation tests (test_mot_ref_cpu.py, test_gpu_mot.py).

Hand cases: boxes are 10 x 10 on one line unless said otherwise, so two boxes shifted by d have IoU (10 - d) / (10 + d):
d = 1: 9/11 = .818, 2: 8/12 = .667, 3: 7/13 = .538, 4: 6/14 = .429, 6: 4/16 = .25, 9: 1/19 = .053."""
import numpy as np


def box(x, y=0.0, w=10.0, h=10.0, label=6.0, score=0.9):
    return [x, y, x + w, y + h, score, label]


def rec(items):
    """items: [(window, track, box)] -> (rows, window, track)"""
    rows = np.array([b for _, _, b in items], np.float32).reshape(-1, 6)
    return rows, np.array([w for w, _, _ in items], np.int64), np.array([t for _, t, _ in items], np.int64)


def hand_cases():
    """name -> (gt, hyp, n_windows, iou_min, expected counts worked out by hand)"""
    c = {}
    # greedy takes (G0, H0) = .667 first and then finds nothing allowed for G1; the optimum is (G0, H1) + (G1, H0) = .429 + .538
    c["greedy_not_optimum"] = (rec([(0, 0, box(0)), (0, 1, box(5)), (0, 2, box(100))]),
                               rec([(0, 0, box(2)), (0, 1, box(-4)), (0, 2, box(101))]), 1, 0.3,
                               dict(n_gt=3, n_hyp=3, tp=3, fp=0, fn=0, idsw=0, frag=0, mt=3, pt=0, ml=0, idtp=3, idfp=0, idfn=0))
    # hypothesis track 5 follows the vehicle for two windows, then track 7 takes over
    c["id_switch"] = (rec([(w, 0, box(w)) for w in range(3)]), rec([(0, 5, box(0)), (1, 5, box(1)), (2, 7, box(2))]), 3, 0.5,
                      dict(n_gt=3, n_hyp=3, tp=3, fp=0, fn=0, idsw=1, frag=0, mt=1, pt=0, ml=0, idtp=2, idfp=1, idfn=1))
    # the hypothesis misses window 1 and comes back with the same id: one fragmentation, no switch
    c["fragmentation"] = (rec([(w, 3, box(w)) for w in range(4)]), rec([(w, 9, box(w)) for w in (0, 2, 3)]), 4, 0.5,
                          dict(n_gt=4, n_hyp=3, tp=3, fp=0, fn=1, idsw=0, frag=1, mt=0, pt=1, ml=0, idtp=3, idfp=0, idfn=1))
    # windows 0 and 1 leave map[a] = map[b] = hypothesis track 1.  Window 2 lists b in front of a: b keeps track 1 (.818) although the
    # free optimum would be (a, track 1) + (b, track 2) = .667 + .538; a is left with track 2 at .25 < iou_min: a miss and a false positive.
    # Identity: C = [[2, 0], [2, 1]] over (a, b) x (track 1, track 2), whose best matching is a - 1, b - 2 = 3
    c["keep_conflict"] = (rec([(0, 0, box(0)), (1, 1, box(3)), (2, 1, box(3)), (2, 0, box(0))]),
                          rec([(0, 1, box(0)), (1, 1, box(3)), (2, 1, box(2)), (2, 2, box(6))]), 3, 0.3,
                          dict(n_gt=4, n_hyp=4, tp=3, fp=1, fn=1, idsw=0, frag=0, mt=1, pt=1, ml=0, idtp=3, idfp=1, idfn=1))
    # inter 50, union 100: 0.5 in float32 exactly, and iou >= iou_min holds
    c["iou_equals_iou_min"] = (rec([(0, 0, box(0))]), rec([(0, 0, box(0, h=5.0))]), 1, 0.5,
                               dict(n_gt=1, n_hyp=1, tp=1, fp=0, fn=0, idsw=0, frag=0, mt=1, pt=0, ml=0, idtp=1, idfp=0, idfn=0))
    c["labels_differ"] = (rec([(0, 0, box(0, label=6.0))]), rec([(0, 0, box(0, label=14.0))]), 1, 0.5,
                          dict(n_gt=1, n_hyp=1, tp=0, fp=1, fn=1, idsw=0, frag=0, mt=0, pt=0, ml=1, idtp=0, idfp=1, idfn=1))
    # a row without a track can never be paired; the tracked row beside it can
    c["hyp_without_track"] = (rec([(0, 0, box(0)), (0, 1, box(50))]), rec([(0, -1, box(0)), (0, 4, box(50)), (0, -1, box(51))]), 1, 0.5,
                              dict(n_gt=2, n_hyp=3, tp=1, fp=2, fn=1, idsw=0, frag=0, mt=1, pt=0, ml=1, idtp=1, idfp=2, idfn=1))
    return c


def crowd(seed, ng, nh, n_windows=2, size=20.0, jitter=3.0):
    """One crowded scene: max(ng, nh) vehicles on a field so dense that every box has several allowed partners at iou_min = 0.3 (the
    assignment has to augment along paths longer than one); ground truth = the first ng, hypothesis = a shuffled, jittered copy of the
    first nh, in every window, the scene drifting; in the later windows a few hypothesis ids are exchanged, so the keep step meets
    wrong, taken and missing tracks.  -> (gt, hyp, n_windows, 0.3)"""
    r = np.random.RandomState(seed)
    n = max(ng, nh)
    field = max(30.0, (n * 324.0 / 6.0) ** 0.5)
    centre = r.uniform(0, field, (n, 2))
    label = np.where(r.rand(n) < 0.8, 6.0, 14.0)
    g_items, h_items = [], []
    ids = r.permutation(nh) + 100
    for w in range(n_windows):
        pos = centre + w * np.array([2.0, 1.0])
        for k in r.permutation(ng):
            g_items.append((w, int(k), [pos[k, 0], pos[k, 1], pos[k, 0] + size, pos[k, 1] + size, 1.0, label[k]]))
        if w == 1 and nh >= 4:
            sw = r.choice(nh, 4, replace=False)
            ids[sw] = ids[np.roll(sw, 1)]
        for k in r.permutation(nh):
            p = pos[k] + r.normal(0, jitter, 2)
            s = size + r.normal(0, 1.0, 2)
            h_items.append((w, int(ids[k]), [p[0], p[1], p[0] + s[0], p[1] + s[1], r.uniform(0.3, 1.0), label[k]]))
    return rec(g_items), rec(h_items), n_windows, 0.3


def traffic(seed, n_windows=12, n_tracks=5, empty=(3,), no_gt=(5,), no_hyp=(7,), extra=3):
    """A sparse recording: n_tracks vehicles drive along lanes; the hypothesis is a jittered copy with dropped rows, rows without a
    track, `extra` spurious tracks and one id change per vehicle; the windows listed are empty on both sides / one side.
    -> (gt, hyp, n_windows, 0.5)"""
    r = np.random.RandomState(seed)
    g_items, h_items = [], []
    change = r.randint(2, n_windows, n_tracks)
    for w in range(n_windows):
        if w in empty:
            continue
        for k in range(n_tracks):
            if r.rand() < 0.1:
                continue
            x, y = 5.0 * w + 3.0 * k, 40.0 * k
            if w not in no_gt:
                g_items.append((w, 10 + k, [x, y, x + 30.0, y + 20.0, 1.0, 6.0 if k % 2 else 14.0]))
            if w not in no_hyp and r.rand() > 0.15:
                j = r.normal(0, 1.5, 4)
                tid = -1 if r.rand() < 0.1 else (k if w < change[k] else 50 + k)
                h_items.append((w, tid, [x + j[0], y + j[1], x + 30.0 + j[2], y + 20.0 + j[3], r.uniform(0.2, 1.0), 6.0 if k % 2 else 14.0]))
        if w not in no_hyp:
            for e in range(extra):
                if r.rand() < 0.5:
                    x, y = r.uniform(0, 200, 2)
                    h_items.append((w, 200 + e, [x, y, x + 30.0, y + 20.0, r.uniform(0.2, 1.0), 6.0]))
    return rec(g_items), rec(h_items), n_windows, 0.5


def with_session(record, s):
    return record + (np.full(len(record[0]), s, np.int64),)


def interleave(records, seed):
    """several one-session records -> one record with a session column whose rows arrive interleaved, as a bank gives them: a random
    merge that keeps every session's own row order"""
    r = np.random.RandomState(seed)
    tagged = [with_session(rc, s) for s, rc in enumerate(records)]
    owner = np.concatenate([np.full(len(rc[0]), s) for s, rc in enumerate(records)])
    owner = owner[r.permutation(len(owner))]
    at = [0] * len(records)
    pick = []
    base = np.concatenate([[0], np.cumsum([len(rc[0]) for rc in records])])
    for s in owner:
        pick.append(base[s] + at[s])
        at[s] += 1
    pick = np.asarray(pick, np.int64)
    return tuple(np.concatenate([t[k] for t in tagged])[pick] for k in range(4))
