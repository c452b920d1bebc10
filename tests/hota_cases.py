"""Helper (not a test): the inputs the HOTA tests share (test_hota_ref_cpu.py proves every one of them unique, test_gpu_hota.py runs them
through the kernels).  name -> (gt, hyp, n_windows); `reference(name)` is tests/hota_ref.evaluate with the uniqueness check, computed
once per process and never changed."""
import functools

import numpy as np

import hota_ref
import mot_cases

box, rec = mot_cases.box, mot_cases.rec


def lanes(seed, n_lanes=5, pool=60, W=80):
    """5 ground-truth tracks on 5 lanes, 300 hypothesis tracks: lane k's hypothesis changes its id (out of `pool` ids of its own) from
    window to window and now and then sits on the next lane's vehicle: 1500 cells, more than the association kernel has threads"""
    r = np.random.RandomState(seed)
    g, h = [], []
    for w in range(W):
        for k in range(n_lanes):
            x, y = 3.0 * w, 25.0 * k
            g.append((w, k, [x, y, x + 30.0, y + 20.0, 1.0, 6.0]))
            tid = 1000 * k + (w if w < pool else int(r.randint(pool)))
            yy = y + (25.0 if r.rand() < 0.3 and k + 1 < n_lanes else 0.0) + r.normal(0, 1.0)
            xx = x + r.normal(0, 1.0)
            h.append((w, tid, [xx, yy, xx + 30.0, yy + 20.0, 0.8, 6.0]))
    return rec(g), rec(h), W


def split_track(n):
    """one ground-truth track of 2n windows followed perfectly by hypothesis id 5 for n windows, then by id 7"""
    return rec([(w, 0, box(3 * w)) for w in range(2 * n)]), rec([(w, 5 if w < n else 7, box(3 * w)) for w in range(2 * n)]), 2 * n


def alignment_wins():
    """Windows 0 .. 3: hypothesis A alone, on the vehicle.  Window 4: A shifted by 3 (IoU .538), a new id B shifted by 1 (.818).  The
    IoU alone prefers B; the alignment (gas(g, A) = .785, gas(g, B) = .112) keeps A: scores .42 against .09."""
    gt = rec([(w, 0, box(0)) for w in range(5)])
    hyp = rec([(w, 11, box(0)) for w in range(4)] + [(4, 22, box(1)), (4, 11, box(3))])
    return gt, hyp, 5


def bank():
    """sessions 0, 1, 3 interleaved as a bank gives them; session 2 has no row at all"""
    recs = [mot_cases.traffic(s) for s in (21, 22, 23)]

    def merged(k, seed):
        got = mot_cases.interleave([r[k] for r in recs], seed)
        return got[:3] + (np.where(got[3] == 2, 3, got[3]),)
    return merged(0, 1), merged(1, 2), 12


def no_hyp_tracks():
    """session 0: the identity-switch case; session 1: ground truth and hypothesis rows, none of which has a track (zero cells);
    session 2: hypothesis tracks and no ground truth"""
    hand = mot_cases.hand_cases()
    g0, h0 = hand["id_switch"][:2]
    g1 = hand["fragmentation"][0]
    h1 = (g1[0], g1[1], np.full(len(g1[0]), -1))
    h2 = hand["fragmentation"][1]
    gt = tuple(np.concatenate([a, b]) for a, b in zip(mot_cases.with_session(g0, 0), mot_cases.with_session(g1, 1)))
    hyp = tuple(np.concatenate([a, b, c]) for a, b, c in zip(mot_cases.with_session(h0, 0), mot_cases.with_session(h1, 1), mot_cases.with_session(h2, 2)))
    return gt, hyp, 4


CROWDS = {"crowd_5x9": 1, "crowd_9x5": 1, "crowd_70x70": 1, "crowd_256x256": 1, "crowd_256x3": 1, "crowd_3x256": 1}      # name -> seed
RANDOM = ("traffic", "bank", "lanes_5x300", "lanes_300x5") + tuple(CROWDS)
HAND = tuple(sorted(mot_cases.hand_cases())) + ("split_track", "alignment_wins", "cells_3x1", "no_hyp_tracks")
NAMES = HAND + RANDOM


@functools.lru_cache(maxsize=None)
def case(name):
    hand = mot_cases.hand_cases()
    if name in hand:
        return hand[name][:3]
    if name == "split_track":
        return split_track(4)
    if name == "alignment_wins":
        return alignment_wins()
    if name == "cells_3x1":                      # three ground-truth tracks one after the other, one hypothesis track: 3 x 1 cells
        return rec([(w, 10 * (w // 2), box(2 * w)) for w in range(6)]), rec([(w, 3, box(2 * w + 1)) for w in range(6)]), 6
    if name == "no_hyp_tracks":
        return no_hyp_tracks()
    if name == "traffic":                        # windows without ground truth, without hypotheses, with neither, with one row
        return mot_cases.traffic(1)[:3]
    if name == "bank":
        return bank()
    if name in CROWDS:                           # crowd_<ng>x<nh>: both transpositions, long augmenting paths, the cap of 256 rows
        ng, nh = (int(v) for v in name[6:].split("x"))
        return mot_cases.crowd(CROWDS[name], ng, nh)[:3]
    if name in ("lanes_5x300", "lanes_300x5"):
        gt, hyp, W = lanes(31)
        return (gt, hyp, W) if name == "lanes_5x300" else (hyp, gt, W)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    return hota_ref.evaluate(*case(name), check_unique=True)
