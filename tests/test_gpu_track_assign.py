"""The tracker's optimal association rule on the GPU: mmd_track_update_assign / mmd_track_update_bank_assign with assign = 1
(csrc/track.hip) against the scipy restatement (tests/track_assign_ref.py) - track ids AND final state, bit for bit - and through
TrackConfig(assign="optimal"): tracker.track_rows, AudioDetector.track_stream, live sessions, banks and detect.py --track_assign.

Every scene compared bit for bit is first shown, on the host, to have ONE optimum: the restatement's margin (the loss of the best
matching that lacks a chosen pair) is above 1e-6 in every window, where float64 sums of at most 256 IoUs err by about 1e-13.  The small
detector and the recordings are the ones of tests/test_gpu_track.py, built again here."""
import os
import sys

import numpy as np
import pytest
import torch

import track_assign_ref
import track_ref
from helpers import make_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = -77
MARGIN = 1e-6
NAN = float("nan")
_CACHE = {}
box = track_assign_ref.box


def _cfg(**kw):
    from mm_distillnet_amd.tracker import TrackConfig
    kw.setdefault("assign", "optimal")
    return TrackConfig(**kw)


def _record(windows):
    rows = [r for w in windows for r in w]
    win = [i for i, w in enumerate(windows) for _ in w]
    return np.asarray(rows, np.float32).reshape(-1, 6), np.asarray(win, np.int32), len(windows)


def _grid(n, dx=0, dy=0, cols=10, pitch=12, size=10, label=6, score=0.9):
    """n boxes on a grid that do not touch each other, moved by (dx, dy): each overlaps only its own successor"""
    return [(2 + pitch * (k % cols) + dx, 2 + pitch * (k // cols) + dy, 2 + pitch * (k % cols) + dx + size,
             2 + pitch * (k // cols) + dy + size, score, label) for k in range(n)]


def _want(windows, cfg, slots=None, glob=None):
    """the restatement's (ids, slots, glob) - and the proof that the scene has one optimum per window, before the device is asked"""
    want = track_assign_ref.track(*_record(windows), cfg, slots, glob)
    assert want[3] > MARGIN, "the scene has a window whose optimum is not unique: margin %g" % want[3]
    return want[:3]


def _direct(rows, window, n_windows, cfg, B, cap_img=None, fill=0.0, dirty=False, state=None, assign=1, old_entry=False):
    """The record through direct mmd_track_update_assign calls (old_entry: mmd_track_update), B windows per call -> (ids [R + 2], slots,
    glob) as numpy.  dirty / fill: as tests/test_gpu_track.py - other boxes and counts of 1 << 30, -5 and 3 in the windows behind
    n_valid, a negative count for an empty window, 1 << 30 for a window that fills cap_img; `fill` lies behind the counts."""
    from mm_distillnet_amd import _lib
    from mm_distillnet_amd.tracker import new_state
    R = len(rows)
    counts = np.bincount(window, minlength=n_windows)
    cap_img = max(1, int(counts.max())) if cap_img is None else cap_img
    first_row = np.concatenate([[0], np.cumsum(counts)])
    rec_track = torch.full((R + 2,), GUARD, dtype=torch.int32, device=DEV)
    state = new_state(DEV, cfg) if state is None else state
    junk = np.asarray(_grid(min(cap_img, 7), 1, 1), np.float32)
    for g0 in range(0, n_windows, B):
        nv = min(B, n_windows - g0)
        packed = np.full((B, cap_img, 6), fill, np.float32)
        cnt = np.zeros(B, np.int32)
        for i in range(nv):
            c = int(counts[g0 + i])
            packed[i, :c] = rows[first_row[g0 + i]:first_row[g0 + i + 1]]
            cnt[i] = c
            if dirty and c == 0:
                cnt[i] = -7
            if dirty and c == cap_img:
                cnt[i] = 1 << 30
        if dirty:
            for i in range(nv, B):
                packed[i, :len(junk)] = junk
                cnt[i] = (1 << 30, -5, 3)[i % 3]
        args = (torch.from_numpy(packed).to(DEV), torch.from_numpy(cnt).to(DEV), B, cap_img,
                torch.tensor([nv, g0], dtype=torch.int32, device=DEV), torch.tensor([int(first_row[g0])], dtype=torch.int32, device=DEV),
                max(1, R), rec_track, state[0], state[1], cfg.max_tracks, cfg.iou_min, cfg.beta, cfg.max_age, cfg.birth_score)
        if old_entry:
            _lib.call("mmd_track_update", *args)
        else:
            _lib.call("mmd_track_update_assign", *args, assign)
    torch.cuda.synchronize()
    return rec_track.cpu().numpy(), state[0].cpu().numpy(), state[1].cpu().numpy()


def _check(windows, cfg, B, overflow=0, **kw):
    """direct calls, twice, against the restatement: ids, guard words, slots and {next_id, overflow}"""
    rows, window, n = _record(windows)
    want = _want(windows, cfg)
    assert int(want[2][1]) == overflow
    for _ in range(2):
        ids, slots, glob = _direct(rows, window, n, cfg, B, **kw)
        np.testing.assert_array_equal(ids[:len(rows)], want[0])
        assert (ids[len(rows):] == GUARD).all()
        np.testing.assert_array_equal(slots, want[1])
        np.testing.assert_array_equal(glob, want[2])
    return want


def _check_track_rows(windows, cfg, group):
    from mm_distillnet_amd.tracker import new_state, track_rows
    rows, window, n = _record(windows)
    want = _want(windows, cfg)
    state = new_state(DEV, cfg)
    got = track_rows(rows, window, n, cfg, DEV, group=group, state=state)
    assert got.dtype == np.int32
    np.testing.assert_array_equal(got, want[0])
    np.testing.assert_array_equal(state[0].cpu().numpy(), want[1])
    np.testing.assert_array_equal(state[1].cpu().numpy(), want[2])


def _random_scene(seed=18, n_windows=20, n_obj=12):
    """tests/test_gpu_track.py's scene with float positions, sizes and velocities (no two IoUs tie): n_obj objects, each missed now and
    then, dying and replaced; the row order is shuffled per window; two labels, so that boxes of unequal label overlap; two empty
    windows in a row.  The area is small enough for the boxes to overlap their neighbours: the windows hold real assignment problems."""
    if ("scene", seed, n_windows, n_obj) not in _CACHE:
        rng = np.random.default_rng(seed)

        def born():
            return dict(x=rng.uniform(0, 60), y=rng.uniform(0, 60), s=rng.uniform(12, 25), vx=rng.uniform(-4, 4), vy=rng.uniform(-4, 4),
                        label=int(rng.choice([6, 14])))

        objs = [born() for _ in range(n_obj)]
        windows = []
        for w in range(n_windows):
            dets = []
            for k, o in enumerate(objs):
                if rng.random() < 0.06:
                    objs[k] = o = born()
                if rng.random() < 0.85:
                    dets.append((o["x"], o["y"], o["x"] + o["s"], o["y"] + o["s"], float(rng.integers(30, 100)) / 100, o["label"]))
                o["x"] += o["vx"] + rng.uniform(-1, 1)
                o["y"] += o["vy"] + rng.uniform(-1, 1)
            rng.shuffle(dets)
            windows.append([tuple(d) for d in dets] if w not in (9, 10) else [])
        _CACHE["scene", seed, n_windows, n_obj] = windows
    return _CACHE["scene", seed, n_windows, n_obj]


# ---------------------------------------------------------------------------------------------- kernel against the restatement
def test_optimal_differs_from_greedy():
    cfg = _cfg(**track_assign_ref.DIFFERS_KW)
    want = _check(list(track_assign_ref.DIFFERS), cfg, 2)
    assert want[0].tolist() == [0, 1, 1, 0] and want[2].tolist() == [2, 0]                 # the first track took the second box
    greedy = track_ref.track(*_record(list(track_assign_ref.DIFFERS)), cfg)
    assert greedy[0].tolist() == [0, 1, 0, 2]
    _check(list(track_assign_ref.DIFFERS), cfg, 1)
    _check_track_rows(list(track_assign_ref.DIFFERS), cfg, 1)


def test_maximum_weight_not_maximum_cardinality():
    want = _check(list(track_assign_ref.WEIGHT), _cfg(), 2)
    assert want[0].tolist() == [0, 1, 0, 2] and want[2].tolist() == [3, 0]                 # one pair; the other box is born
    assert want[1][1, 10] == 1 and want[1][1, 11] == 1 and want[1][2, :2].tolist() == [1, 2]      # the other track aged


def test_transposed_problems():
    three = [box(0), box(6, 2), box(-7, 3)]
    one = [box(2, 1)]
    want = _check([three, one, one], _cfg(), 3)                                            # three live tracks, one box
    assert want[0].tolist() == [0, 1, 2, 0, 0]
    want = _check([one, three, three[::-1]], _cfg(), 2)                                    # one track, three boxes
    assert want[0].tolist() == [0, 0, 1, 2, 2, 1, 0]
    # more slots than boxes with several pairs: five tracks, three boxes, the rows shuffled
    five = [box(0), box(30, 4), box(9, 1), box(38, 9), box(70)]
    _check([five, [box(33, 6), box(4, 1), box(72, 1)], [box(5, 1), box(74, 2), box(36, 8), box(12, 2)]], _cfg(), 3)


def test_empty_windows_and_the_first_birth():
    _check([[], [], []], _cfg(), 3)
    _check([[]], _cfg(), 1)
    want = _check([[(10, 10, 30, 30, 0.5, 6)]], _cfg(), 1)
    assert want[0].tolist() == [0] and want[2].tolist() == [1, 0] and want[1][0, :2].tolist() == [1, 0]
    _check([[], [(10, 10, 30, 30, 0.5, 6)], [], [], [], [(10, 10, 30, 30, 0.5, 6)]], _cfg(), 4)
    _check_track_rows([[], [(10, 10, 30, 30, 0.5, 6)], []], _cfg(), 2)


def test_more_objects_than_one_wave():
    cfg = _cfg(max_tracks=128)
    windows = [_grid(65), _grid(70, 1, 0), _grid(70, 2, 1), [], _grid(70, 4, 3)[::-1]]
    want = _check(windows, cfg, 2)
    assert want[0][:65].tolist() == list(range(65)) and want[0][65:135].tolist() == list(range(70))
    assert want[0][-70:].tolist() == list(range(70))[::-1] and want[2].tolist() == [70, 0]
    _check(windows, cfg, 5)
    _check_track_rows(windows, cfg, 3)


def test_full_capacity_and_the_box_cap():
    cfg = _cfg(max_tracks=256)
    many = _grid(257, cols=32, pitch=4, size=3)
    moved = _grid(257, 0.5, 0.25, cols=32, pitch=4, size=3)
    want = _check([many[:256], moved[:256][::-1], many[:256]], cfg, 2)                     # 256 slots, 256 boxes: a 256 x 256 problem
    assert want[0][256:512].tolist() == list(range(256))[::-1] and want[2].tolist() == [256, 0]
    want = _check([many, moved], cfg, 2, overflow=1)                                       # 257 boxes: the last row gets -1
    assert want[0][:257].tolist() == list(range(256)) + [-1] and want[0][257:].tolist() == list(range(256)) + [-1]
    from mm_distillnet_amd.tracker import track_rows
    with pytest.raises(RuntimeError, match="257 detections"):
        track_rows(*_record([many]), cfg, DEV)


def test_a_dense_window_of_overlapping_boxes():
    """48 boxes in a small area, jittered from window to window: most slots have several allowed boxes, so the solver walks augmenting
    paths of more than one step"""
    windows = _random_scene(seed=3, n_windows=5, n_obj=48)[:5]
    cfg = _cfg(max_tracks=128, iou_min=0.2)
    rows, window, n = _record(windows)
    iou = track_ref.iou_matrix(rows[window == 0][:, :4], rows[window == 1][:, :4])
    assert ((iou >= 0.2).sum(axis=1) >= 2).sum() >= 10
    _check(windows, cfg, 5)
    _check(windows, cfg, 2)


def test_label_gating_and_a_nan_coordinate():
    a, b = box(10, 10, label=6), box(10, 10, label=14)                                     # coincident, unequal labels
    want = _check([[a, b], [box(11, 10, label=14), box(9, 10, label=6)]], _cfg(), 2)
    assert want[0].tolist() == [0, 1, 1, 0]
    # a box with a NaN coordinate takes no pair (its IoUs are NaN: not allowed, weight 0); its birth follows the restatement
    bad = (NAN, 10, 30, 30, 0.9, 6)
    want = _check([[box(10, 10), box(50, 10)], [box(52, 10), bad, box(11, 10)], [box(12, 10), box(54, 10), bad]], _cfg(), 3)
    assert want[0].tolist() == [0, 1, 1, 2, 0, 0, 1, 3]


def test_overflow_is_sticky_and_leaves_the_fitting_tracks_alone():
    cfg = _cfg(max_tracks=8)
    extra = (100, 100, 110, 110, 0.9, 6)
    fit = [_grid(8), _grid(8, 1, 0), _grid(8, 2, 0)]
    over = [_grid(8), _grid(8, 1, 0) + [extra], _grid(8, 2, 0)]
    a = _check(fit, cfg, 1)
    b = _check(over, cfg, 1, overflow=1)                     # one launch per window: the flag survives the third launch
    assert a[2].tolist() == [8, 0] and b[2].tolist() == [8, 1] and b[0][16] == -1
    np.testing.assert_array_equal(a[1], b[1])
    _check(over, cfg, 3, overflow=1)
    from mm_distillnet_amd.tracker import track_rows
    with pytest.raises(RuntimeError, match="max_tracks = 8"):
        track_rows(*_record(over), cfg, DEV)


@pytest.mark.parametrize("group", [1, 3, 8])
def test_random_scene_gives_the_same_bits_for_every_group_size(group):
    windows = _random_scene()
    cfg = _cfg()
    want = _check(windows, cfg, group)
    per_id = np.bincount(want[0][want[0] >= 0])
    assert len(windows) == 20 and want[2][0] > 12 and want[2][1] == 0 and (per_id >= 5).sum() >= 8      # births, deaths, long tracks
    greedy = track_ref.track(*_record(windows), cfg)
    print("rows whose id differs from the greedy rule's: %d of %d" % (int((greedy[0] != want[0]).sum()), len(want[0])))
    _check_track_rows(windows, cfg, group)
    _check(windows, _cfg(iou_min=0.5, beta=0.25, max_age=0, birth_score=0.5, max_tracks=16), group)


def test_the_state_of_one_call_is_the_start_of_the_next():
    from mm_distillnet_amd.tracker import new_state
    windows = _random_scene()[:8]
    cfg = _cfg(max_tracks=32)
    rows, window, n = _record(windows)
    want = _want(windows, cfg)
    state = new_state(DEV, cfg)
    ids, slots, glob = _direct(rows, window, n, cfg, 3, state=state)
    np.testing.assert_array_equal(ids[:len(rows)], want[0])
    on = _want(windows, cfg, want[1], want[2])               # the same windows again, from that state: ids go on behind next_id
    ids2, slots2, glob2 = _direct(rows, window, n, cfg, 3, state=state)
    np.testing.assert_array_equal(ids2[:len(rows)], on[0])
    np.testing.assert_array_equal(slots2, on[1])
    np.testing.assert_array_equal(glob2, on[2])
    assert glob2[0] > glob[0]


def test_padding_windows_bad_counts_and_rows_behind_the_counts_are_not_read():
    windows = _random_scene()[:11]                            # 11 windows in groups of 4: the last group has n_valid = 3
    cfg = _cfg()
    clean = _check(windows, cfg, 4)
    dirty = _check(windows, cfg, 4, dirty=True, fill=NAN)
    for a, b in zip(clean, dirty):
        np.testing.assert_array_equal(a, b)
    full = [_grid(5), _grid(3, 1, 0), _grid(5, 2, 0)]         # a window that fills cap_img, its count given as 1 << 30
    _check(full, cfg, 2, cap_img=5, dirty=True, fill=NAN)


def test_assign_zero_through_the_new_entry_point_is_the_old_entry_point():
    windows = _random_scene()
    rows, window, n = _record(windows)
    cfg = _cfg(assign="greedy")
    want = track_ref.track(rows, window, n, cfg)
    old = _direct(rows, window, n, cfg, 3, old_entry=True)
    new = _direct(rows, window, n, cfg, 3, assign=0)
    for a, b in zip(old, new):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(new[0][:len(rows)], want[0])
    np.testing.assert_array_equal(new[1], want[1])
    np.testing.assert_array_equal(new[2], want[2])
    optimal = _direct(rows, window, n, _cfg(), 3)
    assert not np.array_equal(optimal[0], new[0])             # and assign = 1 is another rule


# ---------------------------------------------------------------------------------------------- the bank kernel
def _bank_direct(sessions, order, cfg, B, n_sessions, assign=1):
    """sessions: per session its list of windows; order: the session of every row of the run, a session's windows in rising order;
    B rows per launch of mmd_track_update_bank_assign -> (per session the ids of its rows in window order, slots [n_sessions, ..], glob)"""
    from mm_distillnet_amd import _lib
    from mm_distillnet_amd.tracker import new_bank_state
    cap_img = max(1, max(len(w) for s in sessions for w in s))
    total = sum(len(sessions[s][k]) for s, k in order)
    rec_track = torch.full((total + 2,), GUARD, dtype=torch.int32, device=DEV)
    state = new_bank_state(DEV, cfg, n_sessions)
    snapshots, done = [], 0
    for g0 in range(0, len(order), B):
        part = order[g0:g0 + B]
        packed = np.full((B, cap_img, 6), NAN, np.float32)
        cnt, sess, widx = np.full(B, 1 << 30, np.int32), np.full(B, 1, np.int32), np.full(B, 5, np.int32)
        for i, (s, k) in enumerate(part):
            packed[i, :len(sessions[s][k])] = np.asarray(sessions[s][k], np.float32).reshape(-1, 6)
            cnt[i], sess[i], widx[i] = len(sessions[s][k]), s, k
        _lib.call("mmd_track_update_bank_assign", torch.from_numpy(packed).to(DEV), torch.from_numpy(cnt).to(DEV), B, cap_img,
                  torch.tensor([len(part)], dtype=torch.int32, device=DEV), torch.from_numpy(sess).to(DEV), torch.from_numpy(widx).to(DEV),
                  n_sessions, torch.tensor([done], dtype=torch.int32, device=DEV), max(1, total), rec_track, state[0], state[1],
                  cfg.max_tracks, cfg.iou_min, cfg.beta, cfg.max_age, cfg.birth_score, assign)
        done += sum(len(sessions[s][k]) for s, k in part)
        snapshots.append((sorted({s for s, _ in part}), state[0].cpu().numpy().copy()))
    torch.cuda.synchronize()
    flat = rec_track.cpu().numpy()
    assert (flat[total:] == GUARD).all()
    ids, at = [[] for _ in sessions], 0
    for s, k in order:
        ids[s].append(flat[at:at + len(sessions[s][k])])
        at += len(sessions[s][k])
    return [np.concatenate(x) if x else np.zeros(0, np.int32) for x in ids], state[0].cpu().numpy(), state[1].cpu().numpy(), snapshots


@pytest.mark.parametrize("n_sessions", [2, 3])
def test_bank_sessions_interleaved_give_the_single_kernels_bits(n_sessions):
    cfg = _cfg(max_tracks=32)
    sessions = [_random_scene(seed=7)[:9], _random_scene(seed=8)[:7], list(track_assign_ref.DIFFERS) * 2][:n_sessions]
    # session 2 (when there) runs in the first rows only: the later groups do not hold it
    order = [(2, k) for k in range(4)] if n_sessions == 3 else []
    left = [list(range(len(s))) for s in sessions[:2]]
    rng = np.random.default_rng(n_sessions)
    while left[0] or left[1]:
        s = int(rng.choice([k for k in (0, 1) if left[k]]))
        order.append((s, left[s].pop(0)))
    B = 4
    ids, slots, glob, snapshots = _bank_direct(sessions, order, cfg, B, n_sessions)
    assert any(len(present) >= 2 for present, _ in snapshots)                               # a group that mixes sessions
    for s in range(n_sessions):
        want = _want(sessions[s], cfg)
        rows, window, n = _record(sessions[s])
        single = _direct(rows, window, n, cfg, 3)
        np.testing.assert_array_equal(ids[s], want[0])
        np.testing.assert_array_equal(ids[s], single[0][:len(rows)])
        np.testing.assert_array_equal(slots[s], want[1])
        np.testing.assert_array_equal(slots[s], single[1])
        np.testing.assert_array_equal(glob[s], want[2])
    # a session absent from a group keeps every word of its state
    absent = 0
    for (_, before), (present, after) in zip(snapshots[:-1], snapshots[1:]):
        for s in range(n_sessions):
            if s not in present:
                np.testing.assert_array_equal(before[s], after[s])
                absent += bool(before[s][:, 0].any())
    assert absent >= 1 or n_sessions == 2


# ---------------------------------------------------------------------------------------------- through the layers
S, COEF, C = 128, 2, 8
WIN, HOP, BATCH, N_REC = 4096, 1531, 3, 14000             # 7 windows: two full groups, one of one window; a tail is dropped


def _recording(seed):
    from mm_distillnet_amd.data import synthetic_waveforms
    return synthetic_waveforms(24, seed, N_REC)


def _state():
    if "state" not in _CACHE:
        from mm_distillnet_amd.audio import MelFrontEnd
        from mm_distillnet_amd.synth import tune_teacher_bias
        spec, st = make_state(COEF, 8, 13, "audio")
        w = _recording(11)
        x = MelFrontEnd(DEV).student_input(torch.stack([w[:, k * HOP:k * HOP + WIN] for k in range(7)]).to(DEV), None, S, db=True).cpu()
        tune_teacher_bias(spec, st, x, DEV, 40)
        _CACHE["state"] = (spec, st)
    spec, st = _CACHE["state"]
    return spec, {k: v.clone() for k, v in st.items()}


def _detector():
    from mm_distillnet_amd.detector import AudioDetector
    spec, st = _state()
    det = AudioDetector(spec, DEV, image_size=S)
    det.load(st)
    return det


def _e2e(**kw):
    return _cfg(max_tracks=256, **kw)


def _plain():
    """detect_stream's record of recording 11 from a detector that never tracked, the restatements' ids on it (optimal: its margin is
    checked here, before any tracked run) -> (rows, window, optimal ids, greedy ids)"""
    if "plain" not in _CACHE:
        rows, window = _detector().detect_stream(_recording(11).to(DEV), WIN, HOP, batch=BATCH)
        ids, _, glob, margin = track_assign_ref.track(rows, window, 7, _e2e())
        greedy = track_ref.track(rows, window, 7, _e2e(assign="greedy"))[0]
        print("rows per window %s, tracks %d, margin %g, rows whose id differs from greedy's: %d"
              % (np.bincount(window, minlength=7).tolist(), glob[0], margin, int((ids != greedy).sum())))
        assert glob[1] == 0 and margin > MARGIN and len(rows) > 0 and ids.max() >= 1
        _CACHE["plain"] = (rows, window, ids, greedy)
    return _CACHE["plain"]


def _same(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape
        np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32))


def test_track_stream_track_rows_and_the_rekeyed_graph():
    from mm_distillnet_amd.tracker import track_rows
    rows, window, ids, greedy = _plain()
    det = _detector()
    w = _recording(11).to(DEV)
    first = det.track_stream(w, WIN, HOP, batch=BATCH, track=_e2e(assign="greedy"))
    _same(first, (rows, window, greedy))
    assert det.stream_captures == 1
    _same(det.track_stream(w, WIN, HOP, batch=BATCH, track=_e2e()), (rows, window, ids))       # detect_stream's rows, the restatement's ids
    assert det.stream_captures == 2                                                       # the rule re-keyed the captured chain
    _same(det.track_stream(w, WIN, HOP, batch=BATCH, track=_e2e()), (rows, window, ids))
    assert det.stream_captures == 2
    _same(det.track_stream(w, WIN, HOP, batch=BATCH, track=_e2e(assign="greedy")), first)      # and greedy again: the first result
    assert det.stream_captures == 3
    np.testing.assert_array_equal(track_rows(rows, window, 7, _e2e(), DEV), ids)
    np.testing.assert_array_equal(track_rows(rows, window, 7, _e2e(), DEV, group=3), ids)
    det.use_graph = False
    _same(det.track_stream(w, WIN, HOP, batch=BATCH, track=_e2e()), (rows, window, ids))


def test_live_session_and_bank_fed_in_chunks_give_the_same_ids():
    rows, window, ids, _ = _plain()
    w = _recording(11)
    edges = [0, 1, 3000, 10500, 10501, N_REC]
    chunks = [w[:, a:b] for a, b in zip(edges[:-1], edges[1:])]
    det = _detector()
    session = det.open_stream(WIN, HOP, batch=BATCH, track=_e2e())
    parts = [session.push(c) for c in chunks] + [session.flush()]
    _same(tuple(np.concatenate([p[i] for p in parts]) for i in range(3)), (rows, window, ids))
    session.close()
    bank = det.open_bank(2, WIN, HOP, batch=BATCH, track=_e2e())
    parts = []
    for k, c in enumerate(chunks):                            # the two sessions hear the same recording, a chunk apart
        parts.append(bank.push(k % 2, c))
        parts.append(bank.push(1 - k % 2, c))
    got = bank.concat(parts + [bank.flush()])
    bank.close()
    assert len(got) == 4
    for s in range(2):                                        # per session: the restatement on the rows the bank returned for it
        m = got[1] == s
        assert (np.diff(got[2][m]) >= 0).all() and m.sum() == len(rows)
        want = track_assign_ref.track(got[0][m], got[2][m], 7, _e2e())
        assert want[3] > MARGIN and want[2][1] == 0
        np.testing.assert_array_equal(got[3][m], want[0])
        np.testing.assert_array_equal(got[3][m], ids)         # the same vehicles, the same ids as the stream gave


def test_command_line_tool_takes_the_rule(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    sys.path.insert(0, ROOT)
    import detect
    rows, window, ids, greedy = _plain()
    spec, st = _state()
    torch.save({"state_dict": st, "epoch": 3}, tmp_path / "student.pth")
    np.save(tmp_path / "rec.npy", _recording(11).numpy())
    cfgf = os.path.join(ROOT, "configs", "mm-distillnet.cfg")
    argv = ["--config_file", cfgf, "--checkpoint", str(tmp_path / "student.pth"), "--input", str(tmp_path / "rec.npy"),
            "--overwrite", '{"image_size": %d}' % S, "--window_s", repr(WIN / 44100), "--hop_s", repr(HOP / 44100), "--batch", str(BATCH),
            "--track", "--track_max", "256"]
    _same(detect.main(argv + ["--output", "optimal.csv", "--track_assign", "optimal"]), (rows, window, ids))
    lines = open(tmp_path / "optimal.csv").read().strip().split("\n")
    assert lines[0] == "window,t_start_s,x1,y1,x2,y2,score,label,track" and len(lines) == 1 + len(rows)
    assert [int(ln.split(",")[8]) for ln in lines[1:]] == ids.tolist()
    # without the flag: the rows and ids of the greedy rule, the file byte for byte the one --track_assign greedy writes
    _same(detect.main(argv + ["--output", "default.csv"]), (rows, window, greedy))
    _same(detect.main(argv + ["--output", "greedy.csv", "--track_assign", "greedy"]), (rows, window, greedy))
    default = open(tmp_path / "default.csv", "rb").read()
    assert default == open(tmp_path / "greedy.csv", "rb").read()
    assert [int(ln.split(",")[8]) for ln in default.decode().strip().split("\r\n")[1:]] == greedy.tolist()
