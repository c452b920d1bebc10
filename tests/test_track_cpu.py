"""Streaming tracking, CPU side: the numpy restatement of the association rule (tests/track_ref.py) on hand-made scenes, TrackConfig's
range checks, `tracker.tracks_table`, detect.py's --track option and its CSV writer, and the C ABI of mmd_track_update without a GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

import track_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _detect():
    sys.path.insert(0, ROOT)
    import detect
    return detect


def _cfg(**kw):
    from mm_distillnet_amd.tracker import TrackConfig
    return TrackConfig(**kw)


def _record(windows):
    """windows: per window a list of (x1, y1, x2, y2, score, label) -> (rows [R, 6], window [R], n_windows)"""
    rows = [r for w in windows for r in w]
    win = [i for i, w in enumerate(windows) for _ in w]
    return np.asarray(rows, np.float32).reshape(-1, 6), np.asarray(win, np.int32), len(windows)


def _box(x, y, size=20, score=0.9, label=6):
    return (x, y, x + size, y + size, score, label)


def _ids(windows, **kw):
    out, slots, glob = track_ref.track(*_record(windows), _cfg(**kw))
    return out.tolist(), slots, glob


# ---------------------------------------------------------------------------------------------- the rule, restated
def test_two_boxes_that_cross_keep_their_ids():
    # A moves right, B moves left on the same line, 8 pixels per window; they pass each other between windows 5 and 6 (A 50 -> 58,
    # B 60 -> 52: each lies nearer the OTHER one's last box than its own).  The row order flips in every other window.
    windows = []
    for w in range(11):
        a, b = _box(10 + 8 * w, 40), _box(100 - 8 * w, 40)
        windows.append([a, b] if w % 2 == 0 else [b, a])
    ids, slots, glob = _ids(windows)
    want = [i for w in range(11) for i in ((0, 1) if w % 2 == 0 else (1, 0))]
    assert ids == want
    assert glob.tolist() == [2, 0]
    f = slots.view(np.float32)
    assert slots[0, 0] == 1 and slots[0, 1] == 0 and slots[0, 10] == 11 and slots[0, 11] == 0 and slots[0, 12] == 10
    assert f[0, 2:6].tolist() == [90, 40, 110, 60] and f[1, 2:6].tolist() == [20, 40, 40, 60]
    assert 7.5 < f[0, 6] <= 8 and -8 <= f[1, 6] < -7.5 and f[0, 7] == 0                   # the velocities converged on +-8
    # without the velocity model (beta = 0) the nearer box wins at the crossing and the ids swap
    swapped, _, _ = _ids(windows, beta=0.0)
    assert swapped[:12] == want[:12] and swapped[12:14] == [1, 0]


def test_a_gap_of_max_age_keeps_the_id_one_more_gives_a_new_one():
    b = _box(30, 30)
    for age in (0, 2, 3):
        ids, _, glob = _ids([[b], [b]] + [[]] * age + [[b]], max_age=age)
        assert ids == [0, 0, 0] and glob.tolist() == [1, 0], age
        ids, slots, glob = _ids([[b], [b]] + [[]] * (age + 1) + [[b]], max_age=age)
        assert ids == [0, 0, 1] and glob.tolist() == [2, 0], age
        assert slots[0, 1] == 1 and slots[0, 10] == 1 and slots[0, 12] == age + 3         # the freed slot was taken again
    # a moving box is picked up where the model coasts it to: 10 px per window, two windows missed
    mov = [[_box(10 + 10 * w, 30)] for w in range(5)] + [[], [], [_box(80, 30)]]
    assert _ids(mov)[0] == [0] * 6
    assert _ids(mov, beta=0.0)[0] == [0] * 5 + [1]                                        # without it the box is 30 px away: IoU 0


def test_unequal_labels_are_never_paired():
    ids, slots, glob = _ids([[_box(30, 30, label=6)], [_box(30, 30, label=7)], [_box(30, 30, label=6)]])
    assert ids == [0, 1, 0] and glob.tolist() == [2, 0]
    assert slots.view(np.float32)[:2, 8].tolist() == [6, 7]


def test_an_exact_tie_goes_to_the_lower_slot_then_to_the_lower_detection():
    b = _box(30, 30)
    # two tracks on one box, one detection: slot 0 takes it
    ids, slots, _ = _ids([[b, b], [b]])
    assert ids == [0, 1, 0] and slots[0, 10] == 2 and slots[1, 11] == 1
    # one track, two equal detections: the first row continues it, the second starts a track
    assert _ids([[b], [b, b]])[0] == [0, 0, 1]
    # one track, detections 4 px to either side: the same IoU (16 * 20 / (2 * 400 - 320)) exactly
    left, right = _box(26, 30), _box(34, 30)
    assert _ids([[b], [right, left]])[0] == [0, 0, 1]
    assert _ids([[b], [left, right]])[0] == [0, 0, 1]
    # two tracks, two detections, all four IoUs equal: (slot 0, det 0), then (slot 1, det 1)
    assert _ids([[left, right], [b, b]])[0] == [0, 1, 0, 1]
    iou = track_ref.iou_matrix(np.asarray([b[:4]], np.float32), np.asarray([left[:4], right[:4]], np.float32))
    assert iou.dtype == np.float32 and iou[0, 0] == iou[0, 1] == np.float32(320) / np.float32(480)


def test_a_slot_freed_in_a_window_is_reused_by_a_birth_in_that_window():
    ids, slots, glob = _ids([[_box(10, 10)], [_box(80, 80)]], max_tracks=1, max_age=0)
    assert ids == [0, 1] and glob.tolist() == [2, 0]                                      # no overflow: the slot was free in time
    assert slots[0, :2].tolist() == [1, 1] and slots.view(np.float32)[0, 2:6].tolist() == [80, 80, 100, 100]
    # with max_age = 1 the old track still holds the only slot
    ids, _, glob = _ids([[_box(10, 10)], [_box(80, 80)]], max_tracks=1, max_age=1)
    assert ids == [0, -1] and glob.tolist() == [1, 1]


def test_birth_score_holds_back_weak_rows_but_not_matches():
    weak, strong = _box(30, 30, score=0.2), _box(30, 30, score=0.6)
    ids, slots, glob = _ids([[weak], [weak], [strong], [weak]], birth_score=0.5)
    assert ids == [-1, -1, 0, 0] and glob.tolist() == [1, 0]                              # a weak row still continues a track
    assert slots.view(np.float32)[0, 9] == np.float32(0.2) and slots[0, 10] == 2
    assert _ids([[_box(30, 30, score=0.5)]], birth_score=0.5)[0] == [0]                   # >=
    assert _ids([[_box(30, 30, score=float("nan"))]])[0] == [-1]                          # the comparison is false for NaN


def test_one_object_more_than_max_tracks_sets_overflow():
    objs = [_box(5 + 24 * k, 10) for k in range(5)]
    ids, slots, glob = _ids([objs, objs], max_tracks=4)
    assert ids == [0, 1, 2, 3, -1] * 2 and glob.tolist() == [4, 1]
    fit, slots_fit, glob_fit = _ids([objs[:4], objs[:4]], max_tracks=4)
    assert fit == [0, 1, 2, 3] * 2 and glob_fit.tolist() == [4, 0]
    np.testing.assert_array_equal(slots, slots_fit)                                       # the extra object left the others alone
    # more than 256 rows in a window: the first 256 take part
    many = [_box(4 * (k % 32), 12 * (k // 32), size=3) for k in range(257)]
    ids, _, glob = _ids([many], max_tracks=256)
    assert ids == list(range(256)) + [-1] and glob.tolist() == [256, 1]


def test_ids_are_never_reused():
    a, b, c = _box(10, 10), _box(60, 10), _box(10, 60)
    windows = [[a], [a, b], [b], [b], [b], [b, a], [c], [], [], [], [a, b, c]]
    ids, _, glob = _ids(windows, max_tracks=3)
    assert ids == [0, 0, 1, 1, 1, 1, 1, 2, 3, 4, 5, 6]
    births = [i for k, i in enumerate(ids) if i not in ids[:k]]
    assert births == sorted(births) == list(range(7)) and glob.tolist() == [7, 0]


def test_the_restatement_goes_on_from_a_state():
    """a record cut in two, the second half started from the first half's state, gives the bits of one run"""
    windows = [[_box(10 + 7 * w, 20 + 3 * w), _box(90 - 5 * w, 70)] for w in range(8)]
    rows, win, n = _record(windows)
    whole = track_ref.track(rows, win, n, _cfg())
    cut = int(np.searchsorted(win, 3))
    first = track_ref.track(rows[:cut], win[:cut], 3, _cfg())
    second = track_ref.track(rows[cut:], win[cut:] - 3, 5, _cfg(), first[1], first[2])
    np.testing.assert_array_equal(np.concatenate([first[0], second[0]]), whole[0])
    got = second[1].copy()
    got[:, 12] += 3 * (got[:, 0] != 0)                                                    # last_window counts from the cut
    np.testing.assert_array_equal(got, whole[1])
    np.testing.assert_array_equal(second[2], whole[2])


# ---------------------------------------------------------------------------------------------- TrackConfig, tracks_table
def test_track_config_checks_its_ranges():
    c = _cfg()
    assert (c.iou_min, c.beta, c.max_age, c.birth_score, c.max_tracks) == (0.3, 0.5, 2, 0.0, 64)
    assert _cfg(max_tracks=1).max_tracks == 1 and _cfg(max_tracks=256).max_tracks == 256 and _cfg(max_age=0).max_age == 0
    assert _cfg(iou_min=1.0, beta=0.0).key() == (1.0, 0.0, 2, 0.0, 64) and _cfg(beta=1.0).beta == 1.0
    for bad in (dict(max_tracks=0), dict(max_tracks=257), dict(max_tracks=-1), dict(max_tracks=2.5), dict(max_age=-1), dict(max_age=1.5),
                dict(iou_min=0.0), dict(iou_min=-0.1), dict(iou_min=1.5), dict(iou_min=float("nan")), dict(beta=-0.1), dict(beta=1.1),
                dict(beta=float("nan")), dict(birth_score=float("nan"))):
        with pytest.raises(ValueError, match="TrackConfig"):
            _cfg(**bad)


def test_tracks_table():
    from mm_distillnet_amd.tracker import tracks_table
    window = np.array([0, 0, 1, 1, 3, 3, 3, 7], np.int32)
    track = np.array([0, 1, 0, -1, 2, 0, 1, 2], np.int32)
    t = tracks_table(window, track)
    assert t.dtype == np.int64 and t.tolist() == [[0, 0, 3, 3], [1, 0, 3, 2], [2, 3, 7, 2]]
    assert tracks_table(np.zeros(0, np.int32), np.zeros(0, np.int32)).shape == (0, 4)
    assert tracks_table([4, 5], [-1, -1]).shape == (0, 4)
    with pytest.raises(ValueError):
        tracks_table([0, 1], [0])


# ---------------------------------------------------------------------------------------------- detect.py
def test_track_option_needs_window_s_and_is_refused_before_any_gpu_call(tmp_path, monkeypatch):
    det = _detect()
    import torch

    def refuse(*a, **k):
        raise AssertionError("the GPU was reached")

    monkeypatch.setattr(torch.cuda, "set_device", refuse)
    monkeypatch.setattr(torch, "load", refuse)
    np.save(tmp_path / "one.npy", np.zeros((8, 9000), np.float32))
    cfgf = os.path.join(ROOT, "configs", "mm-distillnet.cfg")
    argv = ["--config_file", cfgf, "--checkpoint", str(tmp_path / "none.pth"), "--input", str(tmp_path / "one.npy"),
            "--output", str(tmp_path / "o.csv"), "--track"]
    with pytest.raises(ValueError, match="--window_s"):
        det.main(argv)
    assert not os.path.exists(tmp_path / "o.csv")
    # a bad tracking parameter is refused there too
    with pytest.raises(ValueError, match="TrackConfig: max_tracks"):
        det.main(argv + ["--window_s", "0.1", "--track_max", "300"])
    with pytest.raises(ValueError, match="TrackConfig: iou_min"):
        det.main(argv + ["--window_s", "0.1", "--track_iou", "0"])
    assert not os.path.exists(tmp_path / "o.csv")


def test_track_csv_writer(tmp_path):
    det = _detect()
    rows = np.array([[1, 2, 30, 40, 0.1 + 0.2, 6], [0, 0, 128, 127, np.float32(1) / 3, 6], [5, 6, 7, 8, 0.999999, 14]], np.float32)
    window, track = np.array([0, 0, 7], np.int32), np.array([0, -1, 12], np.int32)
    assert det.write_windows_csv(str(tmp_path / "t.csv"), rows, window, 1531, track) == 3
    assert open(tmp_path / "t.csv", "rb").read() == (b"window,t_start_s,x1,y1,x2,y2,score,label,track\r\n"
                                                     b"0,0,1,2,30,40,0.300000012,6,0\r\n"
                                                     b"0,0,0,0,128,127,0.333333343,6,-1\r\n"
                                                     b"7,0.243015873,5,6,7,8,0.999998987,14,12\r\n")
    assert det.write_windows_csv(str(tmp_path / "e.csv"), np.zeros((0, 6), np.float32), np.zeros(0, np.int32), 100, np.zeros(0, np.int32)) == 0
    assert open(tmp_path / "e.csv", "rb").read() == b"window,t_start_s,x1,y1,x2,y2,score,label,track\r\n"
    with pytest.raises(ValueError):
        det.write_windows_csv(str(tmp_path / "x.csv"), rows, window, 1531, track[:2])
    # the stream writer keeps its eight columns
    assert det.STREAM_COLUMNS == ("window", "t_start_s", "x1", "y1", "x2", "y2", "score", "label")
    assert det.write_windows_csv(str(tmp_path / "s.csv"), rows, window, 1531) == 3
    assert open(tmp_path / "s.csv", "rb").read().split(b"\r\n")[:2] == [b"window,t_start_s,x1,y1,x2,y2,score,label", b"0,0,1,2,30,40,0.300000012,6"]


# ---------------------------------------------------------------------------------------------- C ABI without a GPU
def test_header_declares_and_library_exports_the_entry_point():
    import __graft_entry__ as ge
    ge.build()
    from mm_distillnet_amd import _lib
    sigs = _lib.LIB.symbols()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    assert "mmd_track_update" in sigs and hasattr(dll, "mmd_track_update")
    assert len(sigs["mmd_track_update"]) == 16
    assert sigs["mmd_track_update"][11:15] == [ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.c_float]
    assert len(sigs["mmd_det_record_append"]) == 11                                      # the append keeps its arguments
    text = open(_lib.HEADER).read()
    head = text[:text.index("int mmd_track_update(")]
    comment = head[head.rindex("\n\n"):].replace("\n// ", " ")
    for phrase in ("MUST PRECEDE", "never writes it", "need no zeroing", "sticky", "ZERO FILL", "next_id, overflow", "last_window"):
        assert phrase in comment, phrase


def test_bad_arguments_are_rejected_without_gpu():
    import __graft_entry__ as ge
    ge.build()
    from mm_distillnet_amd import _lib
    tu = _lib.LIB.load().mmd_track_update
    p = ctypes.c_void_p(4096)            # never dereferenced: validation precedes any launch

    def call(ptrs=None, B=3, cap_img=4, rec_cap=6, max_tracks=64, max_age=2):
        q = [p] * 7 if ptrs is None else ptrs
        return tu(q[0], q[1], B, cap_img, q[2], q[3], rec_cap, q[4], q[5], q[6], max_tracks, 0.3, 0.5, max_age, 0.0, None)

    for k in range(7):                   # rows, cnt, ctl, rec_count, rec_track, trk_slots, trk_glob
        assert call([None if j == k else p for j in range(7)]) == -22, k
    for B in (0, -3, 1025):
        assert call(B=B) == -22, B
    for cap_img in (0, -1):
        assert call(cap_img=cap_img) == -22
    for rec_cap in (0, -1):
        assert call(rec_cap=rec_cap) == -22
    for max_tracks in (0, -1, 257):
        assert call(max_tracks=max_tracks) == -22
    assert call(max_age=-1) == -22
