"""Streaming tracking on the GPU: mmd_track_update (csrc/track.hip) against the numpy float32 restatement (tests/track_ref.py) - track
ids AND final state, bit for bit: both sides do the same individually rounded fp32 operations, so there is no tolerance -, its offsets
against mmd_det_record_append on one record count, and AudioDetector.track_stream / detect.py --track against detect_stream and the
restatement.  The small detector and the recordings are the ones of tests/test_gpu_stream.py, built again here."""
import os
import sys

import numpy as np
import pytest
import torch

import track_ref
from helpers import make_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = -77
_CACHE = {}


def _cfg(**kw):
    from mm_distillnet_amd.tracker import TrackConfig
    return TrackConfig(**kw)


def _record(windows):
    rows = [r for w in windows for r in w]
    win = [i for i, w in enumerate(windows) for _ in w]
    return np.asarray(rows, np.float32).reshape(-1, 6), np.asarray(win, np.int32), len(windows)


def _grid(n, dx=0, dy=0, cols=10, pitch=12, size=10, label=6, score=0.9):
    """n boxes on a grid that do not touch each other, moved by (dx, dy)"""
    return [(2 + pitch * (k % cols) + dx, 2 + pitch * (k // cols) + dy, 2 + pitch * (k % cols) + dx + size,
             2 + pitch * (k // cols) + dy + size, score, label) for k in range(n)]


def _direct(rows, window, n_windows, cfg, B, cap_img=None, fill=0.0, dirty=False, state=None, rec_cap=None, first_count=0):
    """The record through direct mmd_track_update calls, B windows per call -> (ids [R + 2], slots, glob) as numpy.
    dirty: what a caller may leave where the kernel must not look - other boxes in the windows behind n_valid with counts of 1 << 30,
    -5 and 3 there, a negative count for an empty window, 1 << 30 for a window that fills cap_img.  fill: what lies behind the counts."""
    from mm_distillnet_amd import _lib
    from mm_distillnet_amd.tracker import new_state
    R = len(rows)
    counts = np.bincount(window, minlength=n_windows)
    cap_img = max(1, int(counts.max())) if cap_img is None else cap_img
    first_row = np.concatenate([[0], np.cumsum(counts)])
    rec_cap = max(1, R + first_count) if rec_cap is None else rec_cap
    rec_track = torch.full((R + first_count + 2,), GUARD, dtype=torch.int32, device=DEV)
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
        _lib.call("mmd_track_update", torch.from_numpy(packed).to(DEV), torch.from_numpy(cnt).to(DEV), B, cap_img,
                  torch.tensor([nv, g0], dtype=torch.int32, device=DEV),
                  torch.tensor([first_count + int(first_row[g0])], dtype=torch.int32, device=DEV), rec_cap, rec_track, state[0], state[1],
                  cfg.max_tracks, cfg.iou_min, cfg.beta, cfg.max_age, cfg.birth_score)
    torch.cuda.synchronize()
    return rec_track.cpu().numpy(), state[0].cpu().numpy(), state[1].cpu().numpy()


def _check(windows, cfg, B, overflow=0, **kw):
    """direct calls, twice, against the restatement: ids, guard words, slots and {next_id, overflow}"""
    rows, window, n = _record(windows)
    want = track_ref.track(rows, window, n, cfg)
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
    want = track_ref.track(rows, window, n, cfg)
    state = new_state(DEV, cfg)
    got = track_rows(rows, window, n, cfg, DEV, group=group, state=state)
    assert got.dtype == np.int32
    np.testing.assert_array_equal(got, want[0])
    np.testing.assert_array_equal(state[0].cpu().numpy(), want[1])
    np.testing.assert_array_equal(state[1].cpu().numpy(), want[2])
    np.testing.assert_array_equal(track_rows(rows, window, n, cfg, DEV, group=group), want[0])      # a state of its own


def _random_scene(seed=7, n_windows=20, n_obj=12):
    """n_obj objects with integer positions, sizes and velocities; each is missed now and then, dies and is replaced; the row order
    is shuffled per window.  Two labels, so that boxes of unequal label overlap."""
    if ("scene", seed) not in _CACHE:
        rng = np.random.default_rng(seed)

        def born():
            return dict(x=int(rng.integers(0, 100)), y=int(rng.integers(0, 100)), s=int(rng.integers(12, 25)),
                        vx=int(rng.integers(-4, 5)), vy=int(rng.integers(-4, 5)), label=int(rng.choice([6, 14])))

        objs = [born() for _ in range(n_obj)]
        windows = []
        for w in range(n_windows):
            dets = []
            for k, o in enumerate(objs):
                if rng.random() < 0.06:
                    objs[k] = o = born()
                if rng.random() < 0.85:
                    dets.append((o["x"], o["y"], o["x"] + o["s"], o["y"] + o["s"], float(rng.integers(30, 100)) / 100, o["label"]))
                o["x"] += o["vx"]
                o["y"] += o["vy"]
            rng.shuffle(dets)
            windows.append([tuple(d) for d in dets] if w not in (9, 10) else [])          # two empty windows in a row
        _CACHE["scene", seed] = windows
    return _CACHE["scene", seed]


# ---------------------------------------------------------------------------------------------- kernel against the restatement
def test_empty_windows_and_the_first_birth():
    _check([[], [], []], _cfg(), 3)
    _check([[]], _cfg(), 1)
    want = _check([[(10, 10, 30, 30, 0.5, 6)]], _cfg(), 1)
    assert want[0].tolist() == [0] and want[2].tolist() == [1, 0] and want[1][0, :2].tolist() == [1, 0]
    _check([[], [(10, 10, 30, 30, 0.5, 6)], [], [], [], [(10, 10, 30, 30, 0.5, 6)]], _cfg(), 4)
    _check_track_rows([[], [(10, 10, 30, 30, 0.5, 6)], []], _cfg(), 2)
    from mm_distillnet_amd.tracker import track_rows
    assert track_rows(np.zeros((0, 6), np.float32), np.zeros(0, np.int32), 5, _cfg(), DEV).shape == (0,)


def test_more_objects_than_one_wave():
    cfg = _cfg(max_tracks=128)
    windows = [_grid(65), _grid(70, 1, 0), _grid(70, 2, 1), [], _grid(70, 4, 3)[::-1]]
    want = _check(windows, cfg, 2)
    assert want[0][:65].tolist() == list(range(65)) and want[0][65:135].tolist() == list(range(70))
    assert want[0][-70:].tolist() == list(range(70))[::-1] and want[2].tolist() == [70, 0]
    _check(windows, cfg, 5)
    _check_track_rows(windows, cfg, 3)


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


def test_a_window_with_257_detections():
    cfg = _cfg(max_tracks=256)
    many = _grid(257, cols=32, pitch=4, size=3)
    want = _check([many, many], cfg, 2, overflow=1)
    assert want[0][:257].tolist() == list(range(256)) + [-1] and want[0][257:].tolist() == list(range(256)) + [-1]
    _check([many[:256], many[:256]], cfg, 1)                 # exactly 256: no overflow
    from mm_distillnet_amd.tracker import track_rows
    with pytest.raises(RuntimeError, match="257 detections"):
        track_rows(*_record([many]), cfg, DEV)


@pytest.mark.parametrize("group", [1, 3, 8])
def test_random_scene_gives_the_same_bits_for_every_group_size(group):
    windows = _random_scene()
    cfg = _cfg()
    want = _check(windows, cfg, group)
    per_id = np.bincount(want[0][want[0] >= 0])
    assert len(windows) == 20 and want[2][0] > 12 and want[2][1] == 0 and (per_id >= 5).sum() >= 8      # births, deaths, long tracks
    assert (want[0] == -1).sum() == 0
    _check_track_rows(windows, cfg, group)
    _check(windows, _cfg(iou_min=0.5, beta=0.25, max_age=0, birth_score=0.5, max_tracks=16), group)


def test_padding_windows_bad_counts_and_rows_behind_the_counts_are_not_read():
    windows = _random_scene()[:11]                            # 11 windows in groups of 4: the last group has n_valid = 3
    cfg = _cfg()
    clean = _check(windows, cfg, 4)
    dirty = _check(windows, cfg, 4, dirty=True, fill=float("nan"))
    for a, b in zip(clean, dirty):
        np.testing.assert_array_equal(a, b)
    # every anchor of the student as cap_img (cand_cap = 0): NaN behind the few real rows changes nothing
    _check(windows[:4], cfg, 2, cap_img=49104, fill=float("nan"), dirty=True)
    # a window that fills cap_img, its count given as 1 << 30: clamped to cap_img
    full = [_grid(5), _grid(3, 1, 0), _grid(5, 2, 0)]
    _check(full, cfg, 2, cap_img=5, dirty=True, fill=float("nan"))


def test_a_zero_fill_resets_the_state():
    from mm_distillnet_amd.tracker import new_state
    windows = _random_scene()[:6]
    cfg = _cfg(max_tracks=32)
    rows, window, n = _record(windows)
    want = track_ref.track(rows, window, n, cfg)
    state = new_state(DEV, cfg)
    g = torch.Generator().manual_seed(3)
    for t in state:
        t.copy_(torch.randint(-2 ** 31, 2 ** 31 - 1, t.shape, generator=g, dtype=torch.int64).to(torch.int32))
    for t in state:
        t.zero_()
    ids, slots, glob = _direct(rows, window, n, cfg, 4, state=state)
    np.testing.assert_array_equal(ids[:len(rows)], want[0])
    np.testing.assert_array_equal(slots, want[1])
    np.testing.assert_array_equal(glob, want[2])
    # the same buffers again without a reset go on from that state: ids continue behind next_id
    on = track_ref.track(rows, window, n, cfg, want[1], want[2])
    ids2, slots2, glob2 = _direct(rows, window, n, cfg, 4, state=state)
    np.testing.assert_array_equal(ids2[:len(rows)], on[0])
    np.testing.assert_array_equal(slots2, on[1])
    np.testing.assert_array_equal(glob2, on[2])
    assert glob2[0] > glob[0]


# ---------------------------------------------------------------------------------------------- offsets: update, then append
@pytest.mark.parametrize("short", [0, 1])
def test_track_ids_land_on_the_rows_the_append_writes(short):
    from mm_distillnet_amd import _lib
    from mm_distillnet_amd.tracker import new_state
    cfg = _cfg()
    windows = [_grid(4), [], _grid(2, 1, 0), _grid(4, 2, 0), [], _grid(3, 3, 0), _grid(2, 4, 0)]      # 15 rows, groups of 3, 3, 1
    rows, window, n = _record(windows)
    want = track_ref.track(rows, window, n, cfg)
    B, cap_img, total = 3, 4, len(rows)
    rec_cap, alloc = total - short, total + 2
    rec_rows = torch.full((alloc, 6), float("nan"), device=DEV)
    rec_win = torch.full((alloc,), GUARD, dtype=torch.int32, device=DEV)
    rec_track = torch.full((alloc,), GUARD, dtype=torch.int32, device=DEV)
    rec_state = torch.zeros(2, dtype=torch.int32, device=DEV)
    state = new_state(DEV, cfg)
    for g0 in range(0, n, B):
        nv = min(B, n - g0)
        packed = np.full((B, cap_img, 6), np.nan, np.float32)
        cnt = np.full(B, 1 << 30, np.int32)
        for i in range(nv):
            sel = rows[window == g0 + i]
            packed[i, :len(sel)] = sel
            cnt[i] = len(sel)
        args = (torch.from_numpy(packed).to(DEV), torch.from_numpy(cnt).to(DEV), B, cap_img,
                torch.tensor([nv, g0], dtype=torch.int32, device=DEV))
        _lib.call("mmd_track_update", *args, rec_state[0:1], rec_cap, rec_track, state[0], state[1], cfg.max_tracks, cfg.iou_min,
                  cfg.beta, cfg.max_age, cfg.birth_score)
        _lib.call("mmd_det_record_append", *args, rec_rows, rec_win, rec_cap, rec_state[0:1], rec_state[1:2])
    torch.cuda.synchronize()
    assert rec_state.cpu().tolist() == [total, short]          # what the append alone leaves
    got_rows, got_win, got_track = rec_rows.cpu().numpy(), rec_win.cpu().numpy(), rec_track.cpu().numpy()
    np.testing.assert_array_equal(got_rows[:rec_cap].view(np.int32), rows[:rec_cap].view(np.int32))
    np.testing.assert_array_equal(got_win[:rec_cap], window[:rec_cap])
    np.testing.assert_array_equal(got_track[:rec_cap], want[0][:rec_cap])                 # rec_track[i] belongs to rec_rows[i]
    assert (got_track[rec_cap:] == GUARD).all() and (got_win[rec_cap:] == GUARD).all() and np.isnan(got_rows[rec_cap:]).all()
    np.testing.assert_array_equal(state[0].cpu().numpy(), want[1])                        # the row that did not fit was still tracked
    np.testing.assert_array_equal(state[1].cpu().numpy(), want[2])


# ---------------------------------------------------------------------------------------------- track_stream
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


def _detector(**kw):
    from mm_distillnet_amd.detector import AudioDetector
    spec, st = _state()
    det = AudioDetector(spec, DEV, image_size=S, **kw)
    det.load(st)
    return det


def _e2e(**kw):
    """256 slots: a random-weight student's boxes jump about, and every one that finds no partner holds a slot for max_age windows"""
    return _cfg(max_tracks=256, **kw)


def _e2e_for(seed):
    """recording 12 gives 116 .. 211 rows per window (the bias is tuned on recording 11: 17 .. 29): with max_age = 0 an unmatched track
    is freed before the births, so the live tracks are at most a window's rows and fit the 256 slots"""
    return _e2e(max_age=0) if seed == 12 else _e2e()


def _plain(seed):
    """detect_stream's record of a recording, from a detector that never tracked: (rows, window), and the restatement's ids on it"""
    if ("plain", seed) not in _CACHE:
        rows, window = _detector().detect_stream(_recording(seed).to(DEV), WIN, HOP, batch=BATCH)
        ids, _, glob = track_ref.track(rows, window, 7, _e2e_for(seed))
        print("recording %d: rows per window %s, tracks %d, overflow %d" % (seed, np.bincount(window, minlength=7).tolist(), glob[0], glob[1]))
        assert glob[1] == 0
        _CACHE["plain", seed] = (rows, window, ids)
    return _CACHE["plain", seed]


def _same(got, want):
    assert got[0].dtype == np.float32 and got[1].dtype == np.int32 and got[0].shape == want[0].shape
    np.testing.assert_array_equal(got[0].view(np.int32), want[0].view(np.int32))
    np.testing.assert_array_equal(got[1], want[1])
    if len(got) == 3:
        assert got[2].dtype == np.int32
        np.testing.assert_array_equal(got[2], want[2])


def test_track_stream_keeps_the_rows_and_gives_the_restatements_ids():
    from mm_distillnet_amd.tracker import tracks_table
    want = _plain(11)
    assert len(want[0]) > 0 and want[2].min() == 0 and want[2].max() >= 1
    table = tracks_table(want[1], want[2])
    print("tracks: %d, of them spanning more than one window: %d" % (len(table), int((table[:, 2] > table[:, 1]).sum())))
    det = _detector()
    w = _recording(11).to(DEV)
    got = det.track_stream(w, WIN, HOP, batch=BATCH, track=_e2e())
    assert len(got) == 3
    _same(got, want)
    assert det.stream_captures == 1 and det.stream_replays == 3
    _same(det.track_stream(w, WIN, HOP, batch=BATCH, track=_e2e()), want)                               # replayed: the state was reset
    assert det.stream_captures == 1 and det.stream_replays == 6
    # detect_stream on the same recording afterwards: its own graph, its 2-tuple, its bits - and back
    plain = det.detect_stream(w, WIN, HOP, batch=BATCH)
    assert len(plain) == 2 and det.stream_captures == 2
    _same(plain, want[:2])
    _same(det.track_stream(w, WIN, HOP, batch=BATCH, track=_e2e()), want)
    assert det.stream_captures == 3
    # other tracking parameters: captured anew, the restatement's ids for them
    tight = _e2e(iou_min=0.6, max_age=0)
    got = det.track_stream(w, WIN, HOP, batch=BATCH, track=tight)
    assert det.stream_captures == 4
    _same(got, want[:2] + (track_ref.track(want[0], want[1], 7, tight)[0],))
    # another recording in a new buffer: its own ids, from 0
    other = _plain(12)
    w2 = _recording(12).to(DEV)
    assert w2.data_ptr() != w.data_ptr()
    _same(det.track_stream(w2, WIN, HOP, batch=BATCH, track=_e2e_for(12)), other)
    assert other[2].min() == 0
    det.check_overflow()


def test_detect_stream_first_then_track_stream():
    want = _plain(11)
    det = _detector()
    w = _recording(11).to(DEV)
    plain = det.detect_stream(w, WIN, HOP, batch=BATCH)
    assert len(plain) == 2
    _same(plain, want[:2])
    _same(det.track_stream(w, WIN, HOP, batch=BATCH, track=_e2e()), want)
    assert det.stream_captures == 2
    # too few slots: the tracker's overflow is raised, naming the capacity
    with pytest.raises(RuntimeError, match="max_tracks = 1"):
        det.track_stream(w, WIN, HOP, batch=BATCH, track=_cfg(max_tracks=1))
    with pytest.raises(ValueError):
        det.track_stream(w, WIN, HOP, batch=BATCH, track=None)


def test_track_stream_without_a_graph_gives_the_same_ids():
    want = _plain(11)
    det = _detector()
    det.use_graph = False
    w = _recording(11).to(DEV)
    _same(det.track_stream(w, WIN, HOP, batch=BATCH, track=_e2e()), want)
    _same(det.track_stream(w, WIN, HOP, batch=BATCH, track=_e2e()), want)
    assert det.stream_captures == 0 and det.stream_replays == 0


def test_command_line_tool_writes_the_track_column(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    sys.path.insert(0, ROOT)
    import detect
    want = _plain(11)
    spec, st = _state()
    torch.save({"state_dict": st, "epoch": 3}, tmp_path / "student.pth")
    np.save(tmp_path / "rec.npy", _recording(11).numpy())
    cfgf = os.path.join(ROOT, "configs", "mm-distillnet.cfg")
    argv = ["--config_file", cfgf, "--checkpoint", str(tmp_path / "student.pth"), "--input", str(tmp_path / "rec.npy"),
            "--output", str(tmp_path / "out.csv"), "--overwrite", '{"image_size": %d}' % S,
            "--window_s", repr(WIN / 44100), "--hop_s", repr(HOP / 44100), "--batch", str(BATCH)]
    got = detect.main(argv + ["--track", "--track_max", "256"])
    assert len(got) == 3
    _same(got, want)
    n_tracks = len(np.unique(want[2][want[2] >= 0]))
    assert capsys.readouterr().out.strip().split("\n")[-1] == "7 windows, %d boxes, %d tracks -> %s" % (len(want[0]), n_tracks,
                                                                                                       tmp_path / "out.csv")
    lines = open(tmp_path / "out.csv").read().strip().split("\n")
    assert lines[0] == "window,t_start_s,x1,y1,x2,y2,score,label,track" and len(lines) == 1 + len(want[0])
    cells = [ln.split(",") for ln in lines[1:]]
    assert [int(c[0]) for c in cells] == want[1].tolist() and [int(c[8]) for c in cells] == want[2].tolist()
    rows = np.array([[float(v) for v in c[2:8]] for c in cells]).reshape(-1, 6).astype(np.float32)
    np.testing.assert_array_equal(rows.view(np.int32), want[0].view(np.int32))
    # the same invocation without --track: the 8-column file and the 2-tuple
    plain = detect.main(argv)
    assert len(plain) == 2
    _same(plain, want[:2])
    assert capsys.readouterr().out.strip().split("\n")[-1] == "7 windows, %d boxes -> %s" % (len(want[0]), tmp_path / "out.csv")
    lines = open(tmp_path / "out.csv").read().strip().split("\n")
    assert lines[0] == "window,t_start_s,x1,y1,x2,y2,score,label" and all(len(ln.split(",")) == 8 for ln in lines)
