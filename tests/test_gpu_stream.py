"""Streaming detection on the GPU: the windowed front end (mmd_melspec_windows) against mmd_melspec_batch on the materialised slices, bit
for bit; the device detection record (mmd_det_record_append) against numpy; AudioDetector.detect_stream and detect.py --window_s against
detect() on the same groups of slices, bit for bit.  The small detector is the one of tests/test_gpu_detector.py (D2 at 128 x 128, the
audio student of test_net_eval_golden), its classifier bias tuned on this file's recording."""
import os
import sys

import numpy as np
import pytest
import torch

from helpers import make_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, COEF, C = 128, 2, 8
N_TOTAL, WIN = 16000, 4096
STARTS = [0, 1531, 3062, 11904]           # hop 1531: no multiple of 256 or 4; first window at the start, last one ends at n_total
_CACHE = {}


def _noise(n, seed):
    """white noise: neighbouring samples differ everywhere, so a reflection that reads the wrong neighbour changes bits"""
    return torch.randn(C, n, generator=torch.Generator().manual_seed(seed)) * 0.3


def _bits(t):
    return t.contiguous().view(torch.int32)


def _front():
    from mm_distillnet_amd.audio import MelFrontEnd
    if "front" not in _CACHE:
        _CACHE["front"] = MelFrontEnd(DEV)
    return _CACHE["front"]


def _windows(wav, starts, win_len, db, out=None, ws=None):
    f = _front()
    B = len(starts)
    if out is None:
        out = torch.full((B, f.n_mels, f.n_frames(win_len), C), float("nan"), device=DEV)
        ws = torch.full((B * C,), -1, dtype=torch.int32, device=DEV)          # 0xFFFFFFFF
    f.melspec_windows_into(wav, torch.tensor(starts, dtype=torch.int64, device=DEV), win_len, db, ws, out)
    return out, ws


def _stacked(wav, starts, win_len, db):
    stack = torch.stack([wav[:, s:s + win_len] for s in starts]).contiguous()
    return _front().melspec(stack, None, db)


# ---------------------------------------------------------------------------------------------- front end
@pytest.mark.parametrize("db", [False, True])
def test_windows_equal_the_batch_entry_point_on_the_slices(db):
    wav = _noise(N_TOTAL, 1).to(DEV)
    assert STARTS[-1] + WIN == N_TOTAL and _front().n_frames(WIN) == 17          # the third 8-frame block is partly masked
    want = _stacked(wav, STARTS, WIN, db)
    out, ws = _windows(wav, STARTS, WIN, db)
    assert out.shape == want.shape == (4, 80, 17, C) and not torch.isnan(out).any()
    assert torch.equal(_bits(out), _bits(want))
    if db:
        assert float(out.max()) == 0.0 and float(out.min()) >= -80.0
        for b in range(4):
            for c in range(C):
                assert float(out[b, :, :, c].max()) == 0.0                        # one maximum per (window, channel)
    first = out.clone()
    _windows(wav, STARTS, WIN, db, out, ws)                                       # dirty buffers: the previous run's contents
    assert torch.equal(_bits(out), _bits(first))
    assert not torch.equal(out[0], out[1])


@pytest.mark.parametrize("db", [False, True])
def test_shortest_windows_at_both_ends_of_the_recording(db):
    wav = _noise(N_TOTAL, 2).to(DEV)
    win = 513 + 256                                                               # reflection covers most of a frame
    for start in (0, N_TOTAL - win):
        out, _ = _windows(wav, [start], win, db)
        assert out.shape == (1, 80, 4, C)
        assert torch.equal(_bits(out), _bits(_stacked(wav, [start], win, db)))


@pytest.mark.parametrize("db", [False, True])
def test_nothing_outside_the_window_is_read(db):
    """NaN guard bands around the recording and NaN over every sample outside one interior window: the window's output keeps the clean
    run's bits, so no read left the window (every read lands in allocated memory either way)."""
    clean = _noise(N_TOTAL, 3)
    start = 3062
    want, _ = _windows(clean.to(DEV), [start], WIN, db)
    buf = torch.full((1024 + C * N_TOTAL + 1024,), float("nan"))
    masked = torch.full_like(clean, float("nan"))
    masked[:, start:start + WIN] = clean[:, start:start + WIN]
    buf[1024:1024 + C * N_TOTAL] = masked.reshape(-1)
    buf = buf.to(DEV)
    wav = buf[1024:1024 + C * N_TOTAL].view(C, N_TOTAL)
    assert wav.is_contiguous() and torch.isnan(wav[:, start - 1]).all() and torch.isnan(wav[:, start + WIN]).all()
    out, _ = _windows(wav, [start], WIN, db)
    assert not torch.isnan(out).any()
    assert torch.equal(_bits(out), _bits(want))
    # the windows that touch the recording's two ends, with the guard bands right beside them
    buf2 = torch.full((1024 + C * N_TOTAL + 1024,), float("nan"))
    buf2[1024:1024 + C * N_TOTAL] = clean.reshape(-1)
    wav2 = buf2.to(DEV)[1024:1024 + C * N_TOTAL].view(C, N_TOTAL)
    ends = [0, N_TOTAL - WIN]
    out2, _ = _windows(wav2, ends, WIN, db)
    assert torch.equal(_bits(out2), _bits(_stacked(clean.to(DEV), ends, WIN, db)))


# ---------------------------------------------------------------------------------------------- record kernel
def _append_ref(rec_rows, rec_win, count, rows, cnt, n_valid, first, rec_cap):
    for i in range(n_valid):
        for j in range(cnt[i]):
            if count < rec_cap:
                rec_rows[count] = rows[i, j]
                rec_win[count] = first + i
            count += 1
    return count


@pytest.mark.parametrize("case", ["exact", "one_short", "garbage_behind_n_valid"])
def test_record_append_against_numpy(case):
    from mm_distillnet_amd import _lib
    B, cap_img, counts = 3, 4, [4, 0, 2]
    rng = np.random.default_rng(5)
    rows = [rng.standard_normal((B, cap_img, 6)).astype(np.float32) for _ in range(2)]
    calls = [(3, 0, list(counts)), (2, 3, list(counts))]                          # (n_valid, first_window, counts): 6 + 4 rows
    if case == "garbage_behind_n_valid":
        calls[1] = (2, 3, [4, 0, 1 << 30])
        calls.append((1, 9, [2, -7, 1 << 30]))                                    # 2 more rows
        calls.append((0, 11, [1 << 30, -1, 5]))                                   # nothing
    total = 12 if case == "garbage_behind_n_valid" else 10
    rec_cap = total - 1 if case == "one_short" else total
    alloc = rec_cap + 2                                                           # two rows behind the capacity: must stay untouched

    def run():
        rec_rows = torch.full((alloc, 6), float("nan"), device=DEV)
        rec_win = torch.full((alloc,), -77, dtype=torch.int32, device=DEV)
        state = torch.zeros(2, dtype=torch.int32, device=DEV)
        for k, (nv, first, cn) in enumerate(calls):
            _lib.call("mmd_det_record_append", torch.from_numpy(rows[k % 2]).to(DEV), torch.tensor(cn, dtype=torch.int32, device=DEV), B,
                      cap_img, torch.tensor([nv, first], dtype=torch.int32, device=DEV), rec_rows, rec_win, rec_cap, state[0:1], state[1:2])
        torch.cuda.synchronize()
        return rec_rows.cpu().numpy(), rec_win.cpu().numpy(), state.cpu().tolist()

    want_rows = np.full((alloc, 6), np.nan, np.float32)
    want_win = np.full(alloc, -77, np.int32)
    count = 0
    for k, (nv, first, cn) in enumerate(calls):
        count = _append_ref(want_rows, want_win, count, rows[k % 2], cn, nv, first, rec_cap)
    assert count == total
    got_rows, got_win, (got_count, got_over) = run()
    assert got_count == total                                                     # the true total, also behind the capacity
    assert got_over == (1 if case == "one_short" else 0)
    np.testing.assert_array_equal(got_rows.view(np.int32), want_rows.view(np.int32))      # order, and the NaN tail untouched
    np.testing.assert_array_equal(got_win, want_win)
    assert np.isnan(got_rows[rec_cap:]).all() and (got_win[rec_cap:] == -77).all()
    assert got_win[:6].tolist() == [0, 0, 0, 0, 2, 2]
    again_rows, again_win, again_state = run()
    np.testing.assert_array_equal(again_rows.view(np.int32), got_rows.view(np.int32))
    np.testing.assert_array_equal(again_win, got_win)
    assert again_state == [got_count, got_over]


# ---------------------------------------------------------------------------------------------- detect_stream
HOP, BATCH, N_REC = 1531, 3, 14000        # W = 1 + (14000 - 4096) // 1531 = 7: two full groups, one of one window; a tail is dropped


def _recording(seed):
    """the detector tests' stand-in recording (tones, a chirp and a noise floor drawn from a torch.Generator: neighbouring samples differ
    everywhere), so the random-weight student stays in the regime those tests keep it in.  (On white noise alone its head saturates -
    scores of exactly 1.0 and boxes of 1e5 pixels by the thousand - which is no detection workload.)"""
    from mm_distillnet_amd.data import synthetic_waveforms
    return synthetic_waveforms(24, seed, N_REC)


def _state():
    """(spec, state) of tests/test_gpu_detector.py's small student, its classifier bias shifted so that the dB maps of the
    recording's windows give detections at the default confidence threshold (as that file tunes it on its own inputs: about 40
    candidates per image over the seven windows the tests slide over)"""
    if "state" not in _CACHE:
        from mm_distillnet_amd.synth import tune_teacher_bias
        spec, st = make_state(COEF, 8, 13, "audio")
        w = _recording(11)
        x = _front().student_input(torch.stack([w[:, k * HOP:k * HOP + WIN] for k in range(7)]).to(DEV), None, S, db=True).cpu()
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


def _oracle(seed):
    """detect() on the materialised slices in the same groups, the last padded by repeating its last window, the padding dropped:
    (rows [R, 6], window [R]), computed once per recording"""
    if ("oracle", seed) not in _CACHE:
        from mm_distillnet_amd.audio import stream_window_starts
        w = _recording(seed).to(DEV)
        starts = stream_window_starts(N_REC, WIN, HOP)
        assert len(starts) == 7
        det = _detector()
        rows, win = [], []
        for g0 in range(0, len(starts), BATCH):
            real = starts[g0:g0 + BATCH]
            padded = real + [real[-1]] * (BATCH - len(real))
            got = det.detect(torch.stack([w[:, s:s + WIN] for s in padded]).contiguous())
            for i in range(len(real)):
                rows.append(got[i])
                win += [g0 + i] * len(got[i])
        det.check_overflow()
        _CACHE["oracle", seed] = (np.concatenate(rows).astype(np.float32).reshape(-1, 6), np.asarray(win, np.int32))
    return _CACHE["oracle", seed]


def _same(got, want):
    rows, win = got
    assert rows.dtype == np.float32 and win.dtype == np.int32 and rows.shape == want[0].shape and win.shape == want[1].shape
    np.testing.assert_array_equal(rows.view(np.int32), want[0].view(np.int32))
    np.testing.assert_array_equal(win, want[1])


def test_detect_on_waveforms_keeps_its_bits_over_many_replays():
    """the oracle of the tests below: detect() replays its waveform graph once per group, so later replays must give the eager run's
    rows (the maxima workspace of the dB step has to be cleared inside every replay)"""
    w = _recording(11).to(DEV)
    clips = [torch.stack([w[:, k * HOP:k * HOP + WIN] for k in ks]).contiguous() for ks in ((4, 5, 6), (0, 1, 2))]
    want = [_detector().detect(c) for c in clips]
    assert sum(len(r) for r in want[0]) > 0 and sum(len(r) for r in want[1]) > 0
    det = _detector()
    for k in range(5):
        got = det.detect(clips[k % 2])
        for a, b in zip(got, want[k % 2]):
            assert a.shape == b.shape, (k, a.shape, b.shape)
            np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32))
    assert det.graph_replays == 4


def test_stream_rows_equal_detect_on_the_same_groups():
    want = _oracle(11)
    print("rows per window:", np.bincount(want[1], minlength=7).tolist())
    per_window = np.bincount(want[1], minlength=7)
    assert (per_window >= 1).sum() >= 5 and per_window[6] >= 1 and per_window.max() <= 100      # most windows give rows, the padded group's
    # one too; no window beyond the 100 rows the detector tests keep their images under
    det = _detector()
    w = _recording(11).to(DEV)
    _same(det.detect_stream(w, WIN, HOP, batch=BATCH), want)
    assert det.stream_captures == 1 and det.stream_replays == 3
    # the same recording again: replayed, no new capture, the same bits
    _same(det.detect_stream(w, WIN, HOP, batch=BATCH), want)
    assert det.stream_captures == 1 and det.stream_replays == 6
    # another recording of the same length in a new buffer: its own rows, not the first one's through a stale address
    other = _oracle(12)
    assert other[0].shape != want[0].shape or not np.array_equal(other[0], want[0])
    w2 = _recording(12).to(DEV)
    assert w2.data_ptr() != w.data_ptr()
    _same(det.detect_stream(w2, WIN, HOP, batch=BATCH), other)
    assert det.stream_captures == 2
    _same(det.detect_stream(w, WIN, HOP, batch=BATCH), want)
    det.check_overflow()


def test_stream_without_a_graph_runs_the_same_chain():
    want = _oracle(11)
    det = _detector()
    det.use_graph = False
    w = _recording(11).to(DEV)
    _same(det.detect_stream(w, WIN, HOP, batch=BATCH), want)
    _same(det.detect_stream(w, WIN, HOP, batch=BATCH), want)
    assert det.stream_captures == 0 and det.stream_replays == 0
    det.use_graph = True                                                          # the buffers are there: capture, then replay
    _same(det.detect_stream(w, WIN, HOP, batch=BATCH), want)
    assert det.stream_captures == 1 and det.stream_replays == 3


def test_full_record_raises_with_the_rows_needed():
    want = _oracle(11)
    R = len(want[0])
    det = _detector()
    w = _recording(11).to(DEV)
    with pytest.raises(RuntimeError, match="%d rows needed, rec_cap = %d" % (R, R - 1)):
        det.detect_stream(w, WIN, HOP, batch=BATCH, rec_cap=R - 1)
    _same(det.detect_stream(w, WIN, HOP, batch=BATCH, rec_cap=R), want)           # exactly enough
    with pytest.raises(ValueError):
        det.detect_stream(w[None], WIN, HOP)
    with pytest.raises(ValueError):
        det.detect_stream(w, 512, HOP)
    with pytest.raises(ValueError):
        det.detect_stream(w, WIN, 0)
    with pytest.raises(ValueError):
        det.detect_stream(w[:, :WIN - 1].contiguous(), WIN, HOP)


def test_command_line_tool_writes_the_rows_of_detect_stream(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    sys.path.insert(0, ROOT)
    import detect
    want = _oracle(11)
    spec, st = _state()
    torch.save({"state_dict": st, "epoch": 3}, tmp_path / "student.pth")
    np.save(tmp_path / "rec.npy", _recording(11).numpy())
    cfgf = os.path.join(ROOT, "configs", "mm-distillnet.cfg")
    rows, window = detect.main(["--config_file", cfgf, "--checkpoint", str(tmp_path / "student.pth"), "--input", str(tmp_path / "rec.npy"),
                                "--output", str(tmp_path / "out.csv"), "--overwrite", '{"image_size": %d}' % S,
                                "--window_s", repr(WIN / 44100), "--hop_s", repr(HOP / 44100), "--batch", str(BATCH)])
    _same((rows, window), want)
    assert capsys.readouterr().out.strip().split("\n")[-1] == "7 windows, %d boxes -> %s" % (len(want[0]), tmp_path / "out.csv")
    lines = open(tmp_path / "out.csv").read().strip().split("\n")
    assert lines[0] == "window,t_start_s,x1,y1,x2,y2,score,label" and len(lines) == 1 + len(want[0])
    cells = [ln.split(",") for ln in lines[1:]]
    assert [int(c[0]) for c in cells] == want[1].tolist()
    assert [c[1] for c in cells] == ["%.9g" % (int(w) * HOP / 44100) for w in want[1]]
    got = np.array([[float(v) for v in c[2:]] for c in cells]).reshape(-1, 6).astype(np.float32)
    np.testing.assert_array_equal(got.view(np.int32), want[0].view(np.int32))
