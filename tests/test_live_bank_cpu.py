"""Live session bank, CPU side: audio.bank_schedule against a numpy simulation of the rings, the control row of a bank's chain, the C
ABI of the three bank entry points and detect.py's handling of several --input, all without a GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIN, HOP, BATCH, S = 4096, 1531, 3, 3
SPAN = (BATCH - 1) * HOP + WIN
LENGTHS = (19500, 14000, 9000)


def _audio():
    from mm_distillnet_amd import audio
    return audio


def _simulate(pushes, win, hop, batch, cap, n_sessions=S, check_rings=True):
    """pushes: (session, n) in order -> (ticks, the FIFO's length after every push).  The rings hold absolute sample indices (-1: never
    written); at every tick every slot a listed window reads must hold that window's sample, and every write is at most cap long"""
    a = _audio()
    rings = np.full((n_sessions, cap), -1, np.int64)
    state, ticks, fifo_len = a.bank_state(n_sessions), [], []
    for s, n in pushes:
        before = state[0][s]
        steps, state = a.bank_schedule(state, s, n, win, hop, batch, cap)
        assert state[0][s] == before + n
        at = before
        for st in steps:
            if st[0] == "write":
                _, q, lo, hi = st
                assert q == s and at <= lo < hi <= before + n and hi - lo <= cap
                rings[s, np.arange(lo, hi) % cap] = np.arange(lo, hi)
                at = hi
            else:
                assert st[0] == "run" and len(st[1]) == batch                     # a tick runs exactly when the FIFO reaches batch
                if check_rings:
                    for q, w in st[1]:
                        p = w * hop + np.arange(win)
                        assert (rings[q, p % cap] == p).all(), (q, w)
                ticks.append(list(st[1]))
        assert len(state[2]) < batch
        fifo_len.append(len(state[2]))
    return ticks, state


def _round_robin(lengths, chunk):
    at, pushes = [0] * len(lengths), []
    while any(a < n for a, n in zip(at, lengths)):
        for s, n in enumerate(lengths):
            if at[s] < n:
                c = min(chunk, n - at[s])
                pushes.append((s, c))
                at[s] += c
    return pushes


def _completion_order(pushes, win, hop, n_sessions=S):
    """the order in which windows complete, from the cumulative totals alone"""
    tot, nxt, order = [0] * n_sessions, [0] * n_sessions, []
    for s, n in pushes:
        tot[s] += n
        while nxt[s] * hop + win <= tot[s]:
            order.append((s, nxt[s]))
            nxt[s] += 1
    return order


@pytest.mark.parametrize("cap", [SPAN, 2 * SPAN])
@pytest.mark.parametrize("chunk", [1, 997, SPAN, 2 * SPAN + 123])
def test_every_tick_finds_its_samples_in_the_rings(chunk, cap):
    lengths = LENGTHS if chunk > 1 else (9000, 7200, 6000)                        # one sample at a time: shorter recordings
    pushes = _round_robin(lengths, chunk)
    ticks, state = _simulate(pushes, WIN, HOP, BATCH, cap)
    order = _completion_order(pushes, WIN, HOP)
    flat = [q for t in ticks for q in t]
    assert flat == order[:len(flat)] and list(state[2]) == order[len(flat):]      # the FIFO is in completion order
    assert len(ticks) == len(order) // BATCH and len(ticks) >= 3
    if chunk > cap:
        assert any(n > cap for _, n in pushes)                                    # a push longer than the ring


def test_windows_that_leave_gaps_skip_the_samples_between_them():
    win, hop, batch = 600, 1000, 2                                                # hop > win_len
    span = (batch - 1) * hop + win
    for cap in (span, 2 * span):
        for chunk in (1, 331, span, 3 * span + 7):
            pushes = _round_robin((7000, 5200), chunk)
            ticks, _ = _simulate(pushes, win, hop, batch, cap, n_sessions=2)
            assert [q for t in ticks for q in t] == _completion_order(pushes, win, hop, 2)[:batch * len(ticks)] and len(ticks) >= 4
    a = _audio()
    steps, _ = a.bank_schedule(a.bank_state(1), 0, 5000, win, hop, 1, win)
    written = sum(st[3] - st[2] for st in steps if st[0] == "write")
    assert written < 5000 and all(st[2] % hop < win for st in steps if st[0] == "write")      # no write starts in a gap


def test_splitting_pushes_leaves_the_ticks_unchanged():
    rng = np.random.default_rng(5)
    for trial in range(300):
        cap = int(rng.choice([SPAN, SPAN + 1, 2 * SPAN]))
        at, pushes = [0, 0, 0], []
        while any(a < n for a, n in zip(at, LENGTHS)):
            s = int(rng.choice([k for k in range(S) if at[k] < LENGTHS[k]]))
            n = min(int(rng.choice([1, 13, 1000, 1531, 4096, 9000])), LENGTHS[s] - at[s])
            pushes.append((s, n))
            at[s] += n
        pieces = []
        for s, n in pushes:
            cuts = sorted(set(rng.integers(1, n, size=int(rng.integers(0, 4))).tolist())) if n > 1 else []
            pieces += [(s, b - a) for a, b in zip([0] + cuts, cuts + [n])]
        assert sum(n for _, n in pieces) == sum(LENGTHS)
        ticks, state = _simulate(pushes, WIN, HOP, BATCH, cap, check_rings=trial < 40)
        ticks2, state2 = _simulate(pieces, WIN, HOP, BATCH, cap, check_rings=trial < 40)
        assert ticks == ticks2 and state == state2
        assert [q for t in ticks for q in t] + list(state[2]) == _completion_order(pushes, WIN, HOP)


def test_a_ring_below_the_span_raises():
    a = _audio()
    with pytest.raises(ValueError, match="shorter than one group"):
        a.bank_schedule(a.bank_state(S), 0, 10, WIN, HOP, BATCH, SPAN - 1)
    a.bank_schedule(a.bank_state(S), 0, 10, WIN, HOP, BATCH, SPAN)
    with pytest.raises(ValueError):
        a.bank_schedule(a.bank_state(S), S, 10, WIN, HOP, BATCH, SPAN)
    with pytest.raises(ValueError):
        a.bank_state(0)


def test_the_short_tick_and_a_reset():
    a = _audio()
    from mm_distillnet_amd.detector import _GroupChain
    state = a.bank_state(S)
    _, state = a.bank_schedule(state, 2, WIN + HOP, WIN, HOP, BATCH, SPAN)        # two windows of session 2: no tick yet
    assert state[2] == ((2, 0), (2, 1))
    steps, after = a.bank_step(state)
    assert steps == [("run", [(2, 0), (2, 1)])] and after[2] == () and after[:2] == state[:2]
    assert a.bank_step(after)[0] == []                                            # nothing waits: no tick
    row = _GroupChain.bank_control_table([steps[0][1]], BATCH, HOP)
    assert row[0, :BATCH].tolist() == [0, HOP, HOP]                               # padded by repeating the last window
    tail = row.view(np.int32)[0, 2 * BATCH:]
    assert tail.tolist() == [2, 2, 2, 0, 1, 1, 2, 0]                              # sess | win | {n_valid = the real windows, pad}
    # reset(2) of the state with the two windows queued: session 2 starts over, its queue is dropped, the others keep theirs
    _, state = a.bank_schedule(state, 0, WIN - 1, WIN, HOP, BATCH, SPAN)
    back = a.bank_reset(state, 2)
    assert back == ((WIN - 1, 0, 0), (0, 0, 0), ())
    steps, _ = a.bank_schedule(back, 2, WIN, WIN, HOP, BATCH, SPAN)
    assert steps == [("write", 2, 0, WIN)]


def test_control_row_lays_out_starts_sessions_windows_and_the_count():
    from mm_distillnet_amd.detector import _GroupChain
    ticks = [[(2, 5), (0, 1 << 21), (1, 0)], [(1, 7)]]
    t = _GroupChain.bank_control_table(ticks, 3, HOP)
    assert t.dtype == np.int64 and t.shape == (2, 7) and t.flags.c_contiguous
    assert t[0, :3].tolist() == [5 * HOP, (1 << 21) * HOP, 0] and (1 << 21) * HOP > 1 << 31       # int64 starts
    i32 = t.view(np.int32).reshape(2, 14)
    assert i32[0, 6:].tolist() == [2, 0, 1, 5, 1 << 21, 0, 3, 0]
    assert t[1, :3].tolist() == [7 * HOP] * 3 and i32[1, 6:].tolist() == [1, 1, 1, 7, 7, 7, 1, 0]
    out = np.full((4, 7), -1, np.int64)
    got = _GroupChain.bank_control_table(ticks, 3, HOP, out)
    assert np.shares_memory(got, out) and np.array_equal(got, t) and (out[2:] == -1).all()
    for bad in ([[]], [[(0, 0)] * 4]):
        with pytest.raises(ValueError):
            _GroupChain.bank_control_table(bad, 3, HOP)
    # today's control table keeps its layout
    old = _GroupChain.control_table([([0, 10], 4)], 3)
    assert old.shape == (1, 4) and old[0, :3].tolist() == [0, 10, 10] and old.view(np.int32)[0, 6:].tolist() == [2, 4]


def test_header_declares_the_three_bank_entry_points():
    from mm_distillnet_amd import _lib
    sigs = _lib.parse_header()
    assert len(sigs["mmd_melspec_windows_rings"]) == len(sigs["mmd_melspec_windows_ring"]) + 2
    assert len(sigs["mmd_track_update_bank"]) == len(sigs["mmd_track_update"]) + 3
    assert len(sigs["mmd_det_record_append_bank"]) == len(sigs["mmd_det_record_append"]) + 3
    if os.path.exists(_lib.LIB_PATH):
        dll = _lib.LIB.load()
        for name in ("mmd_melspec_windows_rings", "mmd_track_update_bank", "mmd_det_record_append_bank"):
            assert hasattr(dll, name)
        # refusals come before any launch: no device is needed for them
        assert dll.mmd_melspec_windows_rings(None, 1, 8, 8192, None, None, 1, 4096, None, None, None, 1, 0, None, None, None) == -22
        assert dll.mmd_track_update_bank(None, None, 1, 1, None, None, None, 1, None, 1, None, None, None, 1, 0.3, 0.5, 2, 0.0, None) == -22
        assert dll.mmd_det_record_append_bank(None, None, 1, 1, None, None, None, None, None, None, 1, None, None, None) == -22


# ---------------------------------------------------------------------------------------------- detect.py
BASE = ["--config_file", "f.cfg", "--checkpoint", "c.pth", "--output", "o.csv"]


def _detect():
    sys.path.insert(0, ROOT)
    import detect
    return detect


def test_one_input_parses_as_before():
    d = _detect()
    a = d.parse_args(BASE + ["--input", "rec.wav"])
    assert a.input == "rec.wav" and a.inputs == ["rec.wav"] and a.batch == 8 and a.chunk_s is None and a.window_s is None
    a = d.parse_args(BASE + ["--input", "rec.npy", "--window_s", "1", "--chunk_s", "0.1", "--batch", "4", "--track"])
    assert a.input == "rec.npy" and a.batch == 4 and a.chunk_s == 0.1 and a.track
    with pytest.raises(ValueError, match="needs --window_s"):
        d.parse_args(BASE + ["--input", "rec.wav", "--chunk_s", "0.1"])
    with pytest.raises(SystemExit):
        d.parse_args(BASE)


def test_several_inputs_make_a_bank_or_are_refused():
    d = _detect()
    three = ["--input", "a.wav", "--input", "b.npy", "--input", "c.wav"]
    a = d.parse_args(BASE + three + ["--window_s", "1", "--hop_s", "0.1", "--chunk_s", "0.1"])
    assert a.inputs == ["a.wav", "b.npy", "c.wav"] and a.batch is None            # the bank: the number of files
    assert d.parse_args(BASE + three + ["--window_s", "1", "--chunk_s", "0.1", "--batch", "2", "--track"]).batch == 2
    for extra, what in ((["--window_s", "1"], "--window_s and --chunk_s"), (["--chunk_s", "0.1"], "--window_s and --chunk_s"),
                        ([], "--window_s and --chunk_s"),
                        (["--window_s", "1", "--chunk_s", "0.1", "--resample"], "44.1 kHz input only"),
                        (["--window_s", "1", "--chunk_s", "0.1", "--sample_rate", "48000"], "44.1 kHz input only"),
                        (["--window_s", "1", "--live_s", "0.1"], "--window_s and --chunk_s"),
                        (["--window_s", "1", "--chunk_s", "0.1", "--live_s", "0.1"], "44.1 kHz input only"),
                        (["--window_s", "1", "--chunk_s", "0"], "positive number of seconds")):
        with pytest.raises(ValueError, match=what):
            d.parse_args(BASE + three + extra)
    with pytest.raises(ValueError, match="c.mp3: unsupported input"):
        d.parse_args(BASE + ["--input", "a.wav", "--input", "c.mp3", "--window_s", "1", "--chunk_s", "0.1"])
    assert d.BANK_COLUMNS == ("session", "window", "t_start_s", "x1", "y1", "x2", "y2", "score", "label")


def test_bank_csv_has_the_session_column(tmp_path):
    d = _detect()
    rows = np.arange(12, dtype=np.float32).reshape(2, 6) / 7
    n = d.write_windows_csv(str(tmp_path / "b.csv"), rows, np.array([5, 1], np.int32), HOP, np.array([3, -1], np.int32), np.array([2, 0], np.int32))
    lines = open(tmp_path / "b.csv").read().splitlines()
    assert n == 2 and lines[0] == "session,window,t_start_s,x1,y1,x2,y2,score,label,track"
    assert lines[1].startswith("2,5,%.9g," % (5 * HOP / 44100)) and lines[1].endswith(",3") and lines[2].startswith("0,1,")
    d.write_windows_csv(str(tmp_path / "c.csv"), rows, np.array([5, 1], np.int32), HOP, session=np.array([2, 0], np.int32))
    assert open(tmp_path / "c.csv").read().splitlines()[0] == "session,window,t_start_s,x1,y1,x2,y2,score,label"
