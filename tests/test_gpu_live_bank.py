"""Live session bank on the GPU, end to end: three recordings pushed side by side through AudioDetector.open_bank - every tick against
`detect` on the stack of its windows, every session's track ids against `tracker.track_rows` on its own rows, the ticks and the bytes
against another cutting of the same pushes and against the eager chain - and detect.py with three WAVs."""
import os
import sys
import wave

import numpy as np
import pytest
import torch

from helpers import make_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, COEF, C = 128, 2, 8
WIN, HOP, BATCH, NS = 4096, 1531, 3, 3
SPAN = (BATCH - 1) * HOP + WIN
SEEDS, LENGTHS = (3, 11, 7), (19500, 14000, 9000)        # 11, 7 and 4 windows: seven full ticks and one window for flush()
N_WIN = tuple(1 + (n - WIN) // HOP for n in LENGTHS)
PLAN_SEED = 2
_CACHE = {}


def _quantised(k, seed=None):
    """recording k -> (int16 [C, n], float32 int16 / 2^15): what push_pcm decodes and what push takes are the same samples"""
    from mm_distillnet_amd.data import synthetic_waveforms
    key = ("rec", k, seed)
    if key not in _CACHE:
        w = synthetic_waveforms(24, SEEDS[k] if seed is None else seed, LENGTHS[k])
        q = torch.clamp(torch.round(w * 32767.0), -32768, 32767).to(torch.int16)
        _CACHE[key] = (q, q.to(torch.float32) / 32768.0)
    return _CACHE[key]


def _state():
    """tests/test_gpu_stream.py's student: make_state's D2 audio net, the classifier bias tuned on the seven windows of recording 11 at
    14 000 samples (session 1's); recordings 3 and 7 at their lengths answer it in the same regime, some 20 to 40 rows per window (the
    response of `synthetic_waveforms` to one bias differs widely between seeds: others give none, or hundreds)"""
    if "state" not in _CACHE:
        from mm_distillnet_amd.audio import MelFrontEnd
        from mm_distillnet_amd.synth import tune_teacher_bias
        spec, st = make_state(COEF, 8, 13, "audio")
        wins = torch.stack([_quantised(1)[1][:, w * HOP:w * HOP + WIN] for w in range(7)])
        tune_teacher_bias(spec, st, MelFrontEnd(DEV).student_input(wins.to(DEV), None, S, db=True).cpu(), DEV, 40)
        _CACHE["state"] = (spec, st)
    spec, st = _CACHE["state"]
    return spec, {k: v.clone() for k, v in st.items()}


def _detector(**kw):
    from mm_distillnet_amd.detector import AudioDetector
    spec, st = _state()
    det = AudioDetector(spec, DEV, image_size=S, **kw)
    det.load(st)
    return det


def _track_config():
    from mm_distillnet_amd.tracker import TrackConfig
    return TrackConfig(max_tracks=256)


def _plan():
    """The seeded interleaving: (session, samples) per push, mixed sizes from one sample to more than a ring's span.  Checked on the
    host schedule, before any device work: the ticks it gives are the ones the tests below need."""
    if "plan" not in _CACHE:
        from mm_distillnet_amd.audio import bank_schedule, bank_state
        rng = np.random.default_rng(PLAN_SEED)
        at, pushes = [0] * NS, []
        while any(a < n for a, n in zip(at, LENGTHS)):
            s = int(rng.choice([k for k in range(NS) if at[k] < LENGTHS[k]]))
            n = min(int(rng.choice([1, 500, 1000, 1531, 2500, 4096, 8000])), LENGTHS[s] - at[s])
            pushes.append((s, n))
            at[s] += n
        state, ticks, most = bank_state(NS), [], 0
        for s, n in pushes:
            steps, state = bank_schedule(state, s, n, WIN, HOP, BATCH, 2 * SPAN)
            runs = [st[1] for st in steps if st[0] == "run"]
            ticks += runs
            most = max(most, len(runs))
        assert len(ticks) == 7 and len(state[2]) == 1                             # flush() will run a short tick of one window
        assert any(len({q for q, _ in t}) == 3 for t in ticks)                    # a tick mixing the three sessions
        assert any([q for q, _ in t].count(s) >= 2 for t in ticks for s in range(NS))      # a session with two windows in one tick
        assert most >= 2 and any(n > SPAN for _, n in pushes) and any(n == 1 for _, n in pushes)
        _CACHE["plan"] = (pushes, ticks + [list(state[2])])
    return _CACHE["plan"]


def _push(bank, s, k, lo, hi):
    """samples lo .. hi-1 of session s in the k-th argument form: numpy, host tensor, device tensor (a column slice), PCM bytes"""
    q, w = _quantised(s)
    if k % 4 == 0:
        return bank.push(s, w[:, lo:hi].numpy())
    if k % 4 == 1:
        return bank.push(s, w[:, lo:hi])
    if k % 4 == 2:
        return bank.push(s, w.to(DEV)[:, lo:hi])
    return bank.push_pcm(s, np.ascontiguousarray(q[:, lo:hi].numpy().T).astype("<i2").tobytes(), 2)


def _run(det, pushes, tracked=True, ring_len=None):
    """the whole run on a fresh bank of det -> (result, ticks)"""
    bank = det.open_bank(NS, WIN, HOP, track=_track_config() if tracked else None, ring_len=ring_len)
    assert bank.batch == NS and bank.ring_len == (2 * SPAN if ring_len is None else ring_len)
    at, parts = [0] * NS, []
    for k, (s, n) in enumerate(pushes):
        parts.append(_push(bank, s, k, at[s], at[s] + n))
        at[s] += n
    assert list(at) == list(LENGTHS) and len(bank.ticks) == 7
    last = bank.flush()
    assert len(bank.ticks) == 8 and len(bank.ticks[7]) == 1                       # the short tick comes from flush() alone
    assert all(len(x) == 0 for x in bank.flush())
    got, ticks = bank.concat(parts + [last]), [list(t) for t in bank.ticks]
    with pytest.raises(RuntimeError, match="flushed"):
        bank.push(0, _quantised(0)[1][:, :10])
    bank.close()
    with pytest.raises(RuntimeError, match="closed"):
        bank.step()
    return got, ticks


def _main_run():
    if "main" not in _CACHE:
        det = _detector()
        got, ticks = _run(det, _plan()[0])
        assert det.bank_captures == 1 and det.bank_replays == len(ticks) == 8
        assert det.live_captures == 0 and det.stream_captures == 0
        _CACHE["main"] = (got, ticks)
    return _CACHE["main"]


def _same(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
        np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32))


def test_every_tick_equals_detect_on_the_stack_of_its_windows():
    got, ticks = _main_run()
    assert ticks == _plan()[1]
    rows, session, window, track = got
    assert rows.dtype == np.float32 and rows.shape[1:] == (6,) and all(x.dtype == np.int32 and x.shape == (len(rows),) for x in got[1:])
    oracle = _detector()                                                          # never the detector the bank ran on
    want_rows, want_sess, want_win = [], [], []
    for t in ticks:
        full = t + [t[-1]] * (BATCH - len(t))                                     # a short tick is padded by repetition
        stack = torch.stack([_quantised(s)[1][:, w * HOP:w * HOP + WIN] for s, w in full]).to(DEV)
        per_image = oracle.detect(stack)
        print("tick", t, "rows", [len(r) for r in per_image])
        for (s, w), r in zip(t, per_image):                                       # only the real windows are recorded
            want_rows.append(r)
            want_sess += [s] * len(r)
            want_win += [w] * len(r)
    _same(got[:3], (np.concatenate(want_rows), np.asarray(want_sess, np.int32), np.asarray(want_win, np.int32)))
    per_session = np.bincount(session, minlength=NS)
    assert (per_session >= 1).all() and len(rows) >= 10                           # every session returns rows
    for s in range(NS):                                                           # window indices count within the session's recording
        assert set(window[session == s].tolist()) <= set(range(N_WIN[s]))


def test_each_sessions_tracks_equal_track_rows_on_its_own_rows():
    from mm_distillnet_amd.tracker import track_rows
    rows, session, window, track = _main_run()[0]
    longest = 0
    for s in range(NS):
        m = session == s
        want = track_rows(rows[m], window[m], N_WIN[s], _track_config(), DEV)
        np.testing.assert_array_equal(track[m], want)
        ids = track[m][track[m] >= 0]
        if len(ids):
            assert ids.min() == 0                                                 # ids count per session from 0
            longest = max(longest, int(np.bincount(ids).max()))
    assert longest >= 2                                                           # a track of two or more hits


def test_another_cutting_of_the_same_pushes_gives_the_same_ticks_and_bytes():
    want, ticks = _main_run()
    rng = np.random.default_rng(8)
    pieces = []
    for s, n in _plan()[0]:
        cuts = sorted(set(rng.integers(1, n, size=int(rng.integers(1, 4))).tolist())) if n > 1 else []
        pieces += [(s, b - a) for a, b in zip([0] + cuts, cuts + [n])]
    assert len(pieces) > len(_plan()[0])
    det = _detector()
    got, ticks2 = _run(det, pieces, ring_len=SPAN)                                # and in rings of exactly one span
    assert ticks2 == ticks
    _same(got, want)
    assert det.bank_captures == 1 and det.bank_replays == 8


def test_bank_without_a_graph_and_without_a_tracker():
    want, ticks = _main_run()
    det = _detector()
    det.use_graph = False
    got, ticks2 = _run(det, _plan()[0])
    assert ticks2 == ticks and det.bank_captures == 0 and det.bank_replays == 0
    _same(got, want)
    det.use_graph = True
    plain, ticks3 = _run(det, _plan()[0], tracked=False)                          # three columns, the same rows
    assert ticks3 == ticks and len(plain) == 3 and det.bank_captures == 1
    _same(plain, want[:3])


def test_reset_restarts_one_session_and_leaves_the_others_alone():
    """sessions 0 and 2 run on while session 1 gets a second recording behind reset(1): their results are those of a run in which session
    1's pushes never happened - checked through the contract: every tick against detect, every session's ids against track_rows"""
    from mm_distillnet_amd.tracker import track_rows
    det = _detector()
    bank = det.open_bank(NS, WIN, HOP, track=_track_config())
    w = [_quantised(k)[1].to(DEV) for k in range(NS)]
    other = _quantised(1, seed=SEEDS[0])[1].to(DEV)                               # session 1's second recording: other audio
    parts = [bank.push(0, w[0][:, :6000]), bank.push(1, w[1][:, :8000]), bank.push(2, w[2][:, :4000])]
    assert bank.ticks == [[(0, 0), (0, 1), (1, 0)]] and bank.state[2] == ((1, 1), (1, 2))
    queued = [q for q in bank.state[2] if q[0] == 1]
    bank.reset(1)
    assert bank.state[0][1] == 0 and bank.state[1][1] == 0 and not any(q[0] == 1 for q in bank.state[2])
    assert bank.state[0][0] == 6000 and bank.state[0][2] == 4000
    first = bank.concat(parts)
    parts = [bank.push(1, other[:, :9000]), bank.push(0, w[0][:, 6000:12000]), bank.push(2, w[2][:, 4000:]), bank.flush()]
    second = bank.concat(parts)
    assert len(queued) == 2 and len(second[0]) >= 1 and len(bank.ticks) == 5
    ticks = [list(t) for t in bank.ticks]
    bank.close()
    oracle = _detector()
    # the ticks behind the reset: session 1's windows start at 0 again and read the SECOND recording
    k0, at = 1, 0
    assert min(wdx for t in ticks[k0:] for q, wdx in t if q == 1) == 0
    for t in ticks[k0:]:
        full = t + [t[-1]] * (BATCH - len(t))
        src = {0: w[0], 1: other, 2: w[2]}
        per_image = oracle.detect(torch.stack([src[q][:, wdx * HOP:wdx * HOP + WIN] for q, wdx in full]))
        for (q, wdx), r in zip(t, per_image):
            n = len(r)
            np.testing.assert_array_equal(second[0][at:at + n].view(np.int32), r.view(np.int32))
            assert (second[1][at:at + n] == q).all() and (second[2][at:at + n] == wdx).all()
            at += n
    assert at == len(second[0])
    both = tuple(np.concatenate([a, b]) for a, b in zip(first, second))
    for s in (0, 2):                                                              # undisturbed: one recording, one tracker, across the reset
        m = both[1] == s
        n_win = 1 + max(wdx for t in ticks for q, wdx in t if q == s)
        np.testing.assert_array_equal(both[3][m], track_rows(both[0][m], both[2][m], n_win, _track_config(), DEV))
    m = second[1] == 1                                                            # session 1: ids from 0 again, on the second recording alone
    n_win = 1 + max(wdx for t in ticks[k0:] for q, wdx in t if q == 1)
    np.testing.assert_array_equal(second[3][m], track_rows(second[0][m], second[2][m], n_win, _track_config(), DEV))


def test_one_stream_session_or_bank_at_a_time_and_a_record_too_small():
    det = _detector()
    bank = det.open_bank(NS, WIN, HOP)
    session = det.open_stream(WIN, HOP, batch=BATCH)
    assert bank.closed and det._held is session
    with pytest.raises(RuntimeError, match="closed"):
        bank.push(0, _quantised(0)[1][:, :100])
    bank = det.open_bank(NS, WIN, HOP, batch=2)
    assert session.closed and det._held is bank and bank.batch == 2
    with pytest.raises(RuntimeError, match="closed"):
        session.push(_quantised(0)[1][:, :100])
    with pytest.raises(ValueError, match="session 3"):
        bank.push(3, _quantised(0)[1][:, :100])
    det.detect_stream(_quantised(0)[1].to(DEV), WIN, HOP, batch=BATCH)
    assert bank.closed and det._held is None
    with pytest.raises(ValueError, match="ring_len = %d is shorter" % (SPAN - 1)):
        det.open_bank(NS, WIN, HOP, ring_len=SPAN - 1)
    with pytest.raises(ValueError, match="n_sessions"):
        det.open_bank(0, WIN, HOP)
    # a record of one row per window: a first window with several rows needs more, and the error says how many
    rows = _main_run()[0]
    first = [int(((rows[1] == s) & (rows[2] == 0)).sum()) for s in range(NS)]
    busiest = int(np.argmax(first))
    assert first[busiest] >= 3
    det.STREAM_ROWS_PER_WINDOW = 1
    bank = det.open_bank(1, WIN, HOP, batch=1)
    with pytest.raises(RuntimeError, match=r"detection record exceeded: \d+ rows needed, rec_cap = 1"):
        bank.push(0, _quantised(busiest)[1][:, :WIN])
    bank.close()


# ---------------------------------------------------------------------------------------------- detect.py with three WAVs
@pytest.mark.parametrize("track", [False, True])
def test_command_line_tool_runs_three_wavs_through_a_bank(tmp_path, monkeypatch, track):
    monkeypatch.chdir(tmp_path)
    sys.path.insert(0, ROOT)
    import detect
    spec, st = _state()
    torch.save({"state_dict": st, "epoch": 3}, tmp_path / "student.pth")
    chunk = 1000
    for k in range(NS):
        with wave.open(str(tmp_path / ("mic%d.wav" % k)), "wb") as w:
            w.setnchannels(C); w.setsampwidth(2); w.setframerate(44100)
            w.writeframes(np.ascontiguousarray(_quantised(k)[0].numpy().T).astype("<i2").tobytes())
    args = ["--config_file", os.path.join(ROOT, "configs", "mm-distillnet.cfg"), "--checkpoint", str(tmp_path / "student.pth"),
            "--overwrite", '{"image_size": %d}' % S, "--window_s", repr(WIN / 44100), "--hop_s", repr(HOP / 44100),
            "--chunk_s", repr(chunk / 44100), "--output", str(tmp_path / "bank.csv")] + (["--track", "--track_max", "256"] if track else [])
    for k in range(NS):
        args += ["--input", str(tmp_path / ("mic%d.wav" % k))]
    got = detect.main(args)
    # the API on the same round robin: a chunk of every file that still has one, in file order
    det = _detector()
    bank = det.open_bank(NS, WIN, HOP, track=_track_config() if track else None)
    parts = []
    for lo in range(0, max(LENGTHS), chunk):
        for k in range(NS):
            if lo < LENGTHS[k]:
                parts.append(bank.push(k, _quantised(k)[1][:, lo:lo + chunk]))
    parts.append(bank.flush())
    want = bank.concat(parts)
    bank.close()
    _same(got, want)
    assert len(want) == (4 if track else 3) and len(want[0]) >= 10 and len(set(want[1].tolist())) == NS
    lines = open(tmp_path / "bank.csv").read().splitlines()
    assert lines[0] == "session,window,t_start_s,x1,y1,x2,y2,score,label" + (",track" if track else "") and len(lines) == 1 + len(want[0])
    for line, r, s, w, t in zip(lines[1:], want[0], want[1], want[2], want[3] if track else [None] * len(lines)):
        cells = [str(int(s)), str(int(w)), "%.9g" % (int(w) * HOP / 44100)] + ["%.9g" % float(v) for v in r] + ([str(int(t))] if track else [])
        assert line == ",".join(cells)
