"""Live streaming detection, CPU side: the C ABI of the ring entry points (mmd_ring_push, mmd_ring_push_pcm, mmd_melspec_windows_ring)
without a GPU, detect.py's --chunk_s checks, and the session's schedule (mm_distillnet_amd.audio.live_schedule) against a restatement
written here: which group runs after which push, and that no sample a pending window needs is ever overwritten."""
import ctypes
import os
import sys
import wave

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = (("mmd_ring_push", 8), ("mmd_ring_push_pcm", 8), ("mmd_melspec_windows_ring", 14))


def _detect():
    sys.path.insert(0, ROOT)
    import detect
    return detect


# ---------------------------------------------------------------------------------------------- C ABI without a GPU
def test_header_declares_the_entry_points_and_the_library_exports_them():
    import __graft_entry__ as ge
    ge.build()
    from mm_distillnet_amd import _lib
    sigs = _lib.LIB.symbols()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    text = open(_lib.HEADER).read()
    for name, nargs in ENTRY_POINTS:
        assert name in sigs and hasattr(dll, name) and len(sigs[name]) == nargs, name
        head = text[:text.index("int %s(" % name)]
        comment = " ".join(ln[2:].strip() for ln in head[head.rindex("\n\n"):].split("\n") if ln.startswith("//"))
        assert "-22" in comment and "no host synchronisation" in comment and "% cap" in comment, name
    assert sigs["mmd_melspec_windows_ring"] == sigs["mmd_melspec_windows"]          # cap in n_total's place, nothing else


def test_bad_arguments_are_rejected_without_gpu():
    import __graft_entry__ as ge
    ge.build()
    from mm_distillnet_amd import _lib
    dll = _lib.LIB.load()
    p = ctypes.c_void_p(4096)            # never dereferenced: validation precedes any launch

    good = dict(src=p, stride=1000, channels=8, n=1000, ring=p, cap=7001, pos=123)

    def push(**kw):
        a = dict(good, **kw)
        return dll.mmd_ring_push(a["src"], a["stride"], a["channels"], a["n"], a["ring"], a["cap"], a["pos"], None)

    for kw in (dict(src=None), dict(ring=None), dict(channels=0), dict(channels=-8), dict(n=0), dict(n=-1), dict(n=7002, stride=7002),
               dict(pos=-1), dict(stride=999), dict(stride=0), dict(cap=0), dict(cap=-7001), dict(channels=65536),
               dict(cap=(1 << 50) + 1), dict(pos=(1 << 50) + 1)):
        assert push(**kw) == -22, kw

    goodp = dict(pcm=p, frames=1000, channels=8, width=2, ring=p, cap=7001, pos=123)

    def push_pcm(**kw):
        a = dict(goodp, **kw)
        return dll.mmd_ring_push_pcm(a["pcm"], a["frames"], a["channels"], a["width"], a["ring"], a["cap"], a["pos"], None)

    for kw in (dict(pcm=None), dict(ring=None), dict(frames=0), dict(frames=-1), dict(channels=0), dict(channels=-8), dict(width=1),
               dict(width=0), dict(width=5), dict(width=8), dict(channels=8193), dict(channels=4097, width=4),       # mmd_pcm_to_float's
               dict(frames=7002), dict(pos=-1), dict(cap=0), dict(cap=(1 << 50) + 1), dict(pos=(1 << 50) + 1)):
        assert push_pcm(**kw) == -22, kw

    goodm = dict(ring=p, channels=8, cap=7001, starts=p, batch=3, win_len=4096, bs=p, bl=p, bw=p, stride=50, db=1, ws=p, out=p)

    def mel(**kw):
        a = dict(goodm, **kw)
        return dll.mmd_melspec_windows_ring(a["ring"], a["channels"], a["cap"], a["starts"], a["batch"], a["win_len"], a["bs"], a["bl"],
                                            a["bw"], a["stride"], a["db"], a["ws"], a["out"], None)

    for name in ("ring", "starts", "bs", "bl", "bw", "out", "ws"):
        assert mel(**{name: None}) == -22, name
    for kw in (dict(channels=0), dict(batch=0), dict(batch=-3), dict(win_len=512), dict(win_len=0), dict(win_len=7002), dict(cap=4095),
               dict(stride=0), dict(stride=52), dict(db=2), dict(db=-1)):
        assert mel(**kw) == -22, kw


# ---------------------------------------------------------------------------------------------- detect.py --chunk_s
def test_chunk_flags_are_refused_before_any_device_work(tmp_path, monkeypatch):
    """main() raises on the flags alone: torch.cuda.set_device would be the first device call, and it is never reached"""
    det = _detect()
    import torch

    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    np.save(tmp_path / "a.npy", np.zeros((8, 700), np.float32))
    with wave.open(str(tmp_path / "a.wav"), "wb") as w:
        w.setnchannels(8); w.setsampwidth(2); w.setframerate(48000)
        w.writeframes(np.zeros((700, 8), "<i2").tobytes())
    base = ["--config_file", os.path.join(ROOT, "configs", "mm-distillnet.cfg"), "--checkpoint", "none.pth", "--output", str(tmp_path / "o.csv")]
    with pytest.raises(ValueError, match="--chunk_s .* needs --window_s"):
        det.main(base + ["--input", str(tmp_path / "a.npy"), "--chunk_s", "0.1"])
    with pytest.raises(ValueError, match="--chunk_s does not go with --resample / --sample_rate"):
        det.main(base + ["--input", str(tmp_path / "a.wav"), "--chunk_s", "0.1", "--window_s", "0.01", "--resample"])
    with pytest.raises(ValueError, match="--chunk_s does not go with --resample / --sample_rate"):
        det.main(base + ["--input", str(tmp_path / "a.npy"), "--chunk_s", "0.1", "--window_s", "0.01", "--sample_rate", "48000"])
    with pytest.raises(ValueError, match="positive number of seconds"):
        det.main(base + ["--input", str(tmp_path / "a.npy"), "--chunk_s", "0", "--window_s", "0.01"])
    assert not os.path.exists(tmp_path / "o.csv")


def test_open_chunked_reads_a_chunk_at_a_time(tmp_path):
    from mm_distillnet_amd import recording as det
    rng = np.random.default_rng(0)
    pcm = rng.integers(-32768, 32768, (1000, 8)).astype("<i2")
    with wave.open(str(tmp_path / "a.wav"), "wb") as w:
        w.setnchannels(8); w.setsampwidth(2); w.setframerate(44100)
        w.writeframes(pcm.tobytes())
    n, _, chunks = det.open_chunks(str(tmp_path / "a.wav"), 300 / 44100, any_rate=False)
    chunks = list(chunks)
    assert n == 1000 and [len(c) // 16 for c, _ in chunks] == [300, 300, 300, 100] and all(wd == 2 for _, wd in chunks)
    assert b"".join(c for c, _ in chunks) == pcm.tobytes()
    wav = rng.standard_normal((8, 1000)).astype(np.float32)
    np.save(tmp_path / "a.npy", wav)
    n, _, chunks = det.open_chunks(str(tmp_path / "a.npy"), 300 / 44100, any_rate=False)
    chunks = list(chunks)
    assert n == 1000 and [c.shape for c, _ in chunks] == [(8, 300)] * 3 + [(8, 100)] and all(wd is None for _, wd in chunks)
    assert np.array_equal(np.concatenate([c for c, _ in chunks], axis=1), wav)
    np.save(tmp_path / "b.npy", np.zeros((2, 8, 1000), np.float32))
    with pytest.raises(ValueError, match="ONE recording"):
        det.open_chunks(str(tmp_path / "b.npy"), 300 / 44100, any_rate=False)


# ---------------------------------------------------------------------------------------------- the schedule
def test_a_ring_below_the_group_span_raises():
    from mm_distillnet_amd.audio import live_group_span, live_schedule
    assert live_group_span(4096, 1531, 3) == 2 * 1531 + 4096 == 7158
    with pytest.raises(ValueError, match="7157 samples is shorter than one group of 3 windows"):
        live_schedule(0, 0, 100, 4096, 1531, 3, 7157)
    assert live_schedule(0, 0, 7158, 4096, 1531, 3, 7158) == ([("write", 0, 7158), ("run", 0)], 7158, 1)
    assert live_schedule(0, 0, 7157, 4096, 1531, 3, 7158) == ([("write", 0, 7157)], 7157, 0)
    assert live_schedule(7157, 0, 1, 4096, 1531, 3, 7158) == ([("write", 7157, 7158), ("run", 0)], 7158, 1)


def test_open_stream_refuses_a_ring_below_the_group_span():
    """the session checks its geometry before it touches the device: a stand-in detector is enough"""
    from types import SimpleNamespace as NS
    from mm_distillnet_amd.detector import LiveSession
    det = NS(net=NS(spec=NS(in_channels=8)), front=NS(n_frames=lambda n: 1 + n // 256))
    with pytest.raises(ValueError, match="ring_len = 7157 is shorter than one group of 3 windows .7158 samples."):
        LiveSession(det, 4096, 1531, 3, None, 7157)
    with pytest.raises(ValueError, match="hop = 0"):
        LiveSession(det, 4096, 0, 3, None, None)
    with pytest.raises(ValueError, match="batch = 0"):
        LiveSession(det, 4096, 1531, 0, None, None)


def _groups_by_definition(chunks, win_len, hop, batch):
    """the restatement: after push k the total is t_k; group g is complete when t_k >= (g * batch + batch - 1) * hop + win_len.
    -> per push, the list of groups that became complete with it"""
    out, total, done = [], 0, 0
    for n in chunks:
        total += n
        full_windows = 0 if total < win_len else 1 + (total - win_len) // hop
        out.append(list(range(done, full_windows // batch)))
        done = full_windows // batch
    return out


def test_schedule_over_random_chunkings():
    """300 random geometries and chunkings, a third of them with hop > win_len: every group runs in the push that brings its last
    sample, in order; and in a simulated ring of slots every sample of a running group's windows is still the one last written there."""
    from mm_distillnet_amd.audio import live_group_span, live_schedule
    rng = np.random.default_rng(2024)
    ran_any = gaps = long_chunks = 0
    for trial in range(300):
        win_len = int(rng.integers(513, 900))
        hop = int(rng.integers(win_len + 1, 3 * win_len)) if trial % 3 == 0 else int(rng.integers(1, win_len + 1))
        batch = int(rng.integers(1, 5))
        span = live_group_span(win_len, hop, batch)
        cap = span if trial % 4 == 0 else span + int(rng.integers(0, 2 * span))
        chunks = [int(n) for n in rng.choice([1, 7, hop, win_len, span - 1, span, span + 1, cap, cap + 1, 3 * cap + 5], size=int(rng.integers(3, 12)))]
        want = _groups_by_definition(chunks, win_len, hop, batch)
        slot = np.full(cap, -1, np.int64)                 # the absolute sample each slot holds
        written, group = 0, 0
        for n, want_groups in zip(chunks, want):
            steps, new_written, new_group = live_schedule(written, group, n, win_len, hop, batch, cap)
            got_groups, at = [], written
            for st in steps:
                if st[0] == "write":
                    _, lo, hi = st
                    assert at <= lo < hi <= written + n and hi - lo <= cap           # in order, inside the chunk, one lap at the most
                    gaps += lo > at
                    p = np.arange(lo, hi)
                    slot[p % cap] = p
                    at = hi
                else:
                    g = st[1]
                    got_groups.append(g)
                    for w in range(g * batch, (g + 1) * batch):
                        p = np.arange(w * hop, w * hop + win_len)
                        assert p[-1] < at                                            # only pushed samples
                        assert np.array_equal(slot[p % cap], p), (trial, g, w)       # and none overwritten or skipped
            assert got_groups == want_groups, (trial, chunks, got_groups, want_groups)
            assert new_written == written + n and new_group == group + len(got_groups)
            written, group = new_written, new_group
            ran_any += len(got_groups)
            long_chunks += n > cap
        # what flush() runs: the complete windows behind the last full group are resident too
        W = 0 if written < win_len else 1 + (written - win_len) // hop
        assert 0 <= W - group * batch < batch
        for w in range(group * batch, W):
            p = np.arange(w * hop, w * hop + win_len)
            assert np.array_equal(slot[p % cap], p), (trial, "flush", w)
    assert ran_any > 300 and gaps > 20 and long_chunks > 50                           # the cases were really met


# ---------------------------------------------------------------------------------------------- one scheduler, one planning function
def _live_schedule_model(written, group, n, win_len, hop, batch, cap):
    """the loop `audio.live_schedule` was before it became `audio.bank_schedule` for one session, kept here as the model"""
    span = (batch - 1) * hop + win_len
    steps, end = [], written + n
    while True:
        start = group * batch * hop
        while start + span <= written:
            steps.append(("run", group))
            group += 1
            start += batch * hop
        if written == end:
            return steps, written, group
        hi = min(end, start + cap)
        lo = max(written, start)
        if lo < hi:
            steps.append(("write", lo, hi))
        written = hi


def test_live_schedule_is_the_bank_schedule_of_one_session():
    """The whole lattice of geometries - win_len x hop (also > win_len) x batch (also 1) x ring (also exactly one span) - each with a
    seeded chain of up to 8 pushes of 1 .. 3 * cap + 5 samples: `live_schedule` gives the model's steps and (written, group); a bank
    of one session, chained on its own state, gives the same steps read as the session's; its state after every push is the one
    `live_schedule` rebuilds from (written, group) - the FIFO is windows group * batch .. W - 1 - and `bank_step` runs exactly those."""
    from mm_distillnet_amd.audio import bank_schedule, bank_state, bank_step, live_group_span, live_schedule
    rng = np.random.default_rng(18165)
    pushes = tight = gapped = single = long_chunks = short_groups = 0
    for win_len in (5, 8, 13, 40):
        for hop in (1, 3, 8, 13, 50, 97):
            for batch in (1, 2, 3, 5):
                span = live_group_span(win_len, hop, batch)
                for extra in (0, 1, 7, span, 3 * span):
                    cap = span + extra
                    written, group, state = 0, 0, bank_state(1)
                    for k in range(int(rng.integers(2, 9))):
                        # every other push anywhere in 1 .. 3 * cap + 5, the others short: they end inside a group, or bring no window
                        n = int(rng.integers(1, 3 * cap + 6)) if k % 2 else int(rng.integers(1, 2 * hop + win_len + 1))
                        want = _live_schedule_model(written, group, n, win_len, hop, batch, cap)
                        assert live_schedule(written, group, n, win_len, hop, batch, cap) == want, (win_len, hop, batch, cap, written, group, n)
                        steps, state = bank_schedule(state, 0, n, win_len, hop, batch, cap)
                        for st in steps:
                            if st[0] == "run":            # a tick is one group: batch consecutive windows from a multiple of batch
                                w0 = st[1][0][1]
                                assert w0 % batch == 0 and list(st[1]) == [(0, w0 + i) for i in range(batch)]
                        read = [("write", st[2], st[3]) if st[0] == "write" else ("run", st[1][0][1] // batch) for st in steps]
                        assert read == want[0]
                        _, written, group = want
                        W = 0 if written < win_len else 1 + (written - win_len) // hop
                        waiting = [(0, w) for w in range(group * batch, W)]
                        assert state == ((written,), (W,), tuple(waiting)) and len(waiting) < batch
                        last, after = bank_step(state)
                        assert last == ([("run", waiting)] if waiting else []) and after == ((written,), (W,), ())
                        pushes += 1
                        tight += extra == 0
                        gapped += hop > win_len
                        single += batch == 1
                        long_chunks += n > cap
                        short_groups += bool(waiting)
    assert pushes > 2000 and min(tight, gapped, single, long_chunks, short_groups) > 100       # no case was left out


def test_one_planning_function_words_both_openings():
    """`_plan_live` refuses for `open_stream` and for `open_bank` in the words each had when it checked for itself (the strings below
    are copied from those two constructors), and plans the same geometry for a session as for a bank of that one session."""
    from types import SimpleNamespace as NS
    from mm_distillnet_amd.detector import _plan_live
    det = NS(net=NS(spec=NS(in_channels=8)), front=NS(n_frames=lambda n: 1 + n // 256), cand_cap=0, STREAM_ROWS_PER_WINDOW=256)

    def refused(text, who, n_sessions, hop=1531, batch=3, ring_len=None, rates=None, in_ring_len=None):
        with pytest.raises(ValueError) as e:
            _plan_live(who, det, n_sessions, 4096, hop, batch, ring_len, rates, in_ring_len)
        assert str(e.value) == text

    for who, n in (("open_stream", None), ("open_bank", 3)):
        refused(who + ": hop = 0: the windows must advance by at least one sample", who, n, hop=0)
        refused(who + ": batch = 0 (1 .. 1024)", who, n, batch=0)
        refused(who + ": batch = 1025 (1 .. 1024)", who, n, batch=1025)
        refused(who + ": ring_len = 7157 is shorter than one group of 3 windows (7158 samples)", who, n, ring_len=7157)
    refused("open_bank: n_sessions = 0 (1 .. 65535)", "open_bank", 0)
    refused("open_bank: n_sessions = 65536 (1 .. 65535)", "open_bank", 65536)
    # an input ring too short
    refused("open_stream: in_ring_len = 300 is shorter than the 301 samples resampling 48000 Hz needs (140 taps + M = 160 + 1, and no fewer "
            "than a block stages)", "open_stream", None, rates=48000, in_ring_len=300)
    refused("open_bank: in_ring_len = 300 of session 2 is shorter than the 301 samples resampling 48000 Hz needs (140 taps + M = 160 + 1, and "
            "no fewer than a block stages)", "open_bank", 3, rates=[16000, None, 48000], in_ring_len=[5000, None, 300])
    refused("open_bank: in_ring_len = 1198 of session 0 is shorter than the 1199 samples resampling 192000 Hz needs (558 taps + M = 640 + 1, and "
            "no fewer than a block stages)", "open_bank", 3, rates=[192000, None, None], in_ring_len=1198)
    # an input ring where nothing is resampled
    refused("open_stream: in_ring_len goes with a sample_rate other than 44100 (nothing is resampled)", "open_stream", None, in_ring_len=5000)
    refused("open_stream: in_ring_len goes with a sample_rate other than 44100 (nothing is resampled)", "open_stream", None, rates=44100,
            in_ring_len=5000)
    bank_text = "open_bank: in_ring_len goes with sessions at a sample rate other than 44100 (nothing else is resampled)"
    refused(bank_text, "open_bank", 3, in_ring_len=5000)
    refused(bank_text, "open_bank", 3, rates=[44100, None, 44100], in_ring_len=5000)
    refused(bank_text, "open_bank", 3, rates=[48000, None, 44100], in_ring_len=[5000, 5000, None])
    # lists of another length than the bank
    refused("open_bank: sample_rates has 2 entries for 3 sessions", "open_bank", 3, rates=[48000, None])
    refused("open_bank: in_ring_len has 2 entries for 3 sessions", "open_bank", 3, rates=[48000, None, 44100], in_ring_len=[5000, None])
    # which error wins: the ring in front of the rates, the rates' lengths in front of the ratio, the ratio in front of the input ring
    refused("open_bank: ring_len = 7157 is shorter than one group of 3 windows (7158 samples)", "open_bank", 3, ring_len=7157, rates=[48000])
    refused("open_stream: ring_len = 7157 is shorter than one group of 3 windows (7158 samples)", "open_stream", None, ring_len=7157,
            rates=48000, in_ring_len=300)
    with pytest.raises(ValueError, match="44100 / 44101"):
        _plan_live("open_bank", det, 3, 4096, 1531, 3, None, [44101, None, 48000], 300)
    # and what is planned: a session is the bank of that one session, but for its 8-word record's limit
    one = _plan_live("open_stream", det, None, 4096, 1531, 3, None, 48000, None)
    assert one == _plan_live("open_bank", det, 1, 4096, 1531, 3, None, [48000], None)
    assert one == (2 * 7158, 3 * 256, [(48000, 147, 160, 70)], [140 + 160 - ((-2 * 7158 * 160) // 147)])
    assert _plan_live("open_bank", det, 2, 4096, 1531, 3, 7158, [None, 44100], None) == (7158, 768, [None, None], [None, None])
