"""Live bank at per-session sample rates, CPU side: the fast-path rule of a round (`audio.bank_round`) on a host model of the rings,
the ABI of the two batched launches and their planner without a GPU, open_bank's argument checks and detect.py's --any_rate parsing."""
import ctypes
import os
import sys
import wave

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIN, HOP, BATCH, NS = 4096, 1531, 3, 3
SPAN = (BATCH - 1) * HOP + WIN
RATES = (44100, 48000, 16000)
PLAN_SEED, ROUNDS = 5, 60
_CACHE = {}


def _audio():
    sys.path.insert(0, ROOT)
    from mm_distillnet_amd import audio
    return audio


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from mm_distillnet_amd import _lib
    return _lib


def _detect():
    sys.path.insert(0, ROOT)
    import detect
    return detect


# ---------------------------------------------------------------------------------------------- the fast-path rule on a ring model
def _in_cap(a, rate, cap):
    """open_bank's default input ring: taps + M + ceil(cap * M / L)"""
    L, M, half = a.resample_ratio(rate)
    return 2 * half + M - ((-cap * M) // L)


def _plan():
    """Seeded rounds for banks of three sessions: per bank the sessions' rates (drawn from RATES) and the ring length, per round a chunk
    for a random subset of the sessions, from one sample to more than a ring's span (in the session's own samples) -> per round
    (bank, {session: n}, pushes as `bank_round` takes them, verdict).  The verdicts come from `bank_round` on the evolving state."""
    if "plan" not in _CACHE:
        a = _audio()
        rng = np.random.default_rng(PLAN_SEED)
        rounds = []
        for bank in range(4):
            rates = [int(r) for r in rng.choice(RATES, size=NS)] if bank else list(RATES)[1:] + [RATES[0]]      # bank 0: one of each
            cap = SPAN if bank % 2 else 2 * SPAN
            state, in_written = a.bank_state(NS), [0] * NS
            for _ in range(ROUNDS):
                sessions = [s for s in range(NS) if rng.random() < 0.8] or [int(rng.integers(NS))]
                chunk, pushes = {}, []
                for s in sessions:
                    n = int(rng.choice([1, 300, 1000, 1531, 2500, 4096, 6000, 9000, 16000, 40000]) * rates[s] / 44100) or 1
                    chunk[s] = n
                    if rates[s] == 44100:
                        pushes.append((s, [n]))
                        continue
                    L, M, half = a.resample_ratio(rates[s])
                    pieces = a.live_pieces(n, in_written[s], state[0][s], L, M, half, _in_cap(a, rates[s], cap))
                    assert sum(c for c, _ in pieces) == n
                    in_written[s] += n
                    pushes.append((s, [out for _, out in pieces]))
                fast, steps, after, why = a.bank_round(state, pushes, WIN, HOP, BATCH, cap)
                rounds.append(dict(bank=bank, rates=rates, cap=cap, chunk=chunk, pushes=pushes, state=state, fast=fast, why=why, steps=steps,
                                   after=after))
                state = after
        _CACHE["plan"] = rounds
    return _CACHE["plan"]


def test_the_seeded_plan_holds_every_kind_of_round():
    plan = _plan()
    kinds = [r["why"] for r in plan]
    print({k: kinds.count(k) for k in set(kinds)})
    assert kinds.count(None) >= 10 and kinds.count("writes") >= 1 and kinds.count("hoist") >= 1 and kinds.count("pieces") >= 1
    assert all(r["fast"] == (r["why"] is None) for r in plan)
    # fast rounds with ticks in them, with several sessions, and at every rate
    assert any(r["fast"] and len(r["pushes"]) == NS and sum(st[0] == "run" for st in r["steps"]) >= 1 for r in plan)
    for rate in RATES:
        assert any(r["fast"] and rate in [r["rates"][s] for s in r["chunk"]] for r in plan), rate
    chunks = [(n, r["rates"][s], r["cap"]) for r in plan for s, n in r["chunk"].items()]
    assert any(n == 1 for n, _, _ in chunks) and any(n * 44100 > rate * cap for n, rate, cap in chunks)      # one sample; more than a ring


def _ticks_read(rings, cap, windows):
    """what a tick's windows find in the rings: per window the sample ids in its slots"""
    return [rings[s, (w * HOP + np.arange(WIN)) % cap].copy() for s, w in windows]


def test_fast_rounds_read_what_the_sequential_order_reads():
    """Two ring models per bank, holding sample ids: one follows every round's steps in their sequential order, the other does a fast
    round's writes first and its ticks afterwards (and follows the sequential order in every other round).  Every tick of both finds,
    in every slot its windows read, exactly that window's samples; and the ticks are the same."""
    a = _audio()
    plan = _plan()
    for bank in sorted({r["bank"] for r in plan}):
        rounds = [r for r in plan if r["bank"] == bank]
        cap = rounds[0]["cap"]
        seq, hoisted = np.full((NS, cap), -1, np.int64), np.full((NS, cap), -1, np.int64)
        state, n_ticks = a.bank_state(NS), 0
        for r in rounds:
            assert r["state"] == state
            # the sequential steps are bank_schedule's, push by push
            steps = []
            for s, pieces in r["pushes"]:
                for n in pieces:
                    got, state = a.bank_schedule(state, s, n, WIN, HOP, BATCH, cap)
                    steps += got
            assert steps == r["steps"] and state == r["after"]
            order = steps if not r["fast"] else [st for st in steps if st[0] == "write"] + [st for st in steps if st[0] == "run"]
            for rings, todo in ((seq, steps), (hoisted, order)):
                for st in todo:
                    if st[0] == "write":
                        _, s, lo, hi = st
                        assert hi - lo <= cap
                        rings[s, np.arange(lo, hi) % cap] = np.arange(lo, hi)
                    else:
                        for (s, w), ids in zip(st[1], _ticks_read(rings, cap, st[1])):
                            assert (ids == w * HOP + np.arange(WIN)).all(), (bank, s, w, r["why"])
            assert [st[1] for st in order if st[0] == "run"] == [st[1] for st in steps if st[0] == "run"]
            n_ticks += sum(st[0] == "run" for st in steps)
        assert n_ticks >= 5


def test_the_hoist_limit_is_needed():
    """at least one round the rule refuses for the hoist limit alone would hand a tick overwritten samples if its writes went first"""
    a = _audio()
    broken = 0
    for bank in sorted({r["bank"] for r in _plan()}):
        rounds = [r for r in _plan() if r["bank"] == bank]
        cap = rounds[0]["cap"]
        rings = np.full((NS, cap), -1, np.int64)
        for r in rounds:
            if r["why"] == "hoist":
                trial = rings.copy()
                for st in [st for st in r["steps"] if st[0] == "write"] + [st for st in r["steps"] if st[0] == "run"]:
                    if st[0] == "write":
                        trial[st[1], np.arange(st[2], st[3]) % cap] = np.arange(st[2], st[3])
                    else:
                        broken += any((ids != w * HOP + np.arange(WIN)).any() for (s, w), ids in zip(st[1], _ticks_read(trial, cap, st[1])))
            for st in r["steps"]:
                if st[0] == "write":
                    rings[st[1], np.arange(st[2], st[3]) % cap] = np.arange(st[2], st[3])
    assert broken >= 1


def test_a_round_names_each_session_once_in_ascending_order():
    a = _audio()
    state = a.bank_state(NS)
    for bad in ([(1, [10]), (0, [10])], [(0, [10]), (0, [10])]):
        with pytest.raises(ValueError, match="at most once, in ascending order"):
            a.bank_round(state, bad, WIN, HOP, BATCH, SPAN)
    fast, steps, after, why = a.bank_round(state, [(0, [WIN]), (2, [0])], WIN, HOP, BATCH, SPAN)
    assert fast and why is None and steps == [("write", 0, 0, WIN)] and after == ((WIN, 0, 0), (1, 0, 0), ((0, 0),))
    assert a.bank_round(state, [(0, [100, 100])], WIN, HOP, BATCH, SPAN)[3] == "pieces"
    assert a.bank_round(state, [(0, [3 * SPAN])], WIN, HOP, BATCH, SPAN)[3] == "writes"


def test_pieces_follow_the_ready_rule():
    a = _audio()
    L, M, half = a.resample_ratio(48000)
    in_cap = 2 * half + M + 1000
    pieces = a.live_pieces(2500, 70, 0, L, M, half, in_cap)
    assert [c for c, _ in pieces] == [1000, 1000, 500]
    total = 0
    for k, (c, out) in enumerate(pieces):
        total += out
        assert total == a.live_resample_ready(70 + sum(c for c, _ in pieces[:k + 1]), L, M, half)
    with pytest.raises(ValueError, match="no room for a piece"):
        a.live_pieces(10, 0, 0, L, M, half, 2 * half + M)


# ---------------------------------------------------------------------------------------------- C ABI without a GPU
def test_header_declares_the_batched_entry_points():
    lib = _lib()
    sigs = lib.LIB.symbols()
    dll = ctypes.CDLL(lib.LIB_PATH)
    assert len(sigs["mmd_rings_push"]) == 6 and len(sigs["mmd_rings_resample"]) == 5 and len(sigs["mmd_rings_resample_plan"]) == 15
    for name in ("mmd_rings_push", "mmd_rings_resample", "mmd_rings_resample_plan"):
        assert hasattr(dll, name)
    assert sigs["mmd_rings_resample_plan"][2:] == sigs["mmd_ring_resample"][:-1]      # the planner takes mmd_ring_resample's arguments
    a = _audio()
    assert (a.RINGS_PUSH_DESC, a.RINGS_RS_DESC) == (64, 192)


def test_bad_tables_are_refused_before_any_launch():
    """validation reads the HOST table alone and precedes any launch: the device pointers are never dereferenced"""
    a = _audio()
    dll = _lib().LIB.load()
    p = ctypes.c_void_p(4096)
    tab = np.zeros((3, 8), np.int64)
    good = (0, 1024, 1000, 0, 4096, 7158, 7000, 0)         # {src_off, src_stride, n, kind, ring, cap, p0, 0}
    tab[:] = good
    h = tab.ctypes.data

    def push(n_desc=3, src=p, host=h, dev=p, channels=8):
        return dll.mmd_rings_push(src, host, dev, n_desc, channels, None)

    assert push(n_desc=0) == -22 and push(n_desc=-1) == -22 and push(host=None) == -22 and push(dev=None) == -22 and push(src=None) == -22
    assert push(channels=0) == -22 and push(channels=65536) == -22 and push(n_desc=65536) == -22
    for col, bad in ((0, -4), (0, 2), (1, 999), (2, 0), (2, 7159), (3, 1), (3, 5), (4, 0), (5, (1 << 50) + 1), (6, -1), (6, 7158)):
        tab[:] = good
        tab[1, col] = bad
        assert push() == -22, (col, bad)
    tab[:] = good
    tab[2, 3] = 2                                          # 16-bit frames of 8193 channels: above the PCM tile
    assert push(channels=8193) == -22

    L, M, taps = 147, 160, 140
    rs = np.zeros(2 * a.RINGS_RS_DESC, np.uint8)
    good = dict(in_cap=3300, channels=8, n_valid=5000, L=L, M=M, taps=taps, out_cap=7158, t_lo=1700, t_hi=4530)      # test_live_resample_cpu's

    def plan(index=0, host=rs.ctypes.data, **kw):
        g = dict(good, **kw)
        return dll.mmd_rings_resample_plan(host, index, p, g["in_cap"], g["channels"], g["n_valid"], p, p, g["L"], g["M"], g["taps"], p,
                                           g["out_cap"], g["t_lo"], g["t_hi"])

    assert plan(host=None) == -22 and plan(index=-1) == -22
    for kw in (dict(channels=0), dict(L=0), dict(M=1025), dict(taps=141), dict(t_hi=1700), dict(t_hi=1700 + 7159), dict(in_cap=192, n_valid=150),
               dict(t_lo=1620),                             # its oldest input, 1694, is overwritten: the ring holds 1700 .. 4999
               dict(n_valid=5082)):
        assert plan(**kw) == -22, kw
    assert not rs.any()                                    # a refused entry is left untouched
    assert plan(0) == 0 and plan(1, t_lo=1626, t_hi=1627) == 0 and rs[:a.RINGS_RS_DESC].any()
    words = rs.view(np.int64).reshape(2, -1)
    assert words[0, :9].tolist() == [4096, 4096, 4096, 4096, 3300, 5000, 7158, 1700, 4530]
    assert words[0, 9:11].view(np.int32).tolist()[:3] == [L, M, taps]

    def launch(n_desc=2, host=rs.ctypes.data, dev=p, channels=8):
        return dll.mmd_rings_resample(host, dev, n_desc, channels, None)

    assert launch(n_desc=0) == -22 and launch(host=None) == -22 and launch(dev=None) == -22 and launch(channels=0) == -22
    assert launch(n_desc=2, channels=40000) == -22         # channels * n_desc rides in gridDim.z
    keep = rs.copy()
    for word, bad in ((7, 1620), (5, 5082), (4, 100), (0, 0), (11, 12345), (12, 7)):      # t_lo / n_valid: overwritten; a plan that is not the planner's
        rs[:] = keep
        words[1, word] = bad
        assert launch() == -22, (word, bad)
    with pytest.raises(ValueError, match="contiguous uint8"):
        a.Resampler.rings_resample_plan(None, np.zeros(100, np.uint8), 0, None, 0, 48000, None, 0, 1)
    with pytest.raises(ValueError, match="host table"):
        a.rings_push_into(4096, np.zeros((2, 7), np.int64), 4096, 2, 8)


# ---------------------------------------------------------------------------------------------- open_bank
def test_open_bank_checks_rates_and_input_rings_before_device_work():
    """the bank settles its geometry before it touches the device: a stand-in detector is enough"""
    from types import SimpleNamespace
    from mm_distillnet_amd.detector import LiveBank
    _lib()
    det = SimpleNamespace(net=SimpleNamespace(spec=SimpleNamespace(in_channels=8)), front=SimpleNamespace(n_frames=lambda n: 1 + n // 256),
                          cand_cap=0, STREAM_ROWS_PER_WINDOW=256)

    def bank(sample_rates=None, in_ring_len=None, ring_len=None):
        return LiveBank(det, NS, WIN, HOP, BATCH, None, ring_len, sample_rates, in_ring_len)

    with pytest.raises(ValueError, match="sample_rates has 2 entries for 3 sessions"):
        bank([48000, None])
    with pytest.raises(ValueError, match="44100 / 44101"):
        bank([None, 44101, 48000])
    with pytest.raises(ValueError, match="in_ring_len = 300 of session 0 is shorter than the 301 samples"):
        bank([48000, None, 16000], 300)
    with pytest.raises(ValueError, match="in_ring_len = 300 of session 2 is shorter than the 301 samples"):
        bank([16000, None, 48000], [5000, None, 300])
    with pytest.raises(ValueError, match="in_ring_len goes with sessions at a sample rate other than 44100"):
        bank(None, 5000)
    with pytest.raises(ValueError, match="in_ring_len goes with sessions at a sample rate other than 44100"):
        bank([44100, None, 44100], 5000)
    with pytest.raises(ValueError, match="in_ring_len goes with sessions at a sample rate other than 44100"):
        bank([48000, None, 44100], [5000, 5000, None])
    with pytest.raises(ValueError, match="in_ring_len has 2 entries"):
        bank([48000, None, 44100], [5000, None])
    with pytest.raises(ValueError, match="ring_len = 7157 is shorter than one group"):       # the 44.1 kHz ring's check stands
        bank([48000, None, 16000], ring_len=7157)


# ---------------------------------------------------------------------------------------------- detect.py --any_rate
BASE = ["--config_file", "c.cfg", "--checkpoint", "p.pth", "--output", "o.csv"]


def test_any_rate_parses_with_several_inputs():
    a = _detect().parse_args(BASE + ["--input", "a.wav", "--input", "b.wav", "--input", "c.WAV", "--window_s", "1", "--chunk_s", "0.1", "--any_rate"])
    assert a.any_rate and a.inputs == ["a.wav", "b.wav", "c.WAV"] and a.batch is None
    assert not _detect().parse_args(BASE + ["--input", "a.wav", "--input", "b.wav", "--window_s", "1", "--chunk_s", "0.1"]).any_rate


@pytest.mark.parametrize("extra,msg", [
    (["--input", "a.wav", "--window_s", "1", "--chunk_s", "0.1"], "--any_rate is for several --input"),
    (["--input", "a.wav", "--input", "b.npy", "--window_s", "1", "--chunk_s", "0.1"], r"b.npy: --any_rate reads 8-channel PCM .wav"),
    (["--input", "a.wav", "--input", "b.wav", "--window_s", "1"], "need --window_s and --chunk_s"),
    (["--input", "a.wav", "--input", "b.wav", "--chunk_s", "0.1"], "need --window_s and --chunk_s"),
    (["--input", "a.wav", "--input", "b.wav", "--window_s", "1", "--chunk_s", "0.1", "--resample"], "--any_rate does not go with --resample"),
    (["--input", "a.wav", "--input", "b.wav", "--window_s", "1", "--chunk_s", "0.1", "--live_s", "0.1"], "--any_rate does not go with"),
])
def test_any_rate_is_refused_from_the_flags_alone(extra, msg):
    with pytest.raises(ValueError, match=msg):
        _detect().parse_args(BASE + extra + ["--any_rate"])


def test_any_rate_refuses_an_unsupported_ratio_before_device_work(tmp_path, monkeypatch):
    det = _detect()
    import torch
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a device call was made")))
    for name, rate in (("a", 48000), ("b", 44101)):
        with wave.open(str(tmp_path / (name + ".wav")), "wb") as w:
            w.setnchannels(8); w.setsampwidth(2); w.setframerate(rate)
            w.writeframes(np.zeros((9000, 8), "<i2").tobytes())
    with pytest.raises(ValueError, match="44100 / 44101"):
        det.main(["--config_file", os.path.join(ROOT, "configs", "mm-distillnet.cfg"), "--checkpoint", "none.pth", "--output", str(tmp_path / "o.csv"),
                  "--input", str(tmp_path / "a.wav"), "--input", str(tmp_path / "b.wav"), "--window_s", "0.05", "--chunk_s", "0.1", "--any_rate"])
    assert not os.path.exists(tmp_path / "o.csv")
