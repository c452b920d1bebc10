"""Live streaming detection at any sample rate, CPU side: the C ABI of mmd_ring_resample without a GPU, the ready rule
(mm_distillnet_amd.audio.live_resample_ready) against its definition, the session's schedule - outputs emitted chunk by chunk from a
bounded input history - in numpy float64 against tests/resample_ref.py on the whole input, open_stream's refusals and detect.py's
--live_s checks and chunk reader."""
import ctypes
import os
import sys
import wave

import numpy as np
import pytest

import resample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = (48000, 16000, 22050, 96000, 192000, 8000)


def _detect():
    sys.path.insert(0, ROOT)
    import detect
    return detect


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from mm_distillnet_amd import _lib
    return _lib


# ---------------------------------------------------------------------------------------------- C ABI without a GPU
def test_header_declares_the_entry_point_and_the_library_exports_it():
    _lib_ = _lib()
    sigs = _lib_.LIB.symbols()
    dll = ctypes.CDLL(_lib_.LIB_PATH)
    text = open(_lib_.HEADER).read()
    assert "mmd_ring_resample" in sigs and hasattr(dll, "mmd_ring_resample") and len(sigs["mmd_ring_resample"]) == 14
    assert "mmd_ring_resample_span" in sigs and hasattr(dll, "mmd_ring_resample_span") and len(sigs["mmd_ring_resample_span"]) == 3
    head = text[:text.index("int mmd_ring_resample(")]
    comment = " ".join(ln[2:].strip() for ln in head[head.rindex("\n\n"):].split("\n") if ln.startswith("//"))
    assert "-22" in comment and "no host synchronisation" in comment and "% cap" in comment
    # the bank arguments are mmd_resample_poly's: bank, phase_off, L, M, taps in one run
    assert sigs["mmd_ring_resample"][4:9] == sigs["mmd_resample_poly"][3:8]


def _span_by_definition(L, M, taps):
    """the staged span of a block of one period, restated from the plan in csrc/resample_tile.h: the taps and the spread of the phase
    offsets inside a tile of PH <= 64 phases (L split into equal tiles)"""
    ntile = -(-L // 64)
    PH = -(-L // ntile)
    return ((PH - 1) * M) // L + 1 + taps


def test_staged_span_is_the_plans():
    dll = _lib().LIB.load()
    for sr in RATES:
        L, M = R.ratio(sr, 44100)
        taps = 2 * R.half_len(L, M)
        span = dll.mmd_ring_resample_span(L, M, taps)
        assert span == _span_by_definition(L, M, taps) and taps < span <= taps + M, (sr, span)
    assert dll.mmd_ring_resample_span(147, 160, 140) == 53 + 140
    for bad in ((0, 160, 140), (147, 0, 140), (1025, 160, 140), (147, 1025, 140), (147, 160, 141), (147, 160, 0), (147, 160, 4098)):
        assert dll.mmd_ring_resample_span(*bad) == -22, bad


def test_bad_arguments_are_rejected_without_gpu():
    dll = _lib().LIB.load()
    p = ctypes.c_void_p(4096)            # never dereferenced: validation precedes any launch
    L, M, taps = 147, 160, 140
    span = dll.mmd_ring_resample_span(L, M, taps)
    big = (1 << 50) + 1
    # 5000 inputs pushed into a ring of 3300: the inputs 1700 .. 4999 are resident.  Output 1700 reads the inputs from
    # (1700 * 160) // 147 - 69 = 1781 on; the outputs up to ceil((5000 - 70) * 147 / 160) - 1 = 4529 have their last tap.
    good = dict(in_ring=p, in_cap=3300, channels=8, n_valid=5000, bank=p, off=p, L=L, M=M, taps=taps, out_ring=p, out_cap=7158, t_lo=1700,
                t_hi=4530)

    def rr(**kw):
        a = dict(good, **kw)
        return dll.mmd_ring_resample(a["in_ring"], a["in_cap"], a["channels"], a["n_valid"], a["bank"], a["off"], a["L"], a["M"], a["taps"],
                                     a["out_ring"], a["out_cap"], a["t_lo"], a["t_hi"], None)

    for name in ("in_ring", "bank", "off", "out_ring"):
        assert rr(**{name: None}) == -22, name
    for kw in (dict(channels=0), dict(channels=-8), dict(channels=65536),
               dict(L=0), dict(L=1025), dict(M=0), dict(M=1025), dict(taps=141), dict(taps=0), dict(taps=-2), dict(taps=4098),
               dict(t_lo=-1), dict(t_hi=1700), dict(t_hi=1699), dict(t_hi=1700 + 7159), dict(out_cap=2829), dict(out_cap=0),
               dict(in_cap=big), dict(out_cap=big), dict(n_valid=big), dict(t_hi=big, out_cap=1 << 50), dict(t_lo=big, t_hi=big + 1),
               dict(n_valid=-1), dict(in_cap=0), dict(in_cap=-3300),
               dict(in_cap=span - 1, n_valid=150),       # below the least staged span (nothing overwritten yet: that alone refuses it)
               dict(t_lo=1620),                          # its oldest input, (1620 * 160) // 147 - 69 = 1694, is overwritten: 1694 < 1700
               dict(n_valid=5082)):                      # the same range after 82 more inputs: 1781 < 5082 - 3300
        assert rr(**kw) == -22, kw
    assert (1621 * 160) // 147 - 69 == 1695 and (1626 * 160) // 147 - 69 == 1700      # the first range that is still whole starts at 1626


# ---------------------------------------------------------------------------------------------- the ready rule
def test_ready_rule_against_its_definition():
    from mm_distillnet_amd.audio import live_resample_ready, resample_len, resample_ratio
    for sr in RATES:
        L, M, half = resample_ratio(sr)
        assert (L, M) == R.ratio(sr, 44100) and half == R.half_len(L, M)
        before = 0
        for n in range(0, 3 * 2 * half + 1):
            # by brute force: the outputs whose last tap (t * M) // L + half is among the n samples form a prefix
            t = 0
            while (t * M) // L + half <= n - 1:
                t += 1
            got = live_resample_ready(n, L, M, half)
            assert got == t, (sr, n, got, t)
            assert got >= before                                                     # monotone
            before = got
            final = live_resample_ready(n, L, M, half, final=True)
            assert final == resample_len(n, sr) == R.n_out(n, L, M) and final >= got, (sr, n)
        assert before > 0


def test_chunked_outputs_from_a_bounded_history_equal_the_whole_resample():
    """The session's schedule in numpy float64: after each chunk the outputs produced .. ready-1 are computed from ONLY the last
    taps + M + chunk inputs (everything older reads as NaN, so a tap that reached further back would poison the sum), then the final
    ones with zeros behind the end.  Equal to resample_ref of the whole array, exactly."""
    from mm_distillnet_amd.audio import live_resample_ready
    rng = np.random.default_rng(7)
    n_in = 5000
    for sr in (48000, 16000):
        L, M = R.ratio(sr, 44100)
        half, bank = R.half_len(L, M), R.bank(L, M).astype(np.float64)
        taps = 2 * half
        x = rng.standard_normal(n_in).astype(np.float32)
        want = R.resample_ref(x, sr, dtype=np.float64)
        for trial in range(6):
            chunks, left = [], n_in
            while left:
                c = int(min(left, rng.choice([1, 2, 37, half, taps, 500, 1500])))
                chunks.append(c)
                left -= c
            out, pushed, produced = [], 0, 0

            def emit(ready, history, final):
                nonlocal produced
                t = np.arange(produced, ready, dtype=np.int64)
                n, p = (t * M) // L, (t * M) % L
                acc = np.zeros(len(t))
                for j in range(taps):                                                # tap order, as resample_ref accumulates
                    i = n + j - half + 1
                    if not final:
                        assert (i < pushed).all(), (j, pushed)                       # the ready rule: no tap ahead of what was pushed
                    inside = (i >= 0) & (i < pushed)
                    v = np.where(inside, x[np.clip(i, 0, n_in - 1)].astype(np.float64), 0.0)
                    v = np.where(inside & (i < pushed - history), np.nan, v)         # older than the history: not there any more
                    acc = acc + v * bank[p, j]
                out.append(acc)
                produced = ready

            for c in chunks:
                pushed += c
                emit(live_resample_ready(pushed, L, M, half), taps + M + c, False)
            emit(live_resample_ready(pushed, L, M, half, final=True), taps + M, True)
            got = np.concatenate(out)
            assert len(got) == len(want) and np.isfinite(got).all(), (sr, trial)
            assert np.array_equal(got, want), (sr, trial, np.abs(got - want).max())


# ---------------------------------------------------------------------------------------------- open_stream
def test_open_stream_refuses_a_short_input_ring_and_an_unsupported_ratio():
    """the session checks its geometry before it touches the device: a stand-in detector is enough"""
    from types import SimpleNamespace as NS
    from mm_distillnet_amd.audio import live_in_ring_min
    from mm_distillnet_amd.detector import LiveSession
    _lib()
    det = NS(net=NS(spec=NS(in_channels=8)), front=NS(n_frames=lambda n: 1 + n // 256))
    assert live_in_ring_min(147, 160, 70) == 140 + 160 + 1                           # above the 193 samples a one-period block stages
    with pytest.raises(ValueError, match="in_ring_len = 300 is shorter than the 301 samples"):
        LiveSession(det, 4096, 1531, 3, None, None, 48000, 300)
    assert live_in_ring_min(147, 640, 279) == 558 + 640 + 1
    with pytest.raises(ValueError, match="in_ring_len = 1198 is shorter than the 1199 samples"):
        LiveSession(det, 4096, 1531, 3, None, None, 192000, 1198)
    with pytest.raises(ValueError, match="44100 / 44101"):
        LiveSession(det, 4096, 1531, 3, None, None, 44101, None)
    with pytest.raises(ValueError, match="in_ring_len goes with a sample_rate"):
        LiveSession(det, 4096, 1531, 3, None, None, 44100, 5000)
    with pytest.raises(ValueError, match="ring_len = 7157 is shorter than one group"):    # the 44.1 kHz ring's check stands
        LiveSession(det, 4096, 1531, 3, None, 7157, 48000, None)


# ---------------------------------------------------------------------------------------------- detect.py --live_s
def test_live_flags_are_refused_before_any_device_work(tmp_path, monkeypatch):
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
    open(tmp_path / "a.mp3", "wb").write(b"x")
    base = ["--config_file", os.path.join(ROOT, "configs", "mm-distillnet.cfg"), "--checkpoint", "none.pth", "--output", str(tmp_path / "o.csv")]
    with pytest.raises(ValueError, match="--live_s .* needs --window_s"):
        det.main(base + ["--input", str(tmp_path / "a.wav"), "--live_s", "0.1"])
    with pytest.raises(ValueError, match="--live_s does not go with --chunk_s"):
        det.main(base + ["--input", str(tmp_path / "a.npy"), "--live_s", "0.1", "--chunk_s", "0.1", "--window_s", "0.01"])
    with pytest.raises(ValueError, match="positive number of seconds"):
        det.main(base + ["--input", str(tmp_path / "a.wav"), "--live_s", "0", "--window_s", "0.01"])
    with pytest.raises(ValueError, match="positive number of seconds"):
        det.main(base + ["--input", str(tmp_path / "a.npy"), "--live_s", "1e-9", "--window_s", "0.01", "--sample_rate", "48000"])
    with pytest.raises(ValueError, match="unsupported input"):
        det.main(base + ["--input", str(tmp_path / "a.mp3"), "--live_s", "0.1", "--window_s", "0.01"])
    with pytest.raises(ValueError, match="a .wav holds its rate"):
        det.main(base + ["--input", str(tmp_path / "a.wav"), "--live_s", "0.1", "--window_s", "0.01", "--sample_rate", "48000"])
    with pytest.raises(ValueError, match="--resample reads a .wav"):
        det.main(base + ["--input", str(tmp_path / "a.npy"), "--live_s", "0.1", "--window_s", "0.01", "--resample"])
    assert not os.path.exists(tmp_path / "o.csv")


def test_open_live_reads_a_chunk_at_a_time_at_the_files_rate(tmp_path):
    from mm_distillnet_amd import recording as det
    rng = np.random.default_rng(0)
    frames = 1000
    raw = rng.integers(0, 256, frames * 8 * 3, dtype=np.uint8).tobytes()              # 24-bit frames, any bytes
    with wave.open(str(tmp_path / "a.wav"), "wb") as w:
        w.setnchannels(8); w.setsampwidth(3); w.setframerate(48000)
        w.writeframes(raw)
    n, rate, chunks = det.open_chunks(str(tmp_path / "a.wav"), 0.00625, any_rate=True)                 # round(0.00625 * 48000) = 300 frames
    chunks = list(chunks)
    assert (n, rate) == (1000, 48000) and [len(c) // 24 for c, _ in chunks] == [300, 300, 300, 100] and all(wd == 3 for _, wd in chunks)
    assert b"".join(c for c, _ in chunks) == raw
    wav = rng.standard_normal((8, 1000)).astype(np.float32)
    np.save(tmp_path / "a.npy", wav)
    n, rate, chunks = det.open_chunks(str(tmp_path / "a.npy"), 0.00625, True, 48000)
    chunks = list(chunks)
    assert (n, rate) == (1000, 48000) and [c.shape for c, _ in chunks] == [(8, 300)] * 3 + [(8, 100)] and all(wd is None for _, wd in chunks)
    assert np.array_equal(np.concatenate([c for c, _ in chunks], axis=1), wav)
    assert det.open_chunks(str(tmp_path / "a.npy"), 0.01, any_rate=True)[1] == 44100
    with wave.open(str(tmp_path / "b.wav"), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(48000)
        w.writeframes(b"\0" * 400)
    with pytest.raises(ValueError, match="expected 8 microphone channels"):
        det.open_chunks(str(tmp_path / "b.wav"), 0.01, any_rate=True)
