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
    det = _detect()
    rng = np.random.default_rng(0)
    pcm = rng.integers(-32768, 32768, (1000, 8)).astype("<i2")
    with wave.open(str(tmp_path / "a.wav"), "wb") as w:
        w.setnchannels(8); w.setsampwidth(2); w.setframerate(44100)
        w.writeframes(pcm.tobytes())
    n, chunks = det.open_chunked(str(tmp_path / "a.wav"), 300)
    chunks = list(chunks)
    assert n == 1000 and [len(c) // 16 for c, _ in chunks] == [300, 300, 300, 100] and all(wd == 2 for _, wd in chunks)
    assert b"".join(c for c, _ in chunks) == pcm.tobytes()
    wav = rng.standard_normal((8, 1000)).astype(np.float32)
    np.save(tmp_path / "a.npy", wav)
    n, chunks = det.open_chunked(str(tmp_path / "a.npy"), 300)
    chunks = list(chunks)
    assert n == 1000 and [c.shape for c, _ in chunks] == [(8, 300)] * 3 + [(8, 100)] and all(wd is None for _, wd in chunks)
    assert np.array_equal(np.concatenate([c for c, _ in chunks], axis=1), wav)
    np.save(tmp_path / "b.npy", np.zeros((2, 8, 1000), np.float32))
    with pytest.raises(ValueError, match="ONE recording"):
        det.open_chunked(str(tmp_path / "b.npy"), 300)


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
