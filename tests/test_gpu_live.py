"""Live streaming detection on the GPU: the ring front end (mmd_melspec_windows_ring) against mmd_melspec_windows on the linear
recording, bit for bit; the ring writers (mmd_ring_push, mmd_ring_push_pcm) against numpy and mmd_pcm_to_float; a LiveSession
(AudioDetector.open_stream) and detect.py --chunk_s against detect_stream / track_stream of a SECOND detector on the whole recording,
bit for bit, for several ways of cutting the recording into chunks.  The small detector, its recording and its bias tuning are those
of tests/test_gpu_stream.py, restated."""
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
N_TOTAL, WIN = 16000, 4096
HOP, BATCH, N_REC = 1531, 3, 14000        # W = 1 + (14000 - 4096) // 1531 = 7: two full groups, one of one window; a tail is dropped
SPAN = (BATCH - 1) * HOP + WIN            # 7158 samples: one group
BIG = 1 << 31
_CACHE = {}


def _noise(n, seed):
    return torch.randn(C, n, generator=torch.Generator().manual_seed(seed)) * 0.3


def _bits(t):
    return t.contiguous().view(torch.int32)


def _front():
    from mm_distillnet_amd.audio import MelFrontEnd
    if "front" not in _CACHE:
        _CACHE["front"] = MelFrontEnd(DEV)
    return _CACHE["front"]


def _call(name, *args):
    from mm_distillnet_amd import _lib
    return _lib.call(name, *args)


# ---------------------------------------------------------------------------------------------- ring front end
def _linear(wav, starts, db):
    f = _front()
    out = torch.full((len(starts), f.n_mels, f.n_frames(WIN), C), float("nan"), device=DEV)
    ws = torch.full((len(starts) * C,), -1, dtype=torch.int32, device=DEV)
    f.melspec_windows_into(wav, torch.tensor(starts, dtype=torch.int64, device=DEV), WIN, db, ws, out)
    return out


def _ring_windows(ring, starts, db):
    f = _front()
    out = torch.full((len(starts), f.n_mels, f.n_frames(WIN), C), float("nan"), device=DEV)
    ws = torch.full((len(starts) * C,), -1, dtype=torch.int32, device=DEV)
    f.melspec_windows_ring_into(ring, torch.tensor(starts, dtype=torch.int64, device=DEV), WIN, db, ws, out)
    return out


def _ring_holding(wav, cap, first_abs, first_lin, n):
    """a NaN ring of cap slots with ONLY the absolute samples first_abs .. first_abs + n - 1 in it, taken from wav[:, first_lin ...]"""
    ring = torch.full((C, cap), float("nan"))
    slots = (first_abs + torch.arange(n, dtype=torch.int64)) % cap
    ring[:, slots] = wav[:, first_lin:first_lin + n]
    return ring.to(DEV)


# (cap, absolute start, what the case is); 7001 is no multiple of 4 or 256
RING_CASES = [(7001, 100, "no wrap"), (7001, 7001 - WIN, "ends on the last slot"), (7001, 7000, "starts on the last slot"),
              (7001, 3 * 7001 + 5555, "straddles the wrap at an odd offset"), (7001, BIG + 12345, "a start beyond 2^31"),
              (WIN, 0, "cap == win_len, no wrap"), (WIN, WIN - 1, "cap == win_len, starts on the last slot"),
              (WIN, 5 * WIN + 1531, "cap == win_len, odd offset"), (WIN, BIG + 777, "cap == win_len, beyond 2^31")]


@pytest.mark.parametrize("db", [False, True])
def test_ring_windows_equal_the_linear_entry_point(db):
    wav = _noise(N_TOTAL, 1)
    lin = [0, 1531, 3062, 11904, 5001, 7777, 2, 9999, 4096]
    want = _linear(wav.to(DEV), lin, db)
    assert not torch.isnan(want).any() and not torch.equal(want[0], want[1])
    for k, (cap, start, what) in enumerate(RING_CASES):
        ring = _ring_holding(wav, cap, start, lin[k], WIN)
        assert int(torch.isnan(ring[0]).sum()) == cap - WIN
        if "last slot" in what and "starts" in what:
            assert start % cap == cap - 1
        if "ends" in what:
            assert (start + WIN - 1) % cap == cap - 1
        out = _ring_windows(ring, [start], db)
        assert torch.isfinite(out).all(), what                                    # nothing outside the window was read
        assert torch.equal(_bits(out[0]), _bits(want[k])), what


@pytest.mark.parametrize("db", [False, True])
def test_a_group_of_windows_in_a_ring_of_exactly_its_span(db):
    wav = _noise(N_TOTAL, 2)
    first_abs, first_lin = 2 * SPAN + 5000, 3000                                  # the group wraps inside the ring
    ring = _ring_holding(wav, SPAN, first_abs, first_lin, SPAN)
    assert not torch.isnan(ring).any() and (first_abs % SPAN) + SPAN > SPAN
    out = _ring_windows(ring, [first_abs + k * HOP for k in range(BATCH)], db)
    want = _linear(wav.to(DEV), [first_lin + k * HOP for k in range(BATCH)], db)
    assert torch.equal(_bits(out), _bits(want)) and not torch.equal(out[0], out[2])
    again = _ring_windows(ring, [first_abs + k * HOP for k in range(BATCH)], db)
    assert torch.equal(_bits(again), _bits(out))


# ---------------------------------------------------------------------------------------------- ring writers
SENTINEL = -7.25
CAP = 7001


def _expect(cap, pos, rows):
    want = np.full((rows.shape[0], cap), SENTINEL, np.float32)
    want[:, (pos + np.arange(rows.shape[1], dtype=np.int64)) % cap] = rows
    return want


@pytest.mark.parametrize("n,pos,what", [(1, 4 * CAP - 1, "one sample on the last slot"), (CAP, 1234, "a whole lap"),
                                        (3000, CAP - 1501, "a wrap in the middle"), (2500, BIG + 4321, "pos beyond 2^31"),
                                        (1025, 0, "just over one block")])
def test_ring_push_against_numpy(n, pos, what):
    src = _noise(n, n)
    ring = torch.full((C, CAP), SENTINEL, device=DEV)
    _call("mmd_ring_push", src.to(DEV), n, C, n, ring, CAP, pos)
    torch.cuda.synchronize()
    want = _expect(CAP, pos, src.numpy())
    assert (want != SENTINEL).sum() == C * n
    np.testing.assert_array_equal(ring.cpu().numpy().view(np.int32), want.view(np.int32))


def test_ring_push_of_a_column_slice():
    big = _noise(5000, 3).to(DEV)
    lo, n, pos = 1237, 2000, 2 * CAP + 6000                                       # wraps; src_stride = 5000 > n
    ring = torch.full((C, CAP), SENTINEL, device=DEV)
    _call("mmd_ring_push", big.data_ptr() + 4 * lo, big.stride(0), C, n, ring, CAP, pos)
    torch.cuda.synchronize()
    want = _expect(CAP, pos, big[:, lo:lo + n].cpu().numpy())
    np.testing.assert_array_equal(ring.cpu().numpy().view(np.int32), want.view(np.int32))


def _pcm_bytes(frames, width, seed):
    """-> (int64 samples [frames, C] with the extreme values in them, their little-endian bytes)"""
    top = 1 << (8 * width - 1)
    s = np.random.default_rng(seed).integers(-top, top, (frames, C))
    s[0, 0], s[1, 0], s[2, 0], s[3, 0], s[frames - 1, C - 1] = -top, top - 1, -1, 0, -top
    le = s.astype("<i8").view(np.uint8).reshape(frames, C, 8)[:, :, :width]
    return s, np.ascontiguousarray(le).reshape(-1)


@pytest.mark.parametrize("width", [2, 3, 4])
def test_ring_push_pcm_against_numpy_and_pcm_to_float(width):
    frames, pos = 3000, (BIG // CAP + 2) * CAP - 1700                             # beyond 2^31, 1700 slots before the ring's end
    assert pos > BIG and pos % CAP == CAP - 1700
    s, raw = _pcm_bytes(frames, width, width)
    buf = torch.zeros(raw.size + 8, dtype=torch.uint8)
    buf[1:1 + raw.size] = torch.from_numpy(raw)                                   # the frames start on an ODD address
    buf = buf.to(DEV)
    assert (buf.data_ptr() + 1) % 2 == 1
    ring = torch.full((C, CAP), SENTINEL, device=DEV)
    _call("mmd_ring_push_pcm", buf.data_ptr() + 1, frames, C, width, ring, CAP, pos)
    aligned = torch.from_numpy(raw).to(DEV)
    linear = torch.empty(C, frames, device=DEV)
    _call("mmd_pcm_to_float", aligned, frames, C, width, linear)
    torch.cuda.synchronize()
    by_numpy = (s.astype(np.float32) / np.float32(1 << (8 * width - 1))).T        # float32(i) / float32(2^k): the header's rule
    np.testing.assert_array_equal(linear.cpu().numpy().view(np.int32), np.ascontiguousarray(by_numpy).view(np.int32))
    want = _expect(CAP, pos, linear.cpu().numpy())
    np.testing.assert_array_equal(ring.cpu().numpy().view(np.int32), want.view(np.int32))
    assert linear.cpu().numpy().min() == -1.0 and (want != SENTINEL).sum() == C * frames


def test_ring_entry_points_refuse_bad_arguments():
    ring, src = torch.zeros(C, CAP, device=DEV), torch.zeros(C, 100, device=DEV)
    raw = torch.zeros(100 * C * 2, dtype=torch.uint8, device=DEV)
    for args in ((src, 100, C, 100, ring, CAP, -1), (src, 99, C, 100, ring, CAP, 0), (src, 100, 0, 100, ring, CAP, 0),
                 (src, 100, C, 0, ring, CAP, 0), (src, CAP + 1, C, CAP + 1, ring, CAP, 0), (None, 100, C, 100, ring, CAP, 0)):
        with pytest.raises(RuntimeError, match="status -22"):
            _call("mmd_ring_push", *args)
    for args in ((raw, 100, C, 5, ring, CAP, 0), (raw, 0, C, 2, ring, CAP, 0), (raw, CAP + 1, C, 2, ring, CAP, 0), (raw, 100, C, 2, ring, CAP, -1)):
        with pytest.raises(RuntimeError, match="status -22"):
            _call("mmd_ring_push_pcm", *args)
    f = _front()
    out, ws = torch.zeros(1, 80, 17, C, device=DEV), torch.zeros(C, device=DEV)
    st = torch.zeros(1, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="status -22"):
        f.melspec_windows_ring_into(ring[:, :WIN - 1].contiguous(), st, WIN, True, ws, out)      # win_len > cap
    torch.cuda.synchronize()
    assert float(ring.abs().sum()) == 0.0


# ---------------------------------------------------------------------------------------------- the session
SECOND = "11 shifted"


def _recording(seed):
    """tests/test_gpu_stream.py's stand-in recording; SECOND: the same tones 700 samples later - other windows, other rows, but the
    regime the classifier bias was tuned for (recording 12 gives some 170 rows per window: more live tracks than a TrackConfig holds)"""
    from mm_distillnet_amd.data import synthetic_waveforms
    if seed == SECOND:
        return synthetic_waveforms(24, 11, N_REC + 700)[:, 700:].contiguous()
    return synthetic_waveforms(24, seed, N_REC)


def _quantised(seed):
    """-> (int16 [C, N_REC], the float32 recording int16 / 2^15)"""
    q = torch.clamp(torch.round(_recording(seed) * 32767.0), -32768, 32767).to(torch.int16)
    return q, q.to(torch.float32) / 32768.0


def _state():
    """tests/test_gpu_stream.py's student: make_state's D2 audio net, the classifier bias tuned on the seven windows of recording 11"""
    if "state" not in _CACHE:
        from mm_distillnet_amd.synth import tune_teacher_bias
        spec, st = make_state(COEF, 8, 13, "audio")
        w = _recording(11)
        x = _front().student_input(torch.stack([w[:, k * HOP:k * HOP + WIN] for k in range(7)]).to(DEV), None, S, db=True).cpu()
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


def _track_config():
    from mm_distillnet_amd.tracker import TrackConfig
    return TrackConfig()


def _oracle(seed, tracked, quantised=False):
    """detect_stream / track_stream of the ORACLE detector (never the one a session runs on) on the whole recording, once per case;
    asserted to hold rows in most windows and in the padded group's window"""
    key = ("oracle", seed, tracked, quantised)
    if key not in _CACHE:
        if "oracle_det" not in _CACHE:
            _CACHE["oracle_det"] = _detector()
        det = _CACHE["oracle_det"]
        w = (_quantised(seed)[1] if quantised else _recording(seed)).to(DEV)
        got = det.track_stream(w, WIN, HOP, batch=BATCH, track=_track_config()) if tracked else det.detect_stream(w, WIN, HOP, batch=BATCH)
        per_window = np.bincount(got[1], minlength=7)
        print("oracle", key, "rows per window:", per_window.tolist())
        # most windows give rows, the padded group's one too; recording 11, which the bias was tuned on, stays under the 100 rows the
        # detector tests keep their images under, and every window under the 256 rows the session's record allows it
        assert len(per_window) == 7 and (per_window >= 1).sum() >= 5 and per_window[6] >= 1
        assert per_window.max() <= (100 if seed == 11 else 256)
        if tracked:
            assert (got[2] >= 0).sum() >= 5
        _CACHE[key] = got
    return _CACHE[key]


def _live_detector():
    """ONE detector for the sessions of this file (a new session closes the one before it)"""
    if "live_det" not in _CACHE:
        _CACHE["live_det"] = _detector()
    return _CACHE["live_det"]


def _same(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
        np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32))


def _cut(w, lengths):
    assert sum(lengths) == w.shape[1]
    edges = np.concatenate([[0], np.cumsum(lengths)])
    return [w[:, a:b] for a, b in zip(edges[:-1], edges[1:])]


def _feed(session, chunks, want):
    """pushes, then flush: the concatenation has the oracle's bits; every push returns whole groups in order and only flush the last"""
    parts = [session.push(c) for c in chunks]
    _check(session, parts, want)


def _check(session, parts, want):
    pushed = tuple(np.concatenate([p[i] for p in parts]) for i in range(len(want)))
    assert (pushed[1] < 6).all() and set(pushed[1].tolist()) == set(want[1][want[1] < 6].tolist())
    last = session.flush()
    assert len(last[1]) >= 1 and (last[1] == 6).all()                             # the one-window group appears at flush() only
    _same(tuple(np.concatenate([a, b]) for a, b in zip(pushed, last)), want)
    assert all(len(x) == 0 for x in session.flush())                              # nothing twice


CHUNKINGS = {"one push": ([N_REC], None), "1000 samples": ([1000] * 14, None),
             "irregular": ([1, 2999, 7500, 1, 3499], SPAN)}                       # a 1-sample chunk; 7500 > the ring of one span


@pytest.mark.parametrize("tracked", [False, True])
@pytest.mark.parametrize("chunking", list(CHUNKINGS))
def test_session_equals_the_stream_on_the_whole_recording(chunking, tracked):
    lengths, ring_len = CHUNKINGS[chunking]
    want = _oracle(11, tracked)
    det = _live_detector()
    before = det.live_captures
    session = det.open_stream(WIN, HOP, batch=BATCH, track=_track_config() if tracked else None, ring_len=ring_len)
    assert session.ring_len == (2 * SPAN if ring_len is None else SPAN)
    w = _recording(11)
    chunks = _cut(w, lengths)
    # device chunks (column slices of the recording: src_stride > n) and host chunks alike
    _feed(session, [c.to(DEV) if k % 2 else c for k, c in enumerate(chunks)] if chunking != "one push" else [w.to(DEV)], want)
    assert det.live_captures == before + 1
    # a second, different recording on the same session: no new capture, its own bits
    other = _oracle(SECOND, tracked)
    assert other[0].shape != want[0].shape or not np.array_equal(other[0], want[0])
    session.reset()
    _feed(session, _cut(_recording(SECOND).to(DEV), lengths), other)
    assert det.live_captures == before + 1
    with pytest.raises(RuntimeError, match="flushed"):
        session.push(chunks[0])
    session.close()
    with pytest.raises(RuntimeError, match="closed"):
        session.push(chunks[0])


@pytest.mark.parametrize("tracked", [False, True])
def test_session_fed_pcm_equals_the_stream_on_the_decoded_recording(tracked):
    q, _ = _quantised(11)
    want = _oracle(11, tracked, quantised=True)
    det = _live_detector()
    session = det.open_stream(WIN, HOP, batch=BATCH, track=_track_config() if tracked else None)
    raw = np.ascontiguousarray(q.numpy().T).astype("<i2").tobytes()               # interleaved frames
    parts, at = [], 0
    for k, n in enumerate([1000] * 13 + [999, 1]):
        piece = raw[2 * C * at:2 * C * (at + n)]
        parts.append(session.push_pcm([piece, bytearray(piece), torch.frombuffer(bytearray(piece), dtype=torch.uint8)][k % 3], 2))
        at += n
    assert at == N_REC
    _check(session, parts, want)
    session.reset()
    with pytest.raises(ValueError, match="whole frames"):
        session.push_pcm(raw[:15], 2)
    session.close()


def test_a_group_runs_with_its_last_sample():
    want = _oracle(11, False)
    first = tuple(x[want[1] < BATCH] for x in want)
    assert len(first[0]) >= 1
    w = _recording(11).to(DEV)
    det = _live_detector()
    session = det.open_stream(WIN, HOP, batch=BATCH)
    _same(session.push(w[:, :SPAN]), first)                                       # exactly (BATCH - 1) * HOP + WIN samples
    session.reset()
    got = session.push(w[:, :SPAN - 1])                                           # one fewer: nothing, in the stream's dtypes
    assert got[0].shape == (0, 6) and got[0].dtype == np.float32 and got[1].shape == (0,) and got[1].dtype == np.int32
    _same(session.push(w[:, SPAN - 1:SPAN]), first)                               # the next sample brings them
    assert all(len(x) == 0 for x in session.push(w[:, SPAN:SPAN + 1]))
    session.close()
    assert det._held is None
    with pytest.raises(ValueError, match="ring_len = %d is shorter" % (SPAN - 1)):
        det.open_stream(WIN, HOP, batch=BATCH, ring_len=SPAN - 1)


def test_session_without_a_graph_runs_the_same_chain():
    want = _oracle(11, True)
    det = _detector()
    det.use_graph = False
    session = det.open_stream(WIN, HOP, batch=BATCH, track=_track_config())
    _feed(session, _cut(_recording(11), [1000] * 14), want)
    assert det.live_captures == 0 and det.live_replays == 0
    det.use_graph = True                                                          # the buffers are there: capture, then replay
    session.reset()
    _feed(session, _cut(_recording(11), [1000] * 14), want)
    assert det.live_captures == 1 and det.live_replays == 3
    # a stream on the same detector closes the session
    w = _recording(11).to(DEV)
    _same(det.track_stream(w, WIN, HOP, batch=BATCH, track=_track_config()), want)
    assert session.closed and det._held is None


# ---------------------------------------------------------------------------------------------- detect.py --chunk_s
@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("ext", [".wav", ".npy"])
def test_command_line_tool_writes_the_same_csv_chunked(tmp_path, monkeypatch, ext, track):
    monkeypatch.chdir(tmp_path)
    sys.path.insert(0, ROOT)
    import detect
    spec, st = _state()
    torch.save({"state_dict": st, "epoch": 3}, tmp_path / "student.pth")
    if ext == ".wav":
        with wave.open(str(tmp_path / "rec.wav"), "wb") as w:
            w.setnchannels(C); w.setsampwidth(2); w.setframerate(44100)
            w.writeframes(np.ascontiguousarray(_quantised(11)[0].numpy().T).astype("<i2").tobytes())
    else:
        np.save(tmp_path / "rec.npy", _recording(11).numpy())
    args = ["--config_file", os.path.join(ROOT, "configs", "mm-distillnet.cfg"), "--checkpoint", str(tmp_path / "student.pth"),
            "--input", str(tmp_path / ("rec" + ext)), "--overwrite", '{"image_size": %d}' % S, "--window_s", repr(WIN / 44100),
            "--hop_s", repr(HOP / 44100), "--batch", str(BATCH)] + (["--track"] if track else [])
    whole = detect.main(args + ["--output", str(tmp_path / "whole.csv")])
    chunked = detect.main(args + ["--output", str(tmp_path / "chunked.csv"), "--chunk_s", repr(1000 / 44100)])
    _same(chunked, whole)
    a, b = open(tmp_path / "whole.csv", "rb").read(), open(tmp_path / "chunked.csv", "rb").read()
    assert a == b and a.count(b"\n") > 10 and len(np.unique(whole[1])) >= 5
