"""Live streaming detection at any sample rate on the GPU: mmd_ring_resample against mmd_resample_poly on the whole input, bit for bit,
fed through rings that wrap, at positions beyond 2^31 and against the float64 restatement (tests/resample_ref.py); a LiveSession opened
with sample_rate=48000 and detect.py --live_s against detect_stream / track_stream of a SECOND detector on the whole resampled
recording, bit for bit, for several ways of cutting the recording into chunks.  The small detector and its bias tuning are those of
tests/test_gpu_live.py, restated on this file's 48 kHz recording."""
import os
import sys
import wave

import numpy as np
import pytest
import torch

import resample_ref as R
from helpers import make_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = (48000, 16000, 22050, 96000, 192000)          # L / M = 147/160, 441/160, 2/1, 147/320, 147/640: taps 140, 128, 128, 280, 558
ROWS, N_IN, OUT_CAP = 8, 4097, 1531
S, COEF, C = 128, 2, 8
SR, N48, N_REC = 48000, 15238, 14000                   # ceil(15238 * 147 / 160) = 14000 samples at 44.1 kHz
WIN, HOP, BATCH = 4096, 1531, 3                        # W = 1 + (14000 - 4096) // 1531 = 7: two full groups, one of one window
SPAN = (BATCH - 1) * HOP + WIN                         # 7158 samples: one group
IN_MIN = 140 + 160 + 1                                 # the smallest input ring at 48 kHz: taps + M + 1
_CACHE = {}


def _rs():
    from mm_distillnet_amd.audio import Resampler
    if "rs" not in _CACHE:
        _CACHE["rs"] = Resampler(DEV)
    return _CACHE["rs"]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _call(name, *args):
    from mm_distillnet_amd import _lib
    return _lib.call(name, *args)


def _case(sr):
    """seeded normal input [8, 4097] on the device and mmd_resample_poly of the whole of it, computed once"""
    if ("case", sr) not in _CACHE:
        x = np.random.default_rng(sr + N_IN).standard_normal((ROWS, N_IN)).astype(np.float32)
        xd = torch.from_numpy(x).to(DEV)
        want = _rs().resample(xd, sr)
        assert want.shape == (ROWS, R.n_out(N_IN, *R.ratio(sr, 44100))) and torch.isfinite(want).all()
        _CACHE["case", sr] = (x, xd, want)
    return _CACHE["case", sr]


def _oldest(t, L, M, half):
    return (t * M) // L - half + 1


# ---------------------------------------------------------------------------------------------- kernel bits against the offline kernel
@pytest.mark.parametrize("fill", [float("nan"), -7.5e8])
@pytest.mark.parametrize("sr,out_cap", [(sr, OUT_CAP) for sr in RATES] + [(192000, 257)])      # 941 outputs never lap a ring of 1531
def test_ring_kernel_equals_the_offline_kernel_bit_for_bit(sr, out_cap, fill):
    """The input goes through the smallest input ring the session allows, plus one slot, in uneven pieces - each as long as the
    oldest pending output's first tap allows, or shorter - and after each piece the ready outputs are computed in uneven sub-ranges.
    After EVERY call the output ring holds the offline kernel's bits in the slots written so far and the fill everywhere else."""
    from mm_distillnet_amd.audio import live_in_ring_min, live_resample_ready
    _, xd, want = _case(sr)
    L, M, taps, bank, off = _rs()._bank(sr, 44100)
    half, n_out = taps // 2, want.shape[1]
    in_cap = live_in_ring_min(L, M, half) + 1
    assert in_cap == taps + M + 2
    in_ring = torch.full((ROWS, in_cap), fill, device=DEV)
    out_ring = torch.full((ROWS, out_cap), fill, device=DEV)
    expect = out_ring.clone()
    pushed = produced = calls = 0
    seen = dict(one=0, out_wrap=0, in_wrap=0, first=0, final=0, in_laps=0)

    def produce(ready, n_valid, final):
        nonlocal produced, calls
        k = 0
        while produced < ready:
            t_lo, t_hi = produced, min(ready, produced + (1, 5, 2, 64, 3, out_cap)[k % 6])
            k += 1
            _call("mmd_ring_resample", in_ring, in_cap, ROWS, n_valid, bank, off, L, M, taps, out_ring, out_cap, t_lo, t_hi)
            slots = torch.arange(t_lo, t_hi, device=DEV) % out_cap
            expect[:, slots] = want[:, t_lo:t_hi]
            assert torch.equal(_bits(out_ring), _bits(expect)), (sr, t_lo, t_hi, n_valid)
            lo_in, hi_in = _oldest(t_lo, L, M, half), _oldest(t_hi - 1, L, M, half) + taps - 1
            seen["one"] += t_hi - t_lo == 1
            seen["out_wrap"] += t_lo % out_cap > (t_hi - 1) % out_cap
            seen["in_wrap"] += lo_in >= 0 and hi_in < n_valid and lo_in % in_cap > hi_in % in_cap
            seen["first"] += t_lo == 0 and lo_in < 0
            seen["final"] += final and hi_in >= n_valid
            calls += 1
            produced = t_hi

    k = 0
    while pushed < N_IN:
        # the longest piece that leaves the first tap of output `produced` in the ring, every other time a shorter one
        room = _oldest(produced, L, M, half) + in_cap - pushed
        assert room >= in_cap - taps - M                                             # the session's piece always fits
        n = min(N_IN - pushed, room if k % 2 == 0 else 1 + (7 * k) % room)
        k += 1
        _call("mmd_ring_push", xd.data_ptr() + 4 * pushed, N_IN, ROWS, n, in_ring, in_cap, pushed)
        pushed += n
        produce(live_resample_ready(pushed, L, M, half), pushed, False)
    assert produced == live_resample_ready(N_IN, L, M, half) < n_out
    produce(live_resample_ready(N_IN, L, M, half, final=True), N_IN, True)
    assert produced == n_out
    seen["in_laps"] = N_IN // in_cap
    print("ring resample %6d: in_cap %d, %d pieces, %d calls, %s" % (sr, in_cap, k, calls, seen))
    assert seen["one"] >= 1 and seen["first"] >= 1 and seen["final"] >= 1 and seen["in_wrap"] >= 1 and seen["in_laps"] >= 2
    assert seen["out_wrap"] >= 1 or (n_out <= out_cap and (sr, out_cap) == (192000, OUT_CAP))      # that rate has its own smaller ring


@pytest.mark.parametrize("sr", RATES)
def test_positions_beyond_2_31_give_the_bits_of_the_unshifted_range(sr):
    """An interior range - no tap before the recording or behind its end - at its own positions and with every absolute position moved
    by 2^31 periods (inputs by 2^31 * M, outputs by 2^31 * L): the same inputs under the same taps, so the same bits."""
    from mm_distillnet_amd.audio import live_resample_ready
    _, xd, want = _case(sr)
    L, M, taps, bank, off = _rs()._bank(sr, 44100)
    half, q = taps // 2, 1 << 31
    t0 = -((-(half - 1) * L) // M)
    t1 = min(live_resample_ready(N_IN, L, M, half), t0 + OUT_CAP)
    assert _oldest(t0, L, M, half) >= 0 and _oldest(t0 - 1, L, M, half) < 0 and t1 - t0 > 300
    in_cap = 4099                                                                     # the whole input is resident, at odd slots
    for shift_in, shift_out in ((0, 0), (q * M, q * L)):
        in_ring = torch.full((ROWS, in_cap), float("nan"), device=DEV)
        out_ring = torch.full((ROWS, OUT_CAP), float("nan"), device=DEV)
        _call("mmd_ring_push", xd, N_IN, ROWS, N_IN, in_ring, in_cap, shift_in)
        _call("mmd_ring_resample", in_ring, in_cap, ROWS, shift_in + N_IN, bank, off, L, M, taps, out_ring, OUT_CAP, shift_out + t0,
              shift_out + t1)
        expect = torch.full((ROWS, OUT_CAP), float("nan"), device=DEV)
        slots = (shift_out + torch.arange(t0, t1, dtype=torch.int64, device=DEV)) % OUT_CAP
        expect[:, slots] = want[:, t0:t1]
        assert torch.equal(_bits(out_ring), _bits(expect)), (sr, shift_in)
    assert q * M >= 1 << 31 and q * L >= 1 << 31                                      # no position fits an int32


@pytest.mark.parametrize("sr", [48000, 192000])
def test_ring_kernel_against_float64(sr):
    """tests/test_gpu_resample.py's rule for the offline kernel, held by the ring kernel on its own: max|d| / max|ref| at most 4 x the
    figure of the host's sequential float32 run on the same input."""
    x, xd, _ = _case(sr)
    L, M, taps, bank, off = _rs()._bank(sr, 44100)
    n_out = R.n_out(N_IN, L, M)
    in_cap = N_IN + taps // 2                          # the range starts at input -(taps / 2 - 1): the rule counts those zeros as inputs
    in_ring = torch.full((ROWS, in_cap), float("nan"), device=DEV)
    out_ring = torch.full((ROWS, n_out), float("nan"), device=DEV)
    _call("mmd_ring_push", xd, N_IN, ROWS, N_IN, in_ring, in_cap, 0)
    _call("mmd_ring_resample", in_ring, in_cap, ROWS, N_IN, bank, off, L, M, taps, out_ring, n_out, 0, n_out)    # the recording ends at N_IN
    got = out_ring.cpu().numpy().astype(np.float64)
    ref, host = R.resample_ref(x, sr, dtype=np.float64), R.resample_ref(x, sr, dtype=np.float32)
    scale = np.abs(ref).max()
    e_gpu, e_host = np.abs(got - ref).max() / scale, np.abs(host.astype(np.float64) - ref).max() / scale
    print("ring resample %6d -> 44100 against float64: kernel %.3e  host float32 %.3e" % (sr, e_gpu, e_host))
    assert np.isfinite(got).all() and e_host > 0.0
    assert e_gpu <= 4.0 * e_host


def test_ring_resample_refuses_an_overwritten_range_on_the_device_too():
    _, xd, _ = _case(48000)
    L, M, taps, bank, off = _rs()._bank(48000, 44100)
    in_ring, out_ring = torch.zeros(ROWS, 302, device=DEV), torch.zeros(ROWS, OUT_CAP, device=DEV)
    for args in ((in_ring, 302, ROWS, 1000, bank, off, L, M, taps, out_ring, OUT_CAP, 0, 10),          # input 0 left the ring long ago
                 (in_ring, 192, ROWS, 100, bank, off, L, M, taps, out_ring, OUT_CAP, 0, 10),           # below the least staged span
                 (in_ring, 302, ROWS, 100, bank, off, L, M, taps, out_ring, OUT_CAP, 0, OUT_CAP + 1)):
        with pytest.raises(RuntimeError, match="status -22"):
            _call("mmd_ring_resample", *args)
    torch.cuda.synchronize()
    assert float(out_ring.abs().sum()) == 0.0


# ---------------------------------------------------------------------------------------------- the session
SECOND = "11 shifted"


def _front():
    from mm_distillnet_amd.audio import MelFrontEnd
    if "front" not in _CACHE:
        _CACHE["front"] = MelFrontEnd(DEV)
    return _CACHE["front"]


def _recording48(seed):
    """tests/test_gpu_live.py's stand-in recording written down at 48 kHz; SECOND: the same tones 762 samples (700 at 44.1 kHz) later"""
    from mm_distillnet_amd.data import synthetic_waveforms
    if seed == SECOND:
        return synthetic_waveforms(24, 11, N48 + 762, sr=SR)[:, 762:].contiguous()
    return synthetic_waveforms(24, seed, N48, sr=SR)


def _quantised48(seed):
    """-> (24-bit samples as int32 [C, N48], their interleaved little-endian frames as bytes)"""
    q = torch.clamp(torch.round(_recording48(seed).to(torch.float64) * 8388607.0), -8388608, 8388607).to(torch.int32)
    le = np.ascontiguousarray(q.numpy().T).astype("<i4").view(np.uint8).reshape(N48, C, 4)[:, :, :3]
    return q, np.ascontiguousarray(le).tobytes()


def _resampled(seed, quantised=False):
    """[8, 14000] on the device: Resampler.resample of the WHOLE recording (of its decoded 24-bit frames: quantised)"""
    key = ("resampled", seed, quantised)
    if key not in _CACHE:
        if quantised:
            raw = torch.frombuffer(bytearray(_quantised48(seed)[1]), dtype=torch.uint8).to(DEV)
            w = _rs().pcm_to_float(raw, N48, C, 3)
        else:
            w = _recording48(seed).to(DEV)
        _CACHE[key] = _rs().resample(w, SR)
        assert _CACHE[key].shape == (C, N_REC)
    return _CACHE[key]


def _state():
    """tests/test_gpu_live.py's student: make_state's D2 audio net, the classifier bias tuned on the seven windows of the resampled
    recording 11"""
    if "state" not in _CACHE:
        from mm_distillnet_amd.synth import tune_teacher_bias
        spec, st = make_state(COEF, 8, 13, "audio")
        w = _resampled(11)
        x = _front().student_input(torch.stack([w[:, k * HOP:k * HOP + WIN] for k in range(7)]).contiguous(), None, S, db=True).cpu()
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
    """detect_stream / track_stream of the ORACLE detector (never the one a session runs on) on the whole resampled recording, once
    per case; asserted to hold rows in most windows and in the padded group's window: equality of empty results would show nothing"""
    key = ("oracle", seed, tracked, quantised)
    if key not in _CACHE:
        if "oracle_det" not in _CACHE:
            _CACHE["oracle_det"] = _detector()
        det = _CACHE["oracle_det"]
        w = _resampled(seed, quantised)
        got = det.track_stream(w, WIN, HOP, batch=BATCH, track=_track_config()) if tracked else det.detect_stream(w, WIN, HOP, batch=BATCH)
        per_window = np.bincount(got[1], minlength=7)
        print("oracle", key, "rows per window:", per_window.tolist())
        assert len(per_window) == 7 and (per_window >= 1).sum() >= 5 and per_window[6] >= 1
        assert per_window.max() <= 256                                                # what the session's record allows a window
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


def _finish(session, parts, want):
    """pushes, then flush: the concatenation has the oracle's bits, in window order; the one-window group comes with flush() only"""
    pushed = tuple(np.concatenate([p[i] for p in parts]) for i in range(len(want)))
    assert (pushed[1] < 6).all()
    last = session.flush()
    assert len(last[1]) >= 1 and (last[1] == 6).sum() >= 1
    _same(tuple(np.concatenate([a, b]) for a, b in zip(pushed, last)), want)
    assert all(len(x) == 0 for x in session.flush())                                  # nothing twice


CHUNKINGS = {"one push": ([N48], None, None), "1000 samples": ([1000] * 15 + [238], None, None),
             "irregular": ([1, 3299, 8200, 1, 3737], SPAN, IN_MIN)}                   # 8200 > both rings: written and resampled in pieces


@pytest.mark.parametrize("tracked", [False, True])
@pytest.mark.parametrize("chunking", list(CHUNKINGS))
def test_session_at_48_khz_equals_the_stream_on_the_resampled_recording(chunking, tracked):
    lengths, ring_len, in_ring_len = CHUNKINGS[chunking]
    want = _oracle(11, tracked)
    det = _live_detector()
    before = det.live_captures
    session = det.open_stream(WIN, HOP, batch=BATCH, track=_track_config() if tracked else None, ring_len=ring_len, sample_rate=SR,
                              in_ring_len=in_ring_len)
    assert session.ring_len == (2 * SPAN if ring_len is None else SPAN)
    assert session.in_ring_len == (IN_MIN if in_ring_len else 140 + 160 - ((-2 * SPAN * 160) // 147))
    assert session.in_ring.shape == (C, session.in_ring_len)
    w = _recording48(11)
    chunks = _cut(w, lengths)
    # device chunks (column slices of the recording: src_stride > n) and host chunks alike
    fed = [c.to(DEV) if k % 2 else c for k, c in enumerate(chunks)] if chunking != "one push" else [w.to(DEV)]
    _finish(session, [session.push(c) for c in fed], want)
    assert det.live_captures == before + 1
    # a second, different recording on the same session: no new capture, its own bits
    other = _oracle(SECOND, tracked)
    assert other[0].shape != want[0].shape or not np.array_equal(other[0], want[0])
    session.reset()
    assert session.in_written == 0 and session.written == 0
    _finish(session, [session.push(c) for c in _cut(_recording48(SECOND).to(DEV), lengths)], other)
    assert det.live_captures == before + 1
    with pytest.raises(RuntimeError, match="flushed"):
        session.push(chunks[0])
    session.close()


@pytest.mark.parametrize("tracked", [False, True])
def test_session_fed_24_bit_pcm_equals_the_stream_on_the_decoded_resampled_recording(tracked):
    _, raw = _quantised48(11)
    want = _oracle(11, tracked, quantised=True)
    det = _live_detector()
    session = det.open_stream(WIN, HOP, batch=BATCH, track=_track_config() if tracked else None, sample_rate=SR)
    parts, fb = [], 3 * C
    for k, at in enumerate(range(0, N48, 1000)):
        piece = raw[fb * at:fb * min(at + 1000, N48)]
        parts.append(session.push_pcm([piece, bytearray(piece), torch.frombuffer(bytearray(piece), dtype=torch.uint8)][k % 3], 3))
    _finish(session, parts, want)
    session.close()


def test_sessions_at_44100_and_without_a_rate_are_the_44_1_khz_session():
    """sample_rate=44100 and sample_rate=None: no input ring, no resampling launch, and the same bits as each other and as the stream"""
    det = _live_detector()
    w = _resampled(11)                                                               # any 44.1 kHz recording: this one has rows
    want = _oracle(11, False)
    got = []
    for rate in (None, 44100):
        session = det.open_stream(WIN, HOP, batch=BATCH, sample_rate=rate)
        assert session.in_ring is None and session.in_ring_len is None and session.rs is None
        called = []
        if det.resampler is not None:
            keep = det.resampler.call
            det.resampler.call = lambda name, *a: called.append(name) or keep(name, *a)
        parts = [session.push(c) for c in _cut(w, [1000] * 14)]
        parts.append(session.flush())
        if det.resampler is not None:
            det.resampler.call = keep
        assert called == []
        got.append(tuple(np.concatenate([p[i] for p in parts]) for i in range(2)))
        session.close()
    _same(got[0], got[1])
    _same(got[0], want)


# ---------------------------------------------------------------------------------------------- detect.py --live_s
@pytest.mark.parametrize("track", [False, True])
@pytest.mark.parametrize("ext", [".wav", ".npy"])
def test_command_line_tool_writes_the_same_csv_live(tmp_path, monkeypatch, ext, track):
    monkeypatch.chdir(tmp_path)
    sys.path.insert(0, ROOT)
    import detect
    spec, st = _state()
    torch.save({"state_dict": st, "epoch": 3}, tmp_path / "student.pth")
    if ext == ".wav":
        with wave.open(str(tmp_path / "rec.wav"), "wb") as w:
            w.setnchannels(C); w.setsampwidth(3); w.setframerate(SR)
            w.writeframes(_quantised48(11)[1])
        whole_flags, live_flags = ["--resample"], []
    else:
        np.save(tmp_path / "rec.npy", _recording48(11).numpy())
        whole_flags = live_flags = ["--sample_rate", str(SR)]
    args = ["--config_file", os.path.join(ROOT, "configs", "mm-distillnet.cfg"), "--checkpoint", str(tmp_path / "student.pth"),
            "--input", str(tmp_path / ("rec" + ext)), "--overwrite", '{"image_size": %d}' % S, "--window_s", repr(WIN / 44100),
            "--hop_s", repr(HOP / 44100), "--batch", str(BATCH)] + (["--track"] if track else [])
    whole = detect.main(args + whole_flags + ["--output", str(tmp_path / "whole.csv")])
    live = detect.main(args + live_flags + ["--output", str(tmp_path / "live.csv"), "--live_s", "0.05"])
    _same(live, whole)
    a, b = open(tmp_path / "whole.csv", "rb").read(), open(tmp_path / "live.csv", "rb").read()
    assert a == b and a.count(b"\n") > 10 and len(np.unique(whole[1])) >= 5
