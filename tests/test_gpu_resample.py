"""Resampling on the GPU: mmd_resample_poly against the float64 restatement (tests/resample_ref.py) with the sequential host-float32
run of the same rule as the yardstick, its reproducibility in dirty buffers, mmd_pcm_to_float against the numpy formula bit for bit, a
three-tone signal against its analytic resample, and detect.py --resample / --sample_rate against AudioDetector on the resampled tensor,
bit for bit.  The small detector is the one of tests/test_gpu_stream.py (D2 at 128 x 128), its classifier bias tuned on this file's
recording."""
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
LENGTHS = (50, 1000, 4097)                             # shorter than the filter; no multiple of a period; across tile ends
ROWS = 16                                              # batch 2 x 8 microphones
_CACHE = {}


def _rs():
    from mm_distillnet_amd.audio import Resampler
    if "rs" not in _CACHE:
        _CACHE["rs"] = Resampler(DEV)
    return _CACHE["rs"]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _case(sr, n_in):
    """seeded normal input [16, n_in] with its float64 and sequential-float32 restatements, computed once"""
    if (sr, n_in) not in _CACHE:
        x = np.random.default_rng(sr + n_in).standard_normal((ROWS, n_in)).astype(np.float32)
        ref = R.resample_ref(x, sr, dtype=np.float64)
        ref.setflags(write=False)
        host = R.resample_ref(x, sr, dtype=np.float32)
        _CACHE[sr, n_in] = (x, ref, host)
    return _CACHE[sr, n_in]


# ---------------------------------------------------------------------------------------------- kernel against float64
@pytest.mark.parametrize("rows", [1, ROWS])
@pytest.mark.parametrize("n_in", LENGTHS)
@pytest.mark.parametrize("sr", RATES)
def test_kernel_against_float64(sr, n_in, rows):
    """max|d| / max|ref| of the kernel at most 4 x the figure of the host's sequential float32 run on the same input (the factor
    tests/test_gpu_melspec.py grants another summation order and fused multiply-adds)."""
    x, ref, host = _case(sr, n_in)
    x, ref, host = x[:rows], ref[:rows], host[:rows]
    shape = (2, 8, n_in) if rows == ROWS else (n_in,)
    got = _rs().resample(torch.from_numpy(x).reshape(shape).to(DEV), sr)
    L, M = R.ratio(sr, 44100)
    assert got.shape == shape[:-1] + (R.n_out(n_in, L, M),) and got.dtype == torch.float32
    got = got.cpu().numpy().reshape(rows, -1).astype(np.float64)
    scale = np.abs(ref).max()
    e_gpu, e_host = np.abs(got - ref).max() / scale, np.abs(host.astype(np.float64) - ref).max() / scale
    print("resample %6d -> 44100  n_in %4d rows %2d  L/M %d/%d taps %d: kernel %.3e  host float32 %.3e" %
          (sr, n_in, rows, L, M, 2 * R.half_len(L, M), e_gpu, e_host))
    assert np.isfinite(got).all() and e_host > 0.0
    assert e_gpu <= 4.0 * e_host


# ---------------------------------------------------------------------------------------------- reproducibility
@pytest.mark.parametrize("rows", [1, ROWS])
@pytest.mark.parametrize("sr", [48000, 16000, 192000])
def test_dirty_buffers_give_the_same_bits_and_the_tail_is_untouched(sr, rows):
    from mm_distillnet_amd import _lib
    n_in, tail = 4097, 333
    x, ref, _ = _case(sr, n_in)
    xd = torch.from_numpy(x[:rows]).to(DEV)
    L, M, taps, bank, off = _rs()._bank(sr, 44100)
    n_out = R.n_out(n_in, L, M)
    outs = []
    for fill in (float("nan"), -7.5e8):
        buf = torch.full((rows * n_out + tail,), fill, device=DEV)
        _lib.call("mmd_resample_poly", xd, rows, n_in, bank, off, L, M, taps, buf, n_out)
        y, behind = buf[:rows * n_out], buf[rows * n_out:]
        assert torch.isfinite(y).all()
        assert torch.equal(_bits(behind), _bits(torch.full((tail,), fill, device=DEV)))
        outs.append(y.clone())
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    assert torch.equal(_bits(outs[0].view(rows, n_out)), _bits(_rs().resample(xd, sr)))
    # (and they are the right samples: the bound of test_kernel_against_float64 is held there; here only that nothing is off by a row)
    np.testing.assert_allclose(outs[0].view(rows, n_out).cpu().numpy(), ref[:rows], atol=1e-4)


def test_same_rate_returns_the_input_without_a_launch():
    from mm_distillnet_amd.audio import Resampler
    rs = Resampler(DEV)

    def no_launch(*a):
        raise AssertionError("a launch for sr_in == sr_out")

    rs.call = no_launch
    x = torch.randn(2, 8, 777, device=DEV)
    keep = x.clone()
    y = rs.resample(x, 44100)
    assert y is x and torch.equal(_bits(y), _bits(keep)) and rs._banks == {}
    assert rs.resample(x, 48000, 48000) is x


def test_resample_refuses_what_the_kernel_does_not_take():
    rs = _rs()
    with pytest.raises(ValueError, match="contiguous float32"):
        rs.resample(torch.zeros(8, 100, device=DEV, dtype=torch.float64), 48000)
    with pytest.raises(ValueError, match="contiguous float32"):
        rs.resample(torch.zeros(100, 8, device=DEV).t(), 48000)
    with pytest.raises(ValueError, match="44100 / 44101"):
        rs.resample(torch.zeros(8, 100, device=DEV), 44101)
    with pytest.raises(ValueError, match="uint8"):
        rs.pcm_to_float(torch.zeros(99, dtype=torch.uint8, device=DEV), 50, 1, 2)
    with pytest.raises(ValueError, match="contiguous uint8"):
        rs.pcm_to_float(torch.zeros(200, dtype=torch.uint8, device=DEV)[::2], 50, 1, 2)
    with pytest.raises(ValueError, match="the tensor is on cpu"):                 # a host pointer never reaches a kernel
        rs.resample(torch.zeros(8, 100), 48000)
    with pytest.raises(ValueError, match="the tensor is on cpu"):
        rs.pcm_to_float(torch.zeros(100, dtype=torch.uint8), 50, 1, 2)


# ---------------------------------------------------------------------------------------------- PCM decoding
def _pcm_bytes(samples, width):
    le = samples.astype("<i8").view(np.uint8).reshape(samples.shape[0], samples.shape[1], 8)[:, :, :width]
    return np.ascontiguousarray(le).reshape(-1)


@pytest.mark.parametrize("frames", [1, 1025])
@pytest.mark.parametrize("channels", [8, 1])
@pytest.mark.parametrize("width", [2, 3, 4])
def test_pcm_to_float_equals_the_numpy_formula(width, channels, frames):
    top = 1 << (8 * width - 1)
    s = np.random.default_rng(100 * width + channels).integers(-top, top, (frames, channels))
    edge = [-top, top - 1, 0, 1, -1, top - 2, -top + 1, (1 << 24) + 1 if width == 4 else 3]      # 2^24 + 1: (float)i has to round
    flat = s.reshape(-1)
    flat[:min(len(edge), flat.size)] = edge[:flat.size]
    if frames > 1:
        s[-1, -1], s[-2, 0] = -top, top - 1
    want = torch.from_numpy(np.ascontiguousarray((s.astype(np.int32).astype(np.float32) / np.float32(top)).T))
    raw = _pcm_bytes(s, width)
    got = _rs().pcm_to_float(torch.from_numpy(raw).to(DEV), frames, channels, width)
    assert got.shape == (channels, frames) and got.dtype == torch.float32
    assert torch.equal(_bits(got.cpu()), _bits(want))
    # a buffer that starts at an odd address, 0xFF bytes around it
    guard = np.full(raw.size + 8, 0xFF, np.uint8)
    guard[1:1 + raw.size] = raw
    odd = torch.from_numpy(guard).to(DEV)[1:1 + raw.size]
    assert odd.data_ptr() % 2 == 1 and odd.is_contiguous()
    assert torch.equal(_bits(_rs().pcm_to_float(odd, frames, channels, width).cpu()), _bits(want))


# ---------------------------------------------------------------------------------------------- tones
def test_three_tones_against_their_analytic_resample():
    """Three tones below 0.4 * 44100 Hz written down at 48 kHz and at 44.1 kHz; the device's resample of the first against the second,
    `half` outputs away from both ends.  Bound: the float64 restatement's own error on this input (the rule's pass-band ripple and the
    float32 rounding of the input and the bank) plus the float32 allowance of test_kernel_against_float64, four times the sequential
    host-float32 run's distance from the float64 restatement.  Nothing is fixed here; the figures are printed."""
    tones = ((997.0, 0.5, 0.3), (7321.0, 0.3, 1.1), (16789.0, 0.2, 2.5))                         # Hz, amplitude, phase
    assert max(f for f, _, _ in tones) < 0.4 * 44100
    n_in = 9600
    L, M = R.ratio(48000, 44100)
    half, n_out = R.half_len(L, M), R.n_out(n_in, L, M)

    def signal(n, sr):
        t = np.arange(n, dtype=np.float64) / sr
        return sum(a * np.sin(2 * np.pi * f * t + ph) for f, a, ph in tones)

    x = signal(n_in, 48000).astype(np.float32)
    want = signal(n_out, 44100)
    inner = slice(half, n_out - half)
    ref, host = R.resample_ref(x, 48000), R.resample_ref(x, 48000, dtype=np.float32).astype(np.float64)
    got = _rs().resample(torch.from_numpy(x).to(DEV), 48000).cpu().numpy().astype(np.float64)
    e_ref, e_host = np.abs(ref - want)[inner].max(), np.abs(host - ref)[inner].max()
    e_gpu = np.abs(got - want)[inner].max()
    print("three tones 48000 -> 44100: device %.3e  float64 restatement %.3e  host float32 against it %.3e  bound %.3e" %
          (e_gpu, e_ref, e_host, e_ref + 4.0 * e_host))
    assert e_gpu <= e_ref + 4.0 * e_host


# ---------------------------------------------------------------------------------------------- detect.py
S, COEF, C = 128, 2, 8
N48 = 28800                                            # 0.6 s at 48 kHz -> 26460 samples at 44.1 kHz
WINDOW_S, HOP_S = 0.25, 0.125                          # 11025 and 5512 samples: 3 windows


def _pcm48():
    """the detector tests' stand-in recording written down at 48 kHz, as 16-bit frames [N48, 8]"""
    from mm_distillnet_amd.data import synthetic_waveforms
    w = synthetic_waveforms(24, 21, N48, sr=48000).numpy()
    return np.clip(np.rint(w * 0.5 * 32768.0), -32768, 32767).astype(np.int16).T.copy()


def _wav44():
    """[8, 26460] on the device: what --resample makes of the file"""
    if "wav44" not in _CACHE:
        pcm = _pcm48()
        raw = torch.from_numpy(pcm.view(np.uint8).reshape(-1).copy()).to(DEV)
        _CACHE["wav44"] = _rs().resample(_rs().pcm_to_float(raw, N48, C, 2), 48000)
    return _CACHE["wav44"]


def _state(kind):
    """(spec, state) of tests/test_gpu_stream.py's small student, its classifier bias shifted - as that file does on its own windows - so
    that the images the test feeds give about 40 candidates each at the default confidence threshold: kind "clip" on the whole resampled
    recording as one clip, kind "stream" on its three windows"""
    if ("state", kind) not in _CACHE:
        from mm_distillnet_amd.audio import MelFrontEnd
        from mm_distillnet_amd.synth import tune_teacher_bias
        spec, st = make_state(COEF, 8, 13, "audio")
        w = _wav44()
        clips = w[None] if kind == "clip" else torch.stack([w[:, k * 5512:k * 5512 + 11025] for k in range(3)])
        # (one image has few anchors whose best class is the one the tuning counts: a smaller target for the single clip)
        tune_teacher_bias(spec, st, MelFrontEnd(DEV).student_input(clips.contiguous(), None, S, db=True).cpu(), DEV, 10 if kind == "clip" else 40)
        _CACHE["state", kind] = (spec, st)
    spec, st = _CACHE["state", kind]
    return spec, {k: v.clone() for k, v in st.items()}


def _detector(kind):
    from mm_distillnet_amd.detector import AudioDetector
    spec, st = _state(kind)
    det = AudioDetector(spec, DEV, image_size=S)
    det.load(st)
    return det


def _files(tmp_path, kind):
    spec, st = _state(kind)
    torch.save({"state_dict": st, "epoch": 3}, tmp_path / "student.pth")
    pcm = _pcm48()
    with wave.open(str(tmp_path / "rec48.wav"), "wb") as w:
        w.setnchannels(C); w.setsampwidth(2); w.setframerate(48000)
        w.writeframes(pcm.astype("<i2").tobytes())
    np.save(tmp_path / "rec48.npy", np.ascontiguousarray(pcm.T.astype(np.float32) / np.float32(32768.0)))
    return ["--config_file", os.path.join(ROOT, "configs", "mm-distillnet.cfg"), "--checkpoint", str(tmp_path / "student.pth"),
            "--output", str(tmp_path / "out.csv"), "--overwrite", '{"image_size": %d}' % S]


def _detect():
    sys.path.insert(0, ROOT)
    import detect
    return detect


def _clip_rows():
    if "clip_rows" not in _CACHE:
        det = _detector("clip")
        rows = det.detect(_wav44()[None].contiguous())
        det.check_overflow()
        _CACHE["clip_rows"] = rows
    return _CACHE["clip_rows"]


def test_resampled_recording_has_the_expected_shape():
    w = _wav44()
    assert w.shape == (C, 26460) and w.dtype == torch.float32 and torch.isfinite(w).all()
    assert 0.1 < float(w.abs().max()) < 1.0


@pytest.mark.parametrize("source", ["wav", "npy"])
def test_command_line_clip_equals_detect_on_the_resampled_tensor(tmp_path, monkeypatch, capsys, source):
    monkeypatch.chdir(tmp_path)
    args = _files(tmp_path, "clip")
    want = _clip_rows()
    print("clip rows:", want[0].shape[0])
    assert len(want) == 1
    extra = ["--input", str(tmp_path / "rec48.wav"), "--resample"] if source == "wav" else \
            ["--input", str(tmp_path / "rec48.npy"), "--sample_rate", "48000"]
    rows = _detect().main(args + extra)
    assert len(rows) == 1 and rows[0].shape == want[0].shape
    np.testing.assert_array_equal(np.asarray(rows[0], np.float32).view(np.int32), np.asarray(want[0], np.float32).view(np.int32))
    assert capsys.readouterr().out.strip().split("\n")[-1] == "1 clips, %d boxes -> %s" % (len(want[0]), tmp_path / "out.csv")


def test_command_line_stream_equals_detect_stream_on_the_resampled_tensor(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    args = _files(tmp_path, "stream")
    win_len, hop = int(round(WINDOW_S * 44100)), int(round(HOP_S * 44100))
    assert (win_len, hop) == (11025, 5512)
    want_rows, want_win = _detector("stream").detect_stream(_wav44(), win_len, hop, batch=8)
    print("stream rows per window:", np.bincount(want_win, minlength=3).tolist())
    assert set(want_win.tolist()) <= {0, 1, 2}
    rows, window = _detect().main(args + ["--input", str(tmp_path / "rec48.wav"), "--resample", "--window_s", repr(WINDOW_S), "--hop_s",
                                          repr(HOP_S)])
    np.testing.assert_array_equal(rows.view(np.int32), want_rows.view(np.int32))
    np.testing.assert_array_equal(window, want_win)
    assert capsys.readouterr().out.strip().split("\n")[-1] == "3 windows, %d boxes -> %s" % (len(want_rows), tmp_path / "out.csv")
    lines = open(tmp_path / "out.csv").read().strip().split("\n")
    assert lines[0] == "window,t_start_s,x1,y1,x2,y2,score,label" and len(lines) == 1 + len(want_rows)
    assert [ln.split(",")[1] for ln in lines[1:]] == ["%.9g" % (int(w) * hop / 44100) for w in want_win]      # seconds of the recording


def test_without_the_flags_the_48_khz_file_is_still_refused(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    args = _files(tmp_path, "clip")
    with pytest.raises(ValueError, match="48000 Hz is not supported"):
        _detect().main(args + ["--input", str(tmp_path / "rec48.wav")])
