"""Resampling, CPU side: the restatement (tests/resample_ref.py) against the direct definition and closed forms, the host bank of
mm_distillnet_amd.audio.resample_bank against the restatement's, the C ABI of the two entry points without a GPU, detect.py's raw
WAV reader."""
import ctypes
import os
import sys
import wave

import numpy as np
import pytest

import resample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = (48000, 16000, 22050, 32000, 96000, 192000)
TAPS = {48000: (147, 160, 140), 16000: (441, 160, 128), 22050: (2, 1, 128), 32000: (441, 320, 128), 96000: (147, 320, 280),
        192000: (147, 640, 558)}


def _detect():
    sys.path.insert(0, ROOT)
    import detect
    return detect


# ---------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("sr", RATES)
def test_ratio_taps_and_phase_sums(sr):
    L, M = R.ratio(sr, 44100)
    b = R.bank(L, M)
    assert (L, M, b.shape[1]) == TAPS[sr] and b.shape == (L, 2 * R.half_len(L, M)) and b.dtype == np.float32
    sums = b.astype(np.float64).sum(1)
    print(sr, "phase sums within", np.abs(sums - 1.0).max())
    assert np.abs(sums - 1.0).max() < 1e-7
    # phase 0 sits on an input sample: its largest tap is the centre one, k = 0
    assert b[0].argmax() == R.half_len(L, M) - 1


@pytest.mark.parametrize("sr", [48000, 16000])
def test_restatement_equals_the_direct_definition(sr):
    x = np.random.default_rng(sr).standard_normal(300).astype(np.float32)
    got, want = R.resample_ref(x, sr), R.direct_ref(x, sr)
    assert got.shape == want.shape == (R.n_out(300, *R.ratio(sr, 44100)),)
    err = np.abs(got - want).max()
    print(sr, "polyphase vs zero-stuff / convolve / decimate:", err)
    assert err < 1e-12 and np.abs(want).max() > 1.0


def test_output_lengths():
    L, M = R.ratio(48000, 44100)
    assert [R.n_out(n, L, M) for n in (1, 159, 160, 161, 4410)] == [1, 147, 147, 148, 4052]
    L, M = R.ratio(16000, 44100)
    assert [R.n_out(n, L, M) for n in (1, 159, 160, 161, 4410)] == [3, 439, 441, 444, 12156]
    from mm_distillnet_amd.audio import resample_len
    for sr in RATES:
        for n in (1, 159, 160, 161, 4410):
            assert resample_len(n, sr) == R.n_out(n, *R.ratio(sr, 44100)) == -((-n * 44100) // sr)
    assert R.resample_ref(np.ones(161, np.float32), 48000).shape == (148,)
    assert R.resample_ref(np.ones((2, 3, 1), np.float32), 16000).shape == (2, 3, 3)


@pytest.mark.parametrize("sr", RATES)
def test_tone_against_its_analytic_resample(sr):
    """A tone at 0.2 * min(sr_in, sr_out), well inside the pass band, over the outputs whose `half` input samples on either side all
    exist (the filter's reach, half * L / M outputs, away from both ends).
    Bound: the design's own pass-band error, 7e-8 of the amplitude (the figure of the float64 prototype the rule was checked with, issue
    and DESIGN.md section 7g), plus what rounding the bank to float32 can add, 2^-25 * sum_k |bank[p][k]| at the worst phase."""
    L, M = R.ratio(sr, 44100)
    half, f = R.half_len(L, M), 0.2 * min(sr, 44100)
    n_in = 6 * half + 400
    x = np.sin(2 * np.pi * f * np.arange(n_in) / sr)
    y = R.resample_ref(x, sr)
    reach = -((-half * L) // M) + 1
    lo, hi = reach, len(y) - reach
    assert hi - lo > 100
    want = np.sin(2 * np.pi * f * np.arange(len(y)) / 44100.0)
    err = np.abs(y - want)[lo:hi].max()
    bound = 7e-8 + 2.0 ** -25 * np.abs(R.bank(L, M)).astype(np.float64).sum(1).max()
    print(sr, "tone error", err, "bound", bound)
    assert err < bound
    # the sequential float32 mode is the same rule, only rounded
    y32 = R.resample_ref(x.astype(np.float32), sr, dtype=np.float32)
    assert y32.dtype == np.float32 and np.abs(y32 - R.resample_ref(x.astype(np.float32), sr))[lo:hi].max() < 5e-6


def test_zero_extension_at_the_ends():
    """an impulse at sample 0 comes out as the filter itself: y[t] = h(t M / L), nothing reflected"""
    L, M = R.ratio(48000, 44100)
    x = np.zeros(400, np.float32)
    x[0] = 1.0
    y = R.resample_ref(x, 48000)
    t = np.arange(len(y))
    want = R.h(t * M, L, M).astype(np.float32).astype(np.float64)              # tau = t M / L
    assert np.array_equal(y, want)
    assert np.all(y[R.n_out(70, L, M) + 1:] == 0.0) and y[0] == np.float32((147 / 160) * R.ROLLOFF)


# ---------------------------------------------------------------------------------------------- the host bank
@pytest.mark.parametrize("sr", RATES)
def test_resample_bank_equals_the_restatement_bit_for_bit(sr):
    from mm_distillnet_amd.audio import resample_bank
    L, M, half, bank, off = resample_bank(sr, 44100)
    assert (L, M) == R.ratio(sr, 44100) and half == R.half_len(L, M)
    want = R.bank(L, M)
    assert bank.dtype == np.float32 and bank.shape == want.shape and np.array_equal(bank.view(np.int32), want.view(np.int32))
    assert off.dtype == np.int32 and off.tolist() == [(p * M) // L for p in range(L)]


def test_resample_bank_refuses_large_factors():
    from mm_distillnet_amd.audio import resample_bank
    with pytest.raises(ValueError, match="44100 / 44101"):
        resample_bank(44101, 44100)
    with pytest.raises(ValueError, match="1025 / 1"):
        resample_bank(1, 1025)
    with pytest.raises(ValueError, match="1 / 1024: its filter has 131072 taps"):             # L, M fit; the kernel's 4096 taps do not
        resample_bank(1024, 1)
    with pytest.raises(ValueError, match="1 / 33: its filter has 4224 taps"):
        resample_bank(33, 1)
    assert resample_bank(32, 1)[:3] == (1, 32, 2048) and resample_bank(32, 1)[3].shape == (1, 4096)
    with pytest.raises(ValueError):
        resample_bank(0, 44100)


# ---------------------------------------------------------------------------------------------- C ABI without a GPU
def test_header_declares_the_entry_points():
    import __graft_entry__ as ge
    ge.build()
    from mm_distillnet_amd import _lib
    sigs = _lib.LIB.symbols()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    text = open(_lib.HEADER).read()

    def comment_of(name):
        head = text[:text.index("int %s(" % name)]
        return " ".join(ln[2:].strip() for ln in head[head.rindex("\n\n"):].split("\n") if ln.startswith("//"))

    for name, nargs in (("mmd_resample_poly", 11), ("mmd_pcm_to_float", 6)):
        assert name in sigs and hasattr(dll, name) and len(sigs[name]) == nargs, name
        comment = comment_of(name)
        assert "mp3_to_pkl.py:31" in comment and "need no zeroing" in comment.replace("needs", "need") and "-22" in comment, name
        assert "Caps:" in comment and "same bits" in comment, name
    comment = comment_of("mmd_resample_poly")
    assert "UNPINNED" in comment and "ZERO-EXTENDED" in comment and "bank[j * L + r]" in comment and "tests/resample_ref.py" in comment


def test_bad_arguments_are_rejected_without_gpu():
    import __graft_entry__ as ge
    ge.build()
    from mm_distillnet_amd import _lib
    dll = _lib.LIB.load()
    p = ctypes.c_void_p(4096)            # never dereferenced: validation precedes any launch
    rs = dll.mmd_resample_poly
    good = dict(x=p, rows=16, n_in=4097, bank=p, off=p, L=147, M=160, taps=140, y=p, n_out=3765)

    def call(**kw):
        a = dict(good, **kw)
        return rs(a["x"], a["rows"], a["n_in"], a["bank"], a["off"], a["L"], a["M"], a["taps"], a["y"], a["n_out"], None)

    assert -((-4097 * 147) // 160) == 3765
    for name in ("x", "bank", "off", "y"):
        assert call(**{name: None}) == -22, name
    for kw in (dict(rows=0), dict(rows=-1), dict(n_in=0, n_out=0), dict(n_in=-5, n_out=-4), dict(L=0), dict(L=1025), dict(M=0), dict(M=1025),
               dict(L=-147), dict(M=-160), dict(taps=139), dict(taps=141), dict(taps=0), dict(taps=1), dict(taps=4098), dict(taps=-2),
               dict(n_out=3764), dict(n_out=3766), dict(n_out=4097), dict(n_in=(1 << 50) + 1, n_out=0), dict(rows=65536)):
        assert call(**kw) == -22, kw
    pf = dll.mmd_pcm_to_float
    assert pf(None, 100, 8, 2, p, None) == -22
    assert pf(p, 100, 8, 2, None, None) == -22
    for bad in ((0, 8, 2), (-1, 8, 2), (100, 0, 2), (100, -8, 2), (100, 8, 1), (100, 8, 0), (100, 8, 5), (100, 8, 8), (100, 8193, 2),
                (100, 4097, 4)):
        assert pf(p, *bad, p, None) == -22, bad


# ---------------------------------------------------------------------------------------------- detect.py's raw reader
def _write_wav(path, samples, rate, width, channels=8):
    """samples: int64 [frames, channels] in the width's range (width 1: unsigned 8-bit, as WAV stores it)"""
    if width == 1:
        raw = samples.astype(np.uint8).tobytes()
    else:
        le = samples.astype("<i8").view(np.uint8).reshape(samples.shape[0], samples.shape[1], 8)[:, :, :width]
        raw = np.ascontiguousarray(le).tobytes()
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels); w.setsampwidth(width); w.setframerate(rate)
        w.writeframes(raw)
    return raw


@pytest.mark.parametrize("rate", [22050, 48000])
@pytest.mark.parametrize("width", [2, 3, 4])
def test_read_recording_hands_over_the_raw_frames(tmp_path, rate, width):
    from mm_distillnet_amd import recording as det
    top = 1 << (8 * width - 1)
    s = np.random.default_rng(width).integers(-top, top, (333, 8))
    s[0, 0], s[1, 0], s[2, 0] = -top, top - 1, -1
    raw = _write_wav(tmp_path / "r.wav", s, rate, width)
    got, frames, channels, w, r = det.read_recording(str(tmp_path / "r.wav"))
    assert (frames, channels, w, r) == (333, 8, width, rate)
    assert got.dtype == np.uint8 and got.shape == (333 * 8 * width,) and got.flags["C_CONTIGUOUS"] and got.flags["WRITEABLE"]
    assert got.tobytes() == raw
    # the bytes are little-endian signed samples, frame by frame
    back = np.zeros((333, 8), np.int64)
    by = got.reshape(333, 8, width).astype(np.int64)
    for k in range(width):
        back |= by[:, :, k] << (8 * k)
    back = np.where(back >= top, back - 2 * top, back)
    assert np.array_equal(back, s)


def test_read_recording_refuses_other_formats_and_read_input_is_untouched(tmp_path):
    from mm_distillnet_amd import recording as det
    s = np.random.default_rng(0).integers(-32768, 32768, (900, 8))
    _write_wav(tmp_path / "narrow.wav", (s >> 8) + 128, 48000, 1)
    with pytest.raises(ValueError, match="16-, 24- or 32-bit PCM"):
        det.read_recording(str(tmp_path / "narrow.wav"))
    _write_wav(tmp_path / "stereo.wav", s[:, :2], 48000, 2, channels=2)
    with pytest.raises(ValueError, match="8 microphone channels, found 2"):
        det.read_recording(str(tmp_path / "stereo.wav"))
    _write_wav(tmp_path / "slow.wav", s, 22050, 2)
    assert det.read_recording(str(tmp_path / "slow.wav"))[1:] == (900, 8, 2, 22050)
    with pytest.raises(ValueError, match="22050 Hz is not supported"):               # the default path still refuses it
        det.read_input(str(tmp_path / "slow.wav"))
    _write_wav(tmp_path / "wide.wav", s << 8, 44100, 3)
    with pytest.raises(ValueError, match="only 16-bit PCM"):
        det.read_input(str(tmp_path / "wide.wav"))


def test_resample_flags_are_checked_before_any_device_work(tmp_path):
    """--resample is for a .wav, --sample_rate for a .npy: the mix-ups are refused by name (no GPU: the check precedes every tensor)"""
    det = _detect()
    import argparse
    np.save(tmp_path / "a.npy", np.zeros((8, 700), np.float32))
    _write_wav(tmp_path / "a.wav", np.zeros((700, 8), np.int64), 48000, 2)
    ns = argparse.Namespace
    with pytest.raises(ValueError, match="--resample reads a .wav"):
        det.load_resampled(ns(input=str(tmp_path / "a.npy"), resample=True, sample_rate=None), "cpu")
    with pytest.raises(ValueError, match="--resample reads a .wav"):
        det.load_resampled(ns(input=str(tmp_path / "a.wav"), resample=True, sample_rate=48000), "cpu")
    with pytest.raises(ValueError, match="--sample_rate R says"):
        det.load_resampled(ns(input=str(tmp_path / "a.wav"), resample=False, sample_rate=48000), "cpu")
    with pytest.raises(ValueError, match="positive number of Hz"):
        det.load_resampled(ns(input=str(tmp_path / "a.npy"), resample=False, sample_rate=0), "cpu")
