"""Waveform front end, CPU side: the float64 restatement (tests/melspec_ref.py) against closed forms, the package's filter bank and
tables against the restatement, the C ABI's argument checks, and the partner draws of `yield_batch_waves`."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import melspec_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- the restatement against closed forms
@pytest.mark.parametrize("k,amp", [(3, 1.0), (100, 0.25), (509, 2.0)])
def test_on_bin_sinusoid_has_closed_form_power(k, amp):
    n = 8192
    y = amp * np.cos(2.0 * np.pi * k * np.arange(n) / R.N_FFT + 0.3)
    p = R.power_spectrum(y)                                  # [513, T]
    t = p.shape[1] // 2                                      # interior frame: no reflected samples
    peak = (amp * 512.0 / 2.0) ** 2                          # window sum 512, half of the amplitude on the positive bin
    assert abs(p[k, t] - peak) <= 1e-9 * peak
    np.testing.assert_allclose(p[[k - 1, k + 1], t], peak / 4.0, rtol=1e-9)      # Hann: -1/2 of the peak amplitude on both neighbours
    rest = np.delete(p[:, t], [k - 1, k, k + 1])
    assert rest.max() <= 1e-20 * peak


@pytest.mark.parametrize("n", [513, 1023, 1024, 1025, 22050, 33000, 44100])
def test_frame_count(n):
    assert R.frames(np.zeros(n)).shape == (1 + n // 256, 1024)
    assert R.melspec_ref(np.zeros(n, np.float32)).shape == (80, 1 + n // 256)


def test_first_frame_of_a_ramp_shows_the_reflect_rule():
    y = np.arange(2048, dtype=np.float64)
    f0 = R.frames(y)[0]
    # padded[j] = y[512 - j] for j < 512: sample 0 sits once, at j = 512, and its neighbours are 1 on both sides
    np.testing.assert_array_equal(f0[:512], np.arange(512, 0, -1))
    np.testing.assert_array_equal(f0[512:], np.arange(0, 512))
    last = R.frames(y)[-1]                                   # frame 8 = padded[2048:3072] = y[1536:2048], then y[2046], y[2045], ...
    np.testing.assert_array_equal(last[:512], np.arange(1536, 2048))
    np.testing.assert_array_equal(last[512:], np.arange(2046, 2046 - 512, -1))


def test_mix_is_a_float32_mean():
    a = np.array([1.0, 3.0000001, 1e-3], np.float32); b = np.array([2.0, 1.0, 7e-4], np.float32)
    m = R.mix(a, b)
    assert m.dtype == np.float32 and np.array_equal(m, (a + b) / np.float32(2))
    assert R.mix(a) is not None and np.array_equal(R.mix(a), a)


def test_mel_centre_frequencies_follow_the_slaney_scale():
    f = R.mel_frequencies()
    assert f.shape == (82,) and f[0] == 0.0 and abs(f[-1] - 22050.0) < 1e-9
    step = R.hz_to_mel(22050.0) / 81.0                       # mels per band edge
    lin = f[f < 1000.0]
    np.testing.assert_allclose(np.diff(lin), step * 200.0 / 3.0, rtol=1e-12)                  # 200/3 Hz per mel
    log = f[f >= 1000.0]
    np.testing.assert_allclose(np.diff(np.log(log)), step * np.log(6.4) / 27.0, rtol=1e-12)   # log(6.4)/27 per mel
    assert abs(R.mel_to_hz(15.0) - 1000.0) < 1e-12 and abs(R.hz_to_mel(6400.0) - 42.0) < 1e-12


def test_filter_bank_rows_are_area_normalised_triangles():
    f = R.mel_frequencies()
    bins = np.arange(513) * (44100.0 / 1024.0)
    w = R.mel_bank64()
    for i in range(80):
        lo, pk, hi = f[i], f[i + 1], f[i + 2]
        tri = np.where(bins <= pk, (bins - lo) / (pk - lo), (hi - bins) / (hi - pk))
        want = np.maximum(tri, 0.0) * 2.0 / (hi - lo)
        np.testing.assert_allclose(w[i], want, rtol=1e-12, atol=1e-18)
        assert w[i].max() <= 2.0 / (hi - lo) * (1 + 1e-12)


# ---------------------------------------------------------------------------------------------- the package against the restatement
def test_package_filter_bank_is_the_restatement_in_float32():
    from mm_distillnet_amd import audio
    w = audio.mel_filters()
    assert w.dtype == np.float32 and w.shape == (80, 513)
    assert np.array_equal(w, R.mel_bank32())


def test_band_form_rebuilds_the_dense_bank_and_rows_are_contiguous():
    from mm_distillnet_amd import audio
    start, length, band = audio.mel_bands()
    w = audio.mel_filters()
    assert start.dtype == np.int32 and length.dtype == np.int32 and band.dtype == np.float32
    assert band.shape == (80, length.max()) and 80 * band.shape[1] <= 4096          # what the kernel keeps in LDS
    assert int(length.sum()) == np.count_nonzero(w) == 997 and length.max() == 50 and length.min() >= 1
    dense = np.zeros_like(w)
    for m in range(80):
        nz = np.flatnonzero(w[m])
        assert nz[-1] - nz[0] + 1 == nz.size                 # one contiguous run
        assert np.all(band[m, length[m]:] == 0)
        dense[m, start[m]:start[m] + length[m]] = band[m, :length[m]]
    assert np.array_equal(dense, w)
    assert (start + length).max() <= 513


def test_kernel_tables_are_double_values_rounded_once():
    text = open(os.path.join(ROOT, "mm_distillnet_amd", "csrc", "melspec_tables.h")).read()

    def table(name):
        body = text[text.index(name):]
        body = body[body.index("{") + 1:body.index("}")]
        return np.array([float.fromhex(v.strip().rstrip("f")) for v in body.split(",") if v.strip()])

    tw, win = table("mmd_mel_twiddle["), table("mmd_mel_hann[")
    a = 2.0 * np.pi * np.arange(1024) / 1024.0
    assert tw.shape == (2048,) and win.shape == (1024,)
    assert np.array_equal(tw[0::2], np.cos(a).astype(np.float32).astype(np.float64))
    assert np.array_equal(tw[1::2], (-np.sin(a)).astype(np.float32).astype(np.float64))
    assert np.array_equal(win, R.hann().astype(np.float32).astype(np.float64))
    src = open(os.path.join(ROOT, "mm_distillnet_amd", "csrc", "melspec.hip")).read()
    assert not re.search(r"__sinf|__cosf|sincosf|\bsinf\b|\bcosf\b", src)       # no device trigonometry on this path


# ---------------------------------------------------------------------------------------------- C ABI without a GPU
def test_frame_count_and_bad_arguments_without_gpu():
    import __graft_entry__ as ge
    ge.build()
    from mm_distillnet_amd import _lib
    dll = _lib.LIB.load()
    for n in (513, 1024, 22050, 33000, 44100, 1 << 33):
        assert dll.mmd_melspec_frames(n) == 1 + n // 256
    for n in (512, 1, 0, -5):
        assert dll.mmd_melspec_frames(n) == -22
    p = ctypes.c_void_p(4096)            # never dereferenced: validation precedes any launch
    assert dll.mmd_melspec_power(None, None, 8, 44100, p, p, p, 50, p, None) == -22
    assert dll.mmd_melspec_power(p, None, 8, 44100, None, p, p, 50, p, None) == -22
    assert dll.mmd_melspec_power(p, None, 8, 44100, p, None, p, 50, p, None) == -22
    assert dll.mmd_melspec_power(p, None, 8, 44100, p, p, None, 50, p, None) == -22
    assert dll.mmd_melspec_power(p, None, 8, 44100, p, p, p, 50, None, None) == -22
    assert dll.mmd_melspec_power(p, p, 8, 512, p, p, p, 50, p, None) == -22
    assert dll.mmd_melspec_power(p, p, 8, 0, p, p, p, 50, p, None) == -22
    assert dll.mmd_melspec_power(p, p, 0, 44100, p, p, p, 50, p, None) == -22
    assert dll.mmd_melspec_power(p, p, 8, 44100, p, p, p, 0, p, None) == -22
    assert dll.mmd_melspec_power(p, p, 8, 44100, p, p, p, 52, p, None) == -22       # 80 * 52 floats do not fit the kernel's LDS table
    text = open(_lib.HEADER).read()
    for name in ("mmd_melspec_frames", "mmd_melspec_power"):
        head = text[:text.index("int %s(" % name)]
        comment = head[head.rindex("\n\n"):]
        assert "MultimodalDetection.py:329-353" in comment and "transformations.py:251-266" in comment, name
    assert "out[80, T, channels]" in text


# ---------------------------------------------------------------------------------------------- synthetic waveforms and partner draws
def test_synthetic_waveforms_are_deterministic_float32():
    from mm_distillnet_amd.data import SyntheticMultimodalDetection, RawSyntheticMultimodalDetection
    ds = SyntheticMultimodalDetection({"image_size": 32, "seed": 5, "synthetic_length": 6})
    w = ds.waveforms(2)
    assert w.shape == (8, 44100) and w.dtype == torch.float32 and torch.equal(w, ds.waveforms(2))
    assert not torch.equal(w, ds.waveforms(3)) and not torch.equal(w[0], w[1])
    assert 0.05 < float(w.std()) < 1.0 and float(w.abs().max()) < 2.0
    ds2 = SyntheticMultimodalDetection({"image_size": 32, "seed": 5, "synthetic_length": 6, "synthetic_wave_samples": 3000})
    assert ds2.waveforms(0).shape == (8, 3000)
    raw = RawSyntheticMultimodalDetection({"seed": 5, "audio_format": "waveform", "synthetic_wave_samples": 2048}, length=3,
                                          frame_hw=(20, 24))
    s = raw[1]
    assert "audio" not in s and s["audio_wave"].shape == (8, 2048) and s["audio_wave"].dtype == torch.float32
    plain = RawSyntheticMultimodalDetection({"seed": 5}, length=3, frame_hw=(20, 24), mel_hw=(8, 8))[1]
    assert "audio_wave" not in plain and torch.equal(plain["rgb"], s["rgb"]) and torch.equal(plain["thermal"], s["thermal"])
    with pytest.raises(Exception, match="Unsupported audio_format"):
        RawSyntheticMultimodalDetection({"audio_format": "mp3"})


def test_collate_raw_stacks_waveform_samples():
    from mm_distillnet_amd.data import RawSyntheticMultimodalDetection, collate_raw
    raw = RawSyntheticMultimodalDetection({"seed": 5, "audio_format": "waveform", "synthetic_wave_samples": 1500}, length=3,
                                          frame_hw=(20, 24))
    st = collate_raw([raw[i] for i in range(3)])
    assert isinstance(st, dict) and st["audio_wave"].shape == (3, 8, 1500) and "audio" not in st and st["id"] == [0, 1, 2]


def test_yield_batch_waves_draws_the_partners_of_yield_batch():
    from mm_distillnet_amd.data import SyntheticMultimodalDetection
    ds = SyntheticMultimodalDetection({"image_size": 16, "seed": 11, "synthetic_length": 9, "synthetic_wave_samples": 2000})
    ids = [4, 0, 7]
    np.random.seed(123)
    rgb_s, _ = ds.yield_batch(3, ids)
    after_s = np.random.get_state()[1].copy()
    np.random.seed(123)
    rgb_w, wav_a, wav_b = ds.yield_batch_waves(3, ids)
    after_w = np.random.get_state()[1].copy()
    assert torch.equal(rgb_s, rgb_w) and np.array_equal(after_s, after_w)            # same partners, same RNG consumption
    np.random.seed(123)
    picks = np.random.choice([i for i in range(9) if i not in ids], size=3)
    assert wav_a.shape == wav_b.shape == (3, 8, 2000)
    for k in range(3):
        assert torch.equal(wav_a[k], ds.waveforms(ids[k])) and torch.equal(wav_b[k], ds.waveforms(int(picks[k])))
        assert torch.equal(rgb_w[k], ds[int(picks[k])][0])
