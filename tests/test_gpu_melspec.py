"""Waveform front end on the GPU: csrc/melspec.hip against the float64 restatement (tests/melspec_ref.py), with the error of the
same chain in host float32 - what librosa 0.7.2 itself computes - as the yardstick; reproducibility; the Python host (MelFrontEnd,
DeviceInputPipeline with waveform samples, train.py's audio_mix = waveform).

Figures of the MI355X run: profiles/melspec_notes.md."""
import os
import sys

import numpy as np
import pytest
import torch

import melspec_ref as R
from oracle import input_ref as I

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dataset(n, length=6):
    from mm_distillnet_amd.data import SyntheticMultimodalDetection
    return SyntheticMultimodalDetection({"image_size": 64, "seed": 24, "synthetic_length": length, "synthetic_wave_samples": n})


def _ref_stack(wa, wb, dtype=np.float64):
    """[C, N] float32 numpy waveform(s) -> [80, T, C] in `dtype` arithmetic."""
    return np.stack([R.melspec_ref(wa[c], None if wb is None else wb[c], dtype=dtype) for c in range(wa.shape[0])], axis=2)


def _errors(got, ref):
    """(max |d| / max(ref), max relative error over the elements above 1e-6 max(ref), share of the elements below that floor)"""
    got, ref = got.astype(np.float64), ref.astype(np.float64)
    top = ref.max()
    big = ref > 1e-6 * top
    d = np.abs(got - ref)
    return d.max() / top, (d[big] / ref[big]).max(), 1.0 - big.mean()


def _resize_atol(ref):
    """Absolute tolerance of the resized map against oracle.input_ref's cubic resize of the float64 restatement: the one
    test_device_cubic_resize_matches_oracle uses (rtol 1e-5, atol 2e-4 on maps of magnitude ~100, -40 +- 4 x 15 dB, i.e. 2e-6 of the
    map's maximum), scaled by this map's maximum."""
    return 2e-6 * float(np.abs(ref).max())


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("n", [1024, 22050, 33000, 44100])
def test_kernel_matches_float64_restatement_within_4x_host_float32(n, mixed):
    """Yardstick: the same arithmetic in host float32 (scipy.fft keeps single precision; float32 bank).  The kernel's two error figures
    against float64 may each be at most 4 x the host-float32 figure on the same input: another FFT factorisation, fused
    multiply-adds and another summation order move the error by small factors; a fast-math twiddle (1e-4), a symmetric window or a
    wrong pad rule miss by orders of magnitude."""
    from mm_distillnet_amd.audio import MelFrontEnd
    ds = _dataset(n)
    wa, wb = ds.waveforms(1), (ds.waveforms(4) if mixed else None)
    fe = MelFrontEnd(DEV)
    got = fe.melspec(wa[None].to(DEV), None if wb is None else wb[None].to(DEV))[0].cpu().numpy()
    ref = _ref_stack(wa.numpy(), None if wb is None else wb.numpy())
    host32 = _ref_stack(wa.numpy(), None if wb is None else wb.numpy(), dtype=np.float32)
    assert got.shape == ref.shape == (80, 1 + n // 256, 8) and host32.dtype == np.float32
    g_abs, g_rel, g_low = _errors(got, ref)
    h_abs, h_rel, _ = _errors(host32, ref)
    print("melspec n=%d mixed=%d: kernel max|d|/max %.3e rel %.3e | host float32 %.3e rel %.3e | below floor %.4f"
          % (n, mixed, g_abs, g_rel, h_abs, h_rel, g_low))
    assert g_low <= 0.01                   # the noise floor keeps the relative metric from leaving anything out
    assert np.isfinite(got).all()
    assert g_abs <= 4.0 * h_abs, (g_abs, h_abs)
    assert g_rel <= 4.0 * h_rel, (g_rel, h_rel)


def test_two_launches_into_dirty_buffers_give_the_same_bits():
    from mm_distillnet_amd import _lib
    from mm_distillnet_amd.audio import MelFrontEnd
    fe = MelFrontEnd(DEV)
    ds = _dataset(33000)
    wa, wb = ds.waveforms(0).to(DEV), ds.waveforms(2).to(DEV)
    T = fe.n_frames(33000)
    o1 = torch.full((80, T, 8), float("nan"), device=DEV)
    o2 = torch.full((80, T, 8), -7.5e8, device=DEV)
    for o in (o1, o2):
        _lib.call("mmd_melspec_power", wa, wb, 8, 33000, fe.start, fe.length, fe.band, fe.stride, o)
    torch.cuda.synchronize()
    assert torch.isfinite(o1).all() and torch.equal(o1, o2)
    assert torch.equal(o1, fe.melspec(wa[None], wb[None])[0])


def test_student_input_batch_equals_per_sample_and_the_oracle_resize():
    from mm_distillnet_amd.audio import MelFrontEnd
    fe = MelFrontEnd(DEV)
    n, S = 22050, 96
    ds = _dataset(n)
    wa = torch.stack([ds.waveforms(i) for i in range(3)]); wb = torch.stack([ds.waveforms(5 - i) for i in range(3)])
    got = fe.student_input(wa.to(DEV), wb.to(DEV), S)
    assert got.shape == (3, 8, S, S)
    for b in range(3):
        one = fe.student_input(wa[b:b + 1].to(DEV), wb[b:b + 1].to(DEV), S)[0]
        assert torch.equal(one, got[b])
        ref = _ref_stack(wa[b].numpy(), wb[b].numpy())
        want = I.prepare_audio(ref, S)
        np.testing.assert_allclose(got[b].cpu().numpy(), want, rtol=1e-5, atol=_resize_atol(ref))
    single = fe.student_input(wa.to(DEV), None, S)            # Audio2Spectogram: one recording
    ref1 = _ref_stack(wa[1].numpy(), None)
    np.testing.assert_allclose(single[1].cpu().numpy(), I.prepare_audio(ref1, S), rtol=1e-5, atol=_resize_atol(ref1))


def test_device_pipeline_takes_waveform_samples():
    from mm_distillnet_amd.audio import MelFrontEnd
    from mm_distillnet_amd.data import RawSyntheticMultimodalDetection, DeviceInputPipeline, collate_raw
    cfg = {"seed": 24, "image_size": 96, "synthetic_wave_samples": 8000}
    wave = RawSyntheticMultimodalDetection(dict(cfg, audio_format="waveform"), length=3, frame_hw=(54, 72))
    spec = RawSyntheticMultimodalDetection(cfg, length=3, frame_hw=(54, 72), mel_hw=(32, 32))
    ws, ss = [wave[i] for i in range(3)], [spec[i] for i in range(3)]
    pipe = DeviceInputPipeline(96, DEV)
    plain = {k: v.clone() for k, v in pipe.submit(ss).wait().items()}
    got = {k: v.clone() for k, v in pipe.submit(ws).wait().items()}
    stacked = {k: v.clone() for k, v in pipe.submit(collate_raw(ws)).wait().items()}
    torch.cuda.synchronize()
    fe = MelFrontEnd(DEV)
    want = fe.student_input(torch.stack([s["audio_wave"] for s in ws]).to(DEV), None, 96)
    assert got["audio"].shape == (3, 8, 96, 96) and torch.equal(got["audio"], want) and torch.equal(stacked["audio"], want)
    for k in ("rgb", "thermal", "depth"):
        assert torch.equal(got[k], plain[k]) and torch.equal(stacked[k], plain[k]), k


def test_device_pipeline_takes_a_list_that_mixes_the_two_audio_formats():
    """A spectrogram sample first, waveform samples behind it: the front end is made when any sample of the list needs it."""
    from mm_distillnet_amd.audio import MelFrontEnd
    from mm_distillnet_amd.data import RawSyntheticMultimodalDetection, DeviceInputPipeline
    cfg = {"seed": 24, "image_size": 64, "synthetic_wave_samples": 4000}
    wave = RawSyntheticMultimodalDetection(dict(cfg, audio_format="waveform"), length=3, frame_hw=(54, 72))
    spec = RawSyntheticMultimodalDetection(cfg, length=3, frame_hw=(54, 72), mel_hw=(32, 32))
    pipe = DeviceInputPipeline(64, DEV)
    only_spec = pipe.submit([spec[0]]).wait()["audio"].clone()
    got = pipe.submit([spec[0], wave[1], wave[2]]).wait()["audio"].clone()
    torch.cuda.synchronize()
    want = MelFrontEnd(DEV).student_input(torch.stack([wave[1]["audio_wave"], wave[2]["audio_wave"]]).to(DEV), None, 64)
    assert torch.equal(got[0], only_spec[0]) and torch.equal(got[1:], want)


def test_train_kdlist_augmented_with_waveform_mix(tmp_path, monkeypatch):
    """audio_mix = waveform: the augmented steps hand the engine MelFrontEnd.student_input of the two recordings' waveforms; without
    the key the batch audio is the spectrogram-domain mix of `_yield_batch`, bit for bit."""
    monkeypatch.chdir(tmp_path)
    sys.path.insert(0, ROOT)
    import train
    from mm_distillnet_amd import data as D
    from mm_distillnet_amd.audio import MelFrontEnd
    from mm_distillnet_amd.step import DistillEngine
    cfgf = os.path.join(ROOT, "configs", "mm-distillnet.cfg")
    ov = ('{"image_size": 128, "batch_size": 2, "synthetic_length": 8, "num_epoches": 1, "resume": "False", "num_workers": 0, '
          '"no_validation": "True", "train_method": "traditional_nms_kdlist_augmented", "synthetic_wave_samples": 22050, "exp_name": "%s"%s}')
    fired = [False, True, True, False]
    seen, waves, mixes = [], [], []
    replay = DistillEngine.replay

    def spy_replay(self, batch):
        seen.append(batch["audio"].clone())
        return replay(self, batch)

    ybw, yb = D.SyntheticMultimodalDetection.yield_batch_waves, D.SyntheticMultimodalDetection.yield_batch

    def spy_waves(self, batch_size, ids):
        out = ybw(self, batch_size, ids)
        waves.append((list(ids), out[1].clone(), out[2].clone()))
        return out

    def spy_mix(self, batch_size, ids):
        state = np.random.get_state()
        out = yb(self, batch_size, ids)
        after = np.random.get_state()
        np.random.set_state(state)
        again = D._yield_batch(self, batch_size, ids)          # the parent's function under the same RNG state
        np.random.set_state(after)
        assert torch.equal(out[1], again[1]) and torch.equal(out[0], again[0])
        mixes.append(out[1].clone())
        return out

    monkeypatch.setattr(DistillEngine, "replay", spy_replay)
    monkeypatch.setattr(D.SyntheticMultimodalDetection, "yield_batch_waves", spy_waves)
    monkeypatch.setattr(D.SyntheticMultimodalDetection, "yield_batch", spy_mix)

    draws = iter(fired)
    monkeypatch.setattr(train.TR, "kdlist_augment_now", lambda epoch: next(draws))
    loss = train.main(["--config_file", cfgf, "--overwrite", ov % ("exp_wave", ', "audio_mix": "waveform"'), "--max_steps", "4"])
    torch.cuda.synchronize()
    assert np.isfinite(loss) and train.LAST_RUN_STEPS == 4
    assert len(waves) == 2 and not mixes
    steps = seen[:4]
    fe = MelFrontEnd(DEV)
    for (ids, wa, wb), audio in zip(waves, [steps[1], steps[2]]):
        assert wa.shape == (2, 8, 22050)
        want = fe.student_input(wa.to(DEV), wb.to(DEV), 128)
        assert torch.isfinite(audio).all() and torch.equal(audio, want)
        ref = _ref_stack(wa[0].numpy(), wb[0].numpy())
        np.testing.assert_allclose(audio[0].cpu().numpy(), I.prepare_audio(ref, 128), rtol=1e-5, atol=_resize_atol(ref))

    # the same run without the key: the parent's spectrogram-domain mix reaches the engine unchanged
    seen.clear(); waves.clear()
    draws = iter(fired)
    loss = train.main(["--config_file", cfgf, "--overwrite", ov % ("exp_spec", ""), "--max_steps", "4"])
    torch.cuda.synchronize()
    assert np.isfinite(loss) and len(mixes) == 2 and not waves
    steps = seen[:4]
    for mix, audio in zip(mixes, [steps[1], steps[2]]):
        assert torch.equal(audio.cpu(), mix)
    with pytest.raises(Exception, match="Unsupported audio_mix"):
        train.main(["--config_file", cfgf, "--overwrite", ov % ("exp_bad", ', "audio_mix": "both"'), "--max_steps", "1"])
    # the refusal of the augmented KD-list method on the raw pipeline stays
    with pytest.raises(Exception, match="not available with input_pipeline = raw"):
        train.main(["--config_file", cfgf, "--overwrite", ov % ("exp_raw", ', "audio_mix": "waveform", "input_pipeline": "raw"'), "--max_steps", "1"])
