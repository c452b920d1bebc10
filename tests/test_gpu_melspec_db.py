"""dB mel front end on the GPU: mmd_melspec_batch / mmd_power_to_db / mmd_resize_cubic_batch (csrc/melspec.hip, csrc/input.hip) against
the float64 restatement (tests/melspec_ref.py + tests/melspec_db_ref.py), with the error of the same chain in host float32 as the
yardstick; batched against per-sample bits; dirty buffers; the Python host (MelFrontEnd, DeviceInputPipeline with audio_db).

Figures of the MI355X run: profiles/melspec_db_notes.md."""
import functools

import numpy as np
import pytest
import torch

import melspec_db_ref as D

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, C = 3, 8
# 3 ulp of float32 at magnitude 100 = |10 log10 1e-10|: the device log10f's documented 2-ulp bound over numpy's, on the two terms
LOG_SLACK = 2.3e-5


@functools.lru_cache(maxsize=None)
def _waves(n):
    """(wav_a, wav_b) float32 [3, 8, n]: sample 1 quiet (x 1e-3), channel 5 of sample 2 silent, channel 2 of sample 0 loud (x 30) - a
    maximum taken over the batch or over the sample instead of per (sample, channel) misses by tens of dB."""
    from mm_distillnet_amd.data import SyntheticMultimodalDetection
    ds = SyntheticMultimodalDetection({"image_size": 64, "seed": 24, "synthetic_length": 6, "synthetic_wave_samples": n})
    wa = torch.stack([ds.waveforms(i) for i in range(B)]); wb = torch.stack([ds.waveforms(5 - i) for i in range(B)])
    wa[1] *= 1e-3
    wa[2, 5] = 0.0
    wa[0, 2] *= 30.0
    return wa, wb


@functools.lru_cache(maxsize=None)
def _refs(n):
    """(float64 dB stack, host-float32 dB stack) [3, 80, T, 8] of the unmixed waveforms; computed once per size and left unchanged"""
    wa = _waves(n)[0].numpy()
    r64 = np.stack([D.stack_db_ref(wa[b]) for b in range(B)])
    r32 = np.stack([D.stack_db_ref(wa[b], dtype=np.float32) for b in range(B)])
    r64.setflags(write=False); r32.setflags(write=False)
    return r64, r32


def _front():
    from mm_distillnet_amd.audio import MelFrontEnd
    return MelFrontEnd(DEV)


def _batch(fe, wa, wb, db, out=None, ws=None):
    from mm_distillnet_amd import _lib
    b, c, n = wa.shape
    out = torch.empty(b, 80, fe.n_frames(n), c, device=DEV) if out is None else out
    ws = torch.empty(b * c, device=DEV) if ws is None and db else ws
    _lib.call("mmd_melspec_batch", wa, wb, b, c, n, fe.start, fe.length, fe.band, fe.stride, db, ws, out)
    return out


@pytest.mark.parametrize("n", [1024, 2100, 33000])
def test_db_map_matches_float64_restatement_within_4x_host_float32(n):
    """n = 1024: T = 5, one partial block; 2100: T = 9, a second block with one frame (the maximum combines across blocks); 33000: T = 129.
    max|d| in dB against the float64 chain may be at most 4 x the host-float32 chain's on the same input (the rule and reasons of
    test_gpu_melspec.py::test_kernel_matches_float64_restatement_within_4x_host_float32) plus LOG_SLACK.  No element is left out."""
    fe = _front()
    wa, _ = _waves(n)
    r64, r32 = _refs(n)
    got = fe.melspec(wa.to(DEV), db=True).cpu().numpy()
    assert got.shape == r64.shape == (B, 80, 1 + n // 256, C) and got.dtype == np.float32
    g, h = np.abs(got.astype(np.float64) - r64).max(), np.abs(r32.astype(np.float64) - r64).max()
    print("melspec dB n=%d: kernel max|d| %.3e dB rms %.3e | host float32 max|d| %.3e dB rms %.3e | min %.2f dB, share at -80: %.4f"
          % (n, g, np.sqrt(((got - r64) ** 2).mean()), h, np.sqrt(((r32 - r64) ** 2).mean()), got.min(), (got == -80.0).mean()))
    assert np.isfinite(got).all()
    assert np.array_equal(got[2, :, :, 5], np.zeros_like(got[2, :, :, 5]))       # the silent channel: exactly 0 dB everywhere
    assert np.array_equal(got.max(axis=(1, 2)), np.zeros((B, C), np.float32))      # every (sample, channel) map peaks at exactly 0
    assert got.min() >= -80.0
    assert g <= 4.0 * h + LOG_SLACK, (g, h)


def test_clipped_map_of_a_pure_tone():
    """0.9 sin(2 pi 1000 t) + 1e-6 noise, n = 22050: most of the float64 map sits on the -80 dB floor.  The clip is 1-Lipschitz, so
    the error bound holds over ALL elements."""
    fe = _front()
    n = 22050
    t = np.arange(n, dtype=np.float64) / 44100.0
    y = (0.9 * np.sin(2.0 * np.pi * 1000.0 * t) + 1e-6 * np.random.default_rng(7).standard_normal(n)).astype(np.float32)
    r64, r32 = D.melspec_db_ref(y), D.melspec_db_ref(y, dtype=np.float32)
    got = fe.melspec(torch.from_numpy(y)[None, None].to(DEV), db=True)[0, :, :, 0].cpu().numpy()
    g, h = np.abs(got.astype(np.float64) - r64).max(), np.abs(r32.astype(np.float64) - r64).max()
    s_got, s_ref = (got == -80.0).mean(), (r64 == -80.0).mean()
    print("melspec dB clip case: kernel max|d| %.3e dB | host float32 %.3e dB | share at -80: kernel %.4f float64 %.4f" % (g, h, s_got, s_ref))
    assert got.min() == -80.0 and got.max() == 0.0
    assert g <= 4.0 * h + LOG_SLACK, (g, h)
    assert abs(s_got - s_ref) <= 0.01


@pytest.mark.parametrize("n", [2100, 33000])
def test_batch_equals_per_sample_bits(n):
    from mm_distillnet_amd import _lib
    fe = _front()
    wa, wb = (w.to(DEV) for w in _waves(n))
    T = fe.n_frames(n)
    for partner in (None, wb):
        power = _batch(fe, wa, partner, 0)
        db = _batch(fe, wa, partner, 1)
        for b in range(B):
            one = torch.empty(80, T, C, device=DEV)
            _lib.call("mmd_melspec_power", wa[b], None if partner is None else partner[b], C, n, fe.start, fe.length, fe.band, fe.stride, one)
            assert torch.equal(power[b], one), (b, partner is not None)
            alone = _batch(fe, wa[b:b + 1], None if partner is None else partner[b:b + 1], 1)
            assert torch.equal(db[b], alone[0]), (b, partner is not None)
        conv = power.clone()
        _lib.call("mmd_power_to_db", conv, B, 80, T, C, torch.empty(B * C, device=DEV))
        assert torch.equal(conv, db)
        assert torch.equal(fe.power_to_db(power.clone()), db)
        assert torch.equal(fe.melspec(wa, partner), power) and torch.equal(fe.melspec(wa, partner, db=True), db)


def test_two_launches_into_dirty_buffers_give_the_same_bits():
    from mm_distillnet_amd import _lib
    fe = _front()
    n = 2100
    wa, wb = (w.to(DEV) for w in _waves(n))
    T = fe.n_frames(n)
    o1 = torch.full((B, 80, T, C), float("nan"), device=DEV)
    o2 = torch.full((B, 80, T, C), -7.5e8, device=DEV)
    w1 = torch.full((B * C,), 0x7fffffff, dtype=torch.int32, device=DEV)
    w2 = torch.randint(-2 ** 31, 2 ** 31 - 1, (B * C,), dtype=torch.int64, device=DEV).to(torch.int32) | 1
    _batch(fe, wa, wb, 1, o1, w1.view(torch.float32)); _batch(fe, wa, wb, 1, o2, w2.view(torch.float32))
    torch.cuda.synchronize()
    assert torch.isfinite(o1).all() and torch.equal(o1, o2)
    assert torch.equal(o1, _batch(fe, wa, wb, 1))
    # the in-place conversion: the same two workspace states
    power = _batch(fe, wa, wb, 0)
    w1.fill_(0x7fffffff)
    w2 = torch.randint(-2 ** 31, 2 ** 31 - 1, (B * C,), dtype=torch.int64, device=DEV).to(torch.int32) | 1
    p1, p2 = power.clone(), power.clone()
    _lib.call("mmd_power_to_db", p1, B, 80, T, C, w1.view(torch.float32)); _lib.call("mmd_power_to_db", p2, B, 80, T, C, w2.view(torch.float32))
    assert torch.equal(p1, p2) and torch.equal(p1, o1)


@pytest.mark.parametrize("w,S", [(9, 96), (129, 64)])
def test_resize_batch_equals_per_sample_bits(w, S):
    from mm_distillnet_amd import _lib
    src = (torch.randn(B, 80, w, C, generator=torch.Generator().manual_seed(w)) * 15.0 - 40.0).to(DEV)
    got = torch.full((B, C, S, S), float("nan"), device=DEV)
    _lib.call("mmd_resize_cubic_batch", src, B, 80, w, C, S, got)
    for b in range(B):
        one = torch.empty(C, S, S, device=DEV)
        _lib.call("mmd_resize_cubic", src[b], 80, w, C, S, one)
        assert torch.equal(got[b], one), b
    assert torch.isfinite(got).all()


def test_device_pipeline_converts_waveform_samples_with_audio_db():
    from mm_distillnet_amd.data import RawSyntheticMultimodalDetection, DeviceInputPipeline, collate_raw
    fe = _front()
    cfg = {"seed": 24, "image_size": 96, "synthetic_wave_samples": 8000}
    wave = RawSyntheticMultimodalDetection(dict(cfg, audio_format="waveform", audio_db=True), length=3, frame_hw=(54, 72))
    spec = RawSyntheticMultimodalDetection(cfg, length=3, frame_hw=(54, 72), mel_hw=(32, 32))
    ws = [wave[i] for i in range(3)]
    wav = torch.stack([s["audio_wave"] for s in ws]).to(DEV)
    want_db, want_power = fe.student_input(wav, None, 96, db=True), fe.student_input(wav, None, 96)
    assert not torch.equal(want_db, want_power) and float(want_db.mean()) < -5.0          # dB maps, not power
    pipe = DeviceInputPipeline(96, DEV, audio_db=True)
    got = pipe.submit(ws).wait()["audio"].clone()
    stacked = pipe.submit(collate_raw(ws)).wait()["audio"].clone()
    # a list that mixes the two audio formats: the ready-made stack is untouched
    only_spec = DeviceInputPipeline(96, DEV).submit([spec[0]]).wait()["audio"].clone()
    mixed = pipe.submit([spec[0], wave[1], wave[2]]).wait()["audio"].clone()
    plain = DeviceInputPipeline(96, DEV).submit(ws).wait()["audio"].clone()          # key absent: today's power maps
    torch.cuda.synchronize()
    assert torch.equal(got, want_db) and torch.equal(stacked, want_db)
    assert torch.equal(mixed[0], only_spec[0]) and torch.equal(mixed[1:], want_db[1:])
    assert torch.equal(plain, want_power)
