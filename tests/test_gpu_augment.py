"""GPU: mmd_image_letterbox_aug_batch (csrc/input.hip) - the reference's HSVAdjust and 2-pixel column shift in front of Normalizer + Resizer,
one launch per stacked batch of a modality - against tests/hsv_ref.py in float64, against mmd_image_letterbox bit for bit where nothing is
augmented (and where only the shift is), and through DeviceInputPipeline (stacked / list / no augment).

Tolerance.  The composite map RGB -> HSV -> adjust -> RGB is continuous, so the kernel's fp32 stays close to float64; how close is measured
on the CPU on exactly these inputs (tests/test_augment_cpu.py::test_fp32_distance_is_what_the_gpu_tolerance_assumes): hsv_ref in float32
differs from hsv_ref in float64 by at most 1.002e-6.  The kernel is allowed four times that (contraction, another operation order) = 4.0e-6,
which is below the floor - the rtol 1e-5, atol 2e-5 (rgb) / 2e-6 (depth, thermal: values in [0, 1]) of tests/test_input_pipeline.py - so the
comparisons run at atol = max(4 x measured, floor): the floor for rgb, 4.04e-6 for depth; thermal takes no HSV and stays at its floor, 2e-6.
No pixel is excluded.  On an MI355X the kernel's largest |difference from float64| over all cases is 1.0e-6 (rgb) and 3.9e-7 (depth)."""
import functools

import numpy as np
import pytest
import torch

import hsv_ref as R
from oracle import input_ref as I

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 1e-5
ATOL_RGB = max(4 * R.MEASURED_FP32_DISTANCE, 2e-5)
ATOL_01 = max(4 * R.MEASURED_FP32_DISTANCE, 2e-6)      # depth: plain /255, values in [0, 1]
ATOL_THERMAL = 2e-6                                    # no HSV on thermal: the existing floor
IR = (20800.0, 27000.0)


def _call(*a):
    from mm_distillnet_amd import _lib
    return _lib.call(*a)


def _stats():
    return (torch.tensor(I.IMAGENET_MEAN, dtype=torch.float32, device=DEV), torch.tensor(I.IMAGENET_STD, dtype=torch.float32, device=DEV))


@functools.lru_cache(maxsize=None)
def _refs(H, W, S, table, modality):
    """float64 [3, 3, S, S] of hsv_ref for one case; computed once and left unchanged"""
    stats = (I.IMAGENET_MEAN, I.IMAGENET_STD) if modality == "rgb" else (None, None)
    r = R.colour_refs(R.colour_frames(H, W, seed=0 if modality == "rgb" else 1), R.TABLES[table], S, np.float64, *stats)
    r.setflags(write=False)
    return r


def _plain(frame_dev, H, W, S, mean, std):
    out = torch.full((3, S, S), 7.0, device=DEV)
    _call("mmd_image_letterbox", frame_dev, 0, H, W, 3, 1.0 / 255.0, mean, std, 0, 0.0, 0.0, None, S, out)
    return out


@pytest.mark.parametrize("table", sorted(R.TABLES))
@pytest.mark.parametrize("H,W,S", R.SHAPES)
def test_colour_batch_matches_float64_and_plain_bits(H, W, S, table):
    tab = torch.from_numpy(R.TABLES[table]).to(DEV)
    for modality, seed, (mean, std), atol in (("rgb", 0, _stats(), ATOL_RGB), ("depth", 1, (None, None), ATOL_01)):
        frames = torch.from_numpy(R.colour_frames(H, W, seed=seed)).to(DEV)
        got = torch.full((3, 3, S, S), 7.0, device=DEV)                          # dirty: the letterbox border is written too
        _call("mmd_image_letterbox_aug_batch", frames, 3, H, W, 3, 1.0 / 255.0, mean, std, 0, 0.0, 0.0, None, tab, 1, S, got)
        # the all-off sample: exactly mmd_image_letterbox's bits
        assert torch.equal(got[0], _plain(frames[0], H, W, S, mean, std)), modality
        # every sample, every pixel against float64
        ref = _refs(H, W, S, table, modality)
        diff = np.abs(got.cpu().numpy().astype(np.float64) - ref)
        print("%s %s (%d,%d,%d): max |kernel - float64| per sample %s" % (modality, table, H, W, S, diff.reshape(3, -1).max(1)))
        np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=RTOL, atol=atol, err_msg=modality)
        # the augmentation did something: the adjusted samples are far from their un-augmented selves
        for b in (1, 2):
            assert (got[b] - _plain(frames[b], H, W, S, mean, std)).abs().max() > 0.05
        # hsv = 0 ignores the `on` column (the form the thermal launch uses): rows 0 and 1 are plain, row 2 is the shift alone
        noh = torch.full((3, 3, S, S), 7.0, device=DEV)
        _call("mmd_image_letterbox_aug_batch", frames, 3, H, W, 3, 1.0 / 255.0, mean, std, 0, 0.0, 0.0, None, tab, 0, S, noh)
        shifted = torch.from_numpy(R.shift_frame(R.colour_frames(H, W, seed=seed)[2], 2)).to(DEV)
        assert torch.equal(noh[0], got[0]) and torch.equal(noh[1], _plain(frames[1], H, W, S, mean, std))
        assert torch.equal(noh[2], _plain(shifted, H, W, S, mean, std)), modality


@pytest.mark.parametrize("H,W,S", R.SHAPES)
def test_thermal_shift_matches_shifted_frame_through_plain_path(H, W, S):
    th = R.thermal_frames(H, W)
    tab_np = np.array([[1, 20, 1.2, 1.2, 0], [0, 0, 1, 1, 2], [1, -20, 0.8, 0.8, 2]], dtype=np.float32)      # `on` is ignored with hsv = 0
    tdev = torch.from_numpy(th.view(np.int16)).to(DEV)                          # torch has no uint16 arithmetic; the bytes are what travels
    mm = torch.zeros(3, 2, device=DEV)
    for b in range(3):
        _call("mmd_image_minmax", tdev[b], 1, H * W, IR[0], IR[1], mm[b])
    got = torch.full((3, 1, S, S), 7.0, device=DEV)
    _call("mmd_image_letterbox_aug_batch", tdev, 3, H, W, 1, 1.0 / 255.0, None, None, 1, IR[0], IR[1], mm, torch.from_numpy(tab_np).to(DEV),
          0, S, got)
    for b in range(3):
        # the existing path on the shifted frame, stretched with the UNSHIFTED frame's (min, max); its vacated columns hold the clamped
        # minimum, the count that stretches to the 0 upstream's shift-after-stretch leaves there
        sh = th[b].copy()
        if tab_np[b, 4] > 0:
            sh = R.shift_frame(sh, 2)
            sh[:, W - 2:] = np.uint16(np.clip(th[b], *IR).min())
        one = torch.full((1, S, S), 7.0, device=DEV)
        _call("mmd_image_letterbox", torch.from_numpy(sh.view(np.int16)).to(DEV), 1, H, W, 1, 1.0 / 255.0, None, None, 1, IR[0], IR[1], mm[b], S, one)
        assert torch.equal(got[b], one), b
        np.testing.assert_allclose(got[b].cpu().numpy(), R.prepare_thermal(th[b], tab_np[b], S), rtol=RTOL, atol=ATOL_THERMAL)
    assert not torch.equal(got[1], got[2]) and (got[1, 0, :, -1] == 0).all()


def test_bad_arguments_return_minus_22():
    H, W, S = 5, 7, 8
    frames = torch.from_numpy(R.colour_frames(H, W)).to(DEV)
    th = torch.from_numpy(R.thermal_frames(H, W).view(np.int16)).to(DEV)
    tab = torch.from_numpy(R.TABLES["up"]).to(DEV)
    out3, out1, mm = torch.full((3, 3, S, S), 7.0, device=DEV), torch.full((3, 1, S, S), 7.0, device=DEV), torch.zeros(3, 2, device=DEV)
    bad = [
        ("HSV with C = 1", (th, 3, H, W, 1, 1.0 / 255.0, None, None, 1, IR[0], IR[1], mm, tab, 1, S, out1)),
        ("null src", (None, 3, H, W, 3, 1.0 / 255.0, None, None, 0, 0.0, 0.0, None, tab, 1, S, out3)),
        ("null aug", (frames, 3, H, W, 3, 1.0 / 255.0, None, None, 0, 0.0, 0.0, None, None, 1, S, out3)),
        ("null dst", (frames, 3, H, W, 3, 1.0 / 255.0, None, None, 0, 0.0, 0.0, None, tab, 1, S, None)),
        ("null mm", (th, 3, H, W, 1, 1.0 / 255.0, None, None, 1, IR[0], IR[1], None, tab, 0, S, out1)),
        ("B = 0", (frames, 0, H, W, 3, 1.0 / 255.0, None, None, 0, 0.0, 0.0, None, tab, 1, S, out3)),
        ("C = 2", (frames, 3, H, W, 2, 1.0 / 255.0, None, None, 0, 0.0, 0.0, None, tab, 1, S, out3)),
    ]
    for what, args in bad:
        with pytest.raises(RuntimeError, match="mmd_image_letterbox_aug_batch failed with status -22"):
            _call("mmd_image_letterbox_aug_batch", *args)
    torch.cuda.synchronize()
    assert (out3 == 7.0).all() and (out1 == 7.0).all(), "a refused call launched"


# ---------------------------------------------------------------------------------------------- DeviceInputPipeline
def _samples(n=3):
    from mm_distillnet_amd.data import RawSyntheticMultimodalDetection
    ds = RawSyntheticMultimodalDetection({"seed": 24, "image_size": 48}, length=n, frame_hw=(27, 36), mel_hw=(16, 16))
    return [ds[i] for i in range(n)]


def _take(pipe, samples, **kw):
    return {k: v.clone() for k, v in pipe.submit(samples, **kw).wait().items()}


def test_pipeline_stacked_equals_list_and_float64():
    from mm_distillnet_amd.data import DeviceInputPipeline, collate_raw
    samples, tab = _samples(), R.TABLES["up"]
    pipe = DeviceInputPipeline(48, DEV)
    lst = _take(pipe, samples, aug=tab)                       # B = 1 launches
    stk = _take(pipe, collate_raw(samples), aug=tab)          # one launch per modality
    torch.cuda.synchronize()
    for k in lst:
        assert torch.equal(lst[k], stk[k]), k
    for b, s in enumerate(samples):
        np.testing.assert_allclose(stk["rgb"][b].cpu().numpy(), R.prepare_colour(s["rgb"].numpy(), tab[b], 48, np.float64, I.IMAGENET_MEAN, I.IMAGENET_STD),
                                   rtol=RTOL, atol=ATOL_RGB)
        np.testing.assert_allclose(stk["depth"][b].cpu().numpy(), R.prepare_colour(s["depth"].numpy(), tab[b], 48), rtol=RTOL, atol=ATOL_01)
        np.testing.assert_allclose(stk["thermal"][b].cpu().numpy(), R.prepare_thermal(s["thermal"].numpy().view(np.uint16), tab[b], 48),
                                   rtol=RTOL, atol=ATOL_THERMAL)
        np.testing.assert_allclose(stk["audio"][b].cpu().numpy(), I.prepare_audio(s["audio"].numpy(), 48), rtol=1e-5, atol=2e-4)
    with pytest.raises(ValueError, match="aug must be"):
        pipe.submit(samples, aug=tab[:2])


def test_pipeline_without_augment_is_todays_output():
    from mm_distillnet_amd.data import AugmentSettings, DeviceInputPipeline, collate_raw
    samples = _samples()
    S = 48
    mean, std = _stats()
    # today's launches, issued by hand
    want = {"rgb": torch.empty(3, 3, S, S, device=DEV), "depth": torch.empty(3, 3, S, S, device=DEV), "thermal": torch.empty(3, 1, S, S, device=DEV)}
    mm = torch.zeros(3, 2, device=DEV)
    for b, s in enumerate(samples):
        H, W = s["rgb"].shape[:2]
        _call("mmd_image_letterbox", s["rgb"].to(DEV), 0, H, W, 3, 1.0 / 255.0, mean, std, 0, 0.0, 0.0, None, S, want["rgb"][b])
        _call("mmd_image_letterbox", s["depth"].to(DEV), 0, H, W, 3, 1.0 / 255.0, None, None, 0, 0.0, 0.0, None, S, want["depth"][b])
        t = s["thermal"].to(DEV)
        _call("mmd_image_minmax", t, 1, H * W, IR[0], IR[1], mm[b])
        _call("mmd_image_letterbox", t, 1, H, W, 1, 1.0 / 255.0, None, None, 1, IR[0], IR[1], mm[b], S, want["thermal"][b])
    plain = DeviceInputPipeline(S, DEV)
    assert plain.augment is None
    off = DeviceInputPipeline(S, DEV, augment=AugmentSettings(hsv=False, shift=False, seed=1))       # the new entry point, every row all-off
    for batch in (samples, collate_raw(samples)):
        a, o = _take(plain, batch), _take(off, batch)
        torch.cuda.synchronize()
        for k in want:
            assert torch.equal(a[k], want[k]) and torch.equal(o[k], want[k]), k
        assert torch.equal(a["audio"], o["audio"])


def test_pipeline_draws_from_its_seed():
    from mm_distillnet_amd.data import AugmentSettings, DeviceInputPipeline, collate_raw, draw_augment
    batch = collate_raw(_samples())
    cfg = AugmentSettings(hsv=True, shift=True, seed=11)
    p1, p2, plain = DeviceInputPipeline(48, DEV, augment=cfg), DeviceInputPipeline(48, DEV, augment=cfg), DeviceInputPipeline(48, DEV)
    rng = np.random.default_rng(11)
    for _ in range(2):                                          # the generator carries on from submit to submit
        a, b = _take(p1, batch), _take(p2, batch)
        c = _take(plain, batch, aug=draw_augment(rng, 3, True, True))
        torch.cuda.synchronize()
        for k in a:
            assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
    assert not torch.equal(a["rgb"], _take(plain, batch)["rgb"])


def test_train_main_refuses_augmentation_on_the_tensor_path(tmp_path, monkeypatch):
    """train.py reads the two keys before it loads anything: on the tensor path they end the job with a message that says why"""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.chdir(tmp_path)
    sys.path.insert(0, root)
    import train
    cfgf = os.path.join(root, "configs", "mm-distillnet.cfg")
    ov = '{"image_size": 128, "batch_size": 2, "synthetic_length": 4, "exp_name": "exp", "resume": "False", "num_workers": 0, %s}'
    with pytest.raises(Exception, match="HSVAdjust needs input_pipeline = raw"):
        train.main(["--config_file", cfgf, "--overwrite", ov % '"train_transformations": "HSVAdjust,Normalizer,Resizer"', "--max_steps", "1"])
    with pytest.raises(Exception, match="data_augment_shift = True needs input_pipeline = raw"):
        train.main(["--config_file", cfgf, "--overwrite", ov % '"data_augment_shift": "True"', "--max_steps", "1"])
    with pytest.raises(Exception, match="No valid transformation Blur provided"):
        train.main(["--config_file", cfgf, "--overwrite", ov % '"input_pipeline": "raw", "train_transformations": "Blur,Normalizer,Resizer"',
                    "--max_steps", "1"])
