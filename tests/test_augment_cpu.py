"""HSVAdjust + shift augmentation of the raw input pipeline, CPU side: tests/hsv_ref.py's colour conversions against the standard library's
colorsys, its closed forms, the fp32 distance that sets the GPU test's tolerance, `draw_augment`, train.py's reading of
train_transformations / data_augment_shift, and the C ABI of mmd_image_letterbox_aug_batch without a GPU."""
import colorsys
import ctypes
import inspect
import os

import numpy as np
import pytest

import hsv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "mm-distillnet.cfg")


def _grid():
    """greys, black, white, the primaries and secondaries, SPECIAL, and a 6^3 lattice of everything else"""
    lat = np.array([(r, g, b) for r in range(0, 256, 51) for g in range(0, 256, 51) for b in range(0, 256, 51)], dtype=np.float64)
    greys = np.repeat(np.array([0, 1, 17, 128, 254, 255], dtype=np.float64)[:, None], 3, 1)
    return np.concatenate([lat, greys, R.SPECIAL.astype(np.float64)]) / 255.0


# ---------------------------------------------------------------------------------------------- the colour conversions
def test_rgb_to_hsv_agrees_with_colorsys():
    rgb = _grid()
    h, s, v = R.rgb_to_hsv(rgb)
    for i, (r, g, b) in enumerate(rgb):
        ch, cs, cv = colorsys.rgb_to_hsv(r, g, b)
        assert abs(h[i] - ch * 360.0) < 1e-10 and abs(s[i] - cs) < 1e-14 and v[i] == cv, (r, g, b)
    assert np.all((h >= 0) & (h < 360))
    grey = rgb[:, 0] == rgb[:, 1]
    grey &= rgb[:, 1] == rgb[:, 2]
    assert grey.sum() >= 8 and np.all(h[grey] == 0) and np.all(s[grey] == 0)              # max = min: H = 0, S = 0 (and 0 at V = 0)
    # the maximal channel is taken in R, G, B order: R = G > B is V = R (hue 60), G = B > R is V = G (180), R = B > G is V = R (300)
    hh, _, _ = R.rgb_to_hsv(np.array([[200, 200, 10], [10, 200, 200], [200, 10, 200]]) / 255.0)
    np.testing.assert_allclose(hh, [60.0, 180.0, 300.0], atol=1e-12)


def test_hsv_to_rgb_agrees_with_colorsys():
    hs = np.array([0.0, 15.0, 59.999, 60.0, 90.0, 120.0, 179.5, 180.0, 240.0, 299.0, 300.0, 330.0, 359.999])
    for s in (0.0, 0.3, 1.0):
        for v in (0.0, 0.4, 1.0):
            got = R.hsv_to_rgb(hs, np.full_like(hs, s), np.full_like(hs, v))
            want = np.array([colorsys.hsv_to_rgb(h / 360.0, s, v) for h in hs])
            np.testing.assert_allclose(got, want, atol=1e-13)
    # h = 360 (a hue that wrapped onto the boundary) is h = 0
    np.testing.assert_allclose(R.hsv_to_rgb(360.0, 0.7, 0.9), R.hsv_to_rgb(0.0, 0.7, 0.9), atol=1e-15)


def test_identity_parameters_round_trip():
    frame = (_grid() * 255.0).reshape(-1, 1, 3)
    np.testing.assert_allclose(R.hsv_adjust(frame, 0.0, 1.0, 1.0), frame, rtol=0, atol=255 * 8 * np.finfo(np.float64).eps)
    # a full turn of the hue is the identity too, and black / white / grey stay what they are under any hue
    np.testing.assert_allclose(R.hsv_adjust(R.hsv_adjust(frame, 25.0, 1.0, 1.0), -25.0, 1.0, 1.0), frame, atol=1e-10)
    grey = np.array([[[0, 0, 0], [255, 255, 255], [128, 128, 128]]], dtype=np.float64)
    np.testing.assert_allclose(R.hsv_adjust(grey, -29.0, 1.5, 1.0), grey, atol=1e-12)


def test_adjust_wraps_and_clips():
    px = np.array([[[255, 0, 40], [255, 40, 0], [255, 0, 0]]], dtype=np.float64)
    h0, _, _ = R.rgb_to_hsv(px / 255.0)
    assert h0[0, 0] > 330 and h0[0, 1] < 30
    up, _, _ = R.rgb_to_hsv(R.hsv_adjust(px, 30.0, 1.0, 1.0) / 255.0)
    dn, _, _ = R.rgb_to_hsv(R.hsv_adjust(px, -30.0, 1.0, 1.0) / 255.0)
    np.testing.assert_allclose(up[0, 0], h0[0, 0] + 30 - 360, atol=1e-9)                  # past 360
    np.testing.assert_allclose(dn[0, 1], h0[0, 1] - 30 + 360, atol=1e-9)                  # below 0
    np.testing.assert_allclose(R.hsv_adjust(px, 0.0, 1.5, 1.5)[0, 2], [255, 0, 0], atol=1e-12)      # S and V clip at 1
    np.testing.assert_allclose(R.hsv_adjust(px, 0.0, 1.0, 0.5)[0, 2], [127.5, 0, 0], atol=1e-12)    # no rounding


def test_shift_and_letterbox_pieces():
    img = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3) + 1
    s = R.shift_frame(img, 2)
    assert np.array_equal(s[:, :5], img[:, 2:]) and np.all(s[:, 5:] == 0)
    # all-off row = the oracle's plain chain
    from oracle import input_ref as I
    off = np.array([0, 0, 1, 1, 0], dtype=np.float32)
    np.testing.assert_allclose(R.prepare_colour(img, off, 8, np.float64, I.IMAGENET_MEAN, I.IMAGENET_STD), I.prepare_rgb(img, 8), atol=1e-6)
    th = R.thermal_frames(5, 7)[0]
    np.testing.assert_allclose(R.prepare_thermal(th, off, 8), I.prepare_thermal(th, 8), atol=1e-7)
    # shifted thermal: the stretch is the unshifted frame's, the vacated columns are 0
    sh = R.prepare_thermal(th, np.array([1, 9, 9, 9, 2], dtype=np.float32), 7)              # S = W: the resize is the identity
    full = R.prepare_thermal(th, off, 7)
    np.testing.assert_allclose(sh[0, :5, :5], full[0, :5, 2:], atol=1e-15)
    assert np.all(sh[0, :5, 5:] == 0)


def test_fp32_distance_is_what_the_gpu_tolerance_assumes():
    """R.MEASURED_FP32_DISTANCE, from which tests/test_gpu_augment.py takes its tolerance, is this measurement (1.002e-6)"""
    d = R.fp32_distance()
    print("hsv_ref float32 vs float64 on the GPU test's inputs: max |diff| = %.3e" % d)
    assert 0.5 * R.MEASURED_FP32_DISTANCE < d <= R.MEASURED_FP32_DISTANCE
    assert 4 * R.MEASURED_FP32_DISTANCE < 2e-5


def test_frames_hold_the_hard_pixels():
    for H, W, _ in R.SHAPES:
        fr = R.colour_frames(H, W)
        for b in range(3):
            flat = {tuple(p) for p in fr[b].reshape(-1, 3)}
            assert all(tuple(p) in flat for p in R.SPECIAL), (H, W, b)
            assert fr[b][:, -2:].any()                                               # the columns the shift drops are not empty
    for tab in R.TABLES.values():
        assert tab[0].tolist() == [0, 0, 1, 1, 0] and tab[1, 0] == 1 and tab[1, 4] == 0 and tab[2, 0] == 1 and tab[2, 4] == 2
    assert {np.sign(t[1, 1]) for t in R.TABLES.values()} == {1.0, -1.0}


# ---------------------------------------------------------------------------------------------- the host's draws
def test_draw_augment_is_deterministic_and_in_range():
    from mm_distillnet_amd.data import draw_augment
    a = draw_augment(np.random.default_rng(7), 4000, True, True)
    b = draw_augment(np.random.default_rng(7), 4000, True, True)
    c = draw_augment(np.random.default_rng(8), 4000, True, True)
    assert a.dtype == np.float32 and a.shape == (4000, 5) and np.array_equal(a, b) and not np.array_equal(a, c)
    assert np.all(a[:, 0] == 1) and np.all(np.abs(a[:, 1]) <= 30)
    for col in (2, 3):
        assert np.all((a[:, col] >= np.float32(1 / 1.5)) & (a[:, col] <= 1.5))
        assert 0.45 < np.mean(a[:, col] < 1) < 0.55                                   # the coin: below 1 about half the time
    assert set(np.unique(a[:, 4])) == {0.0, 2.0} and 0.45 < np.mean(a[:, 4] == 2) < 0.55
    assert a[:, 1].min() < -25 and a[:, 1].max() > 25
    # the documented draw order: hue, sat, sat's coin, val, val's coin, shift's coin
    rng = np.random.default_rng(7)
    hue, sat, c1, val, c2, c3 = rng.uniform(-30, 30), rng.uniform(1, 1.5), rng.uniform(0, 1), rng.uniform(1, 1.5), rng.uniform(0, 1), rng.uniform(0, 1)
    want = [1.0, hue, 1 / sat if c1 >= 0.5 else sat, 1 / val if c2 >= 0.5 else val, 2.0 if c3 > 0.5 else 0.0]
    np.testing.assert_array_equal(a[0], np.array(want, dtype=np.float32))
    # a transform that is off draws nothing and leaves its columns neutral
    only_shift = draw_augment(np.random.default_rng(7), 50, False, True)
    assert np.all(only_shift[:, :4] == [0, 0, 1, 1]) and set(np.unique(only_shift[:, 4])) == {0.0, 2.0}
    only_hsv = draw_augment(np.random.default_rng(7), 50, True, False)
    assert np.all(only_hsv[:, 4] == 0) and np.all(only_hsv[:, 0] == 1)
    assert np.array_equal(draw_augment(np.random.default_rng(7), 3, False, False), np.array([[0, 0, 1, 1, 0]] * 3, dtype=np.float32))


def test_pipeline_takes_augment_settings():
    from mm_distillnet_amd.data import AugmentSettings, DeviceInputPipeline
    assert inspect.signature(DeviceInputPipeline.__init__).parameters["augment"].default is None
    assert inspect.signature(DeviceInputPipeline.submit).parameters["aug"].default is None
    s = AugmentSettings(hsv=True, shift=False, seed=3)
    assert (s.hsv, s.shift, s.seed) == (True, False, 3) and AugmentSettings() == AugmentSettings(False, False, 0)
    assert "thermal" in DeviceInputPipeline.__doc__ and "HSVAdjust" in DeviceInputPipeline.__doc__


# ---------------------------------------------------------------------------------------------- train.py's parsing
def _cfg(overwrite=None, rank=0):
    import json
    import sys
    sys.path.insert(0, ROOT)
    import train
    argv = ["--config_file", CFG, "--rank", str(rank)]
    if overwrite:
        argv += ["--overwrite", json.dumps(overwrite)]
    cfg, args = train.parse_config(argv)
    return train, cfg, args


def test_train_defaults_are_unchanged():
    train, cfg, _ = _cfg()
    assert "train_transformations" not in cfg and "data_augment_shift" not in cfg          # the shipped recipe has neither key
    assert train.augment_from_config(cfg, raw=False) is None and train.augment_from_config(cfg, raw=True) is None
    train, cfg, _ = _cfg({"train_transformations": "Normalizer,Resizer", "data_augment_shift": "False"})
    assert train.augment_from_config(cfg, raw=False) is None and train.augment_from_config(cfg, raw=True) is None


def test_train_reads_hsv_and_shift():
    from mm_distillnet_amd.data import AugmentSettings
    train, cfg, args = _cfg({"train_transformations": "HSVAdjust,Normalizer,Resizer", "input_pipeline": "raw"}, rank=3)
    assert train.augment_from_config(cfg, True, args.rank) == AugmentSettings(hsv=True, shift=False, seed=cfg.getint("seed") + 3)
    train, cfg, _ = _cfg({"data_augment_shift": "True", "input_pipeline": "raw", "seed": 5})
    assert train.augment_from_config(cfg, True, 0) == AugmentSettings(hsv=False, shift=True, seed=5)
    train, cfg, _ = _cfg({"train_transformations": "HSVAdjust,Normalizer,Resizer", "data_augment_shift": "True"})
    assert train.augment_from_config(cfg, True, 1) == AugmentSettings(hsv=True, shift=True, seed=25)


def test_train_refuses_what_it_cannot_run():
    train, cfg, _ = _cfg({"train_transformations": "Normalizer,Resizer,Blur"})
    with pytest.raises(Exception, match="^No valid transformation Blur provided$"):
        train.augment_from_config(cfg, True)
    train, cfg, _ = _cfg({"train_transformations": "Normalizer, Resizer"})                   # upstream does not strip the names
    with pytest.raises(Exception, match="^No valid transformation  Resizer provided$"):
        train.augment_from_config(cfg, True)
    train, cfg, _ = _cfg({"train_transformations": "HSVAdjust,Normalizer,Resizer"})
    with pytest.raises(Exception, match="HSVAdjust needs input_pipeline = raw"):
        train.augment_from_config(cfg, False)
    train, cfg, _ = _cfg({"data_augment_shift": "True"})
    with pytest.raises(Exception, match="data_augment_shift = True needs input_pipeline = raw"):
        train.augment_from_config(cfg, False)
    for name, why in (("ThermalAugmenter", "albumentations"), ("AudioAugmenter", "None"), ("Resize", "Resizer")):
        train, cfg, _ = _cfg({"train_transformations": f"{name},Normalizer,Resizer"})
        with pytest.raises(Exception, match=f"{name} .*not available.*{why}"):
            train.augment_from_config(cfg, True)
    for order in ("Normalizer,HSVAdjust,Resizer", "HSVAdjust,Resizer", "Resizer,Normalizer", "HSVAdjust,HSVAdjust,Normalizer,Resizer"):
        train, cfg, _ = _cfg({"train_transformations": order})
        with pytest.raises(Exception, match="Unsupported train_transformations"):
            train.augment_from_config(cfg, True)


# ---------------------------------------------------------------------------------------------- C ABI without a GPU
def test_entry_point_is_declared_and_validates_before_any_launch():
    import __graft_entry__ as ge
    ge.build()
    from mm_distillnet_amd import _lib
    sigs = _lib.LIB.symbols()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    name = "mmd_image_letterbox_aug_batch"
    assert name in sigs and hasattr(dll, name) and len(sigs[name]) == 17
    text = open(_lib.HEADER).read()
    head = text[:text.index("int %s(" % name)]
    comment = head[head.rindex("\n\n"):]
    assert "transformations.py:133-190" in comment and "MultimodalDetection.py:236-242,320-327" in comment
    assert "UNPINNED" in comment and "tests/hsv_ref.py" in comment and "exactly the bits of mmd_image_letterbox" in comment
    src = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "input.hip")).read()
    assert "UNPINNED" in src[src.index("HSVAdjust"):src.index("hsv_adjust(")]
    fn = _lib.LIB.load().mmd_image_letterbox_aug_batch
    p = ctypes.c_void_p(4096)            # never dereferenced: validation precedes any launch

    def rc(src=p, B=3, H=5, W=7, C=3, mm=None, aug=p, hsv=1, S=8, dst=p, minmax=0):
        return fn(src, B, H, W, C, 1.0 / 255.0, None, None, minmax, 20800.0, 27000.0, mm, aug, hsv, S, dst, None)

    assert rc(src=None) == -22 and rc(aug=None) == -22 and rc(dst=None) == -22
    assert rc(C=1, hsv=0, minmax=1, mm=None) == -22                                   # the stretch needs its (min, max)
    assert rc(B=0) == -22 and rc(H=0) == -22 and rc(W=0) == -22 and rc(S=0) == -22 and rc(B=-1) == -22
    assert rc(C=2) == -22 and rc(C=4) == -22 and rc(C=0) == -22
    assert rc(C=1, hsv=1, mm=p, minmax=1) == -22 and rc(C=1, hsv=1) == -22             # HSVAdjust on the 1-channel thermal frame
    assert rc(C=3, minmax=1, mm=p) == -22
    assert rc(H=1, W=4000, S=8) == -22                                                 # the resized height would be 0 rows
