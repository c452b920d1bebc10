"""Helper (not a test): numpy restatement of what mmd_image_letterbox_aug_batch (csrc/input.hip) computes - the reference's 2-pixel column
shift (src/datasets/MultimodalDetection.py:236-242,320-327), HSVAdjust (src/datasets/transformations.py:133-190), Normalizer and the
Resizer letterbox - in a chosen dtype: float64 is the yardstick, float32 the same statement in the kernel's number format (their distance on
the test inputs sets the GPU test's tolerance).  The resize is oracle/input_ref.py's (float64 in both).

cv2.cvtColor is not on hand: the colour conversions follow OpenCV's DOCUMENTED float formulas
    V = max(R, G, B);  S = (V - min)/V, 0 at V = 0;
    H = 60 (G - B)/(V - min) at V = R, 120 + 60 (B - R)/(V - min) at V = G, 240 + 60 (R - G)/(V - min) at V = B (the maximal channel in R, G, B
    order), + 360 if negative, 0 where max = min;  the inverse is the six-sector form,
so parity with cv2 itself is UNPINNED (its float code adds FLT_EPSILON to both divisors); tests/test_augment_cpu.py pins them to the standard
library's colorsys, an independent statement of the same formulas.

Also here: the frames, tables and shapes that tests/test_gpu_augment.py runs and tests/test_augment_cpu.py measures."""
import numpy as np

from oracle import input_ref as I


def rgb_to_hsv(rgb, dtype=np.float64):
    """rgb [..., 3] in [0, 1] -> (h in [0, 360), s, v), each [...] of `dtype`."""
    a = np.asarray(rgb, dtype=dtype)
    r, g, b = a[..., 0], a[..., 1], a[..., 2]
    zero, one = dtype(0), dtype(1)
    v = np.maximum(r, np.maximum(g, b))
    d = v - np.minimum(r, np.minimum(g, b))
    s = np.where(v != 0, d / np.where(v != 0, v, one), zero)
    dd = np.where(d != 0, d, one)
    h = np.where(v == r, dtype(60) * (g - b) / dd, np.where(v == g, dtype(120) + dtype(60) * (b - r) / dd, dtype(240) + dtype(60) * (r - g) / dd))
    h = np.where(h < 0, h + dtype(360), h)
    return np.where(d != 0, h, zero), s, v


def hsv_to_rgb(h, s, v, dtype=np.float64):
    """(h degrees, s, v) -> rgb [..., 3]: the six-sector inverse (sector = floor(h/60) mod 6, so h = 360 is sector 0)."""
    h, s, v = (np.asarray(t, dtype=dtype) for t in (h, s, v))
    one = dtype(1)
    hs = h / dtype(60)
    fl = np.floor(hs)
    f = hs - fl
    sec = fl.astype(np.int64) % 6
    p, q, t = v * (one - s), v * (one - s * f), v * (one - s * (one - f))
    r = np.choose(sec, [v, q, p, p, t, v])
    g = np.choose(sec, [t, v, v, q, p, p])
    b = np.choose(sec, [p, p, t, v, v, q])
    return np.stack([r, g, b], -1).astype(dtype)


def hsv_adjust(frame, hue, sat, val, dtype=np.float64):
    """HSVAdjust.__call__ on one [H, W, 3] frame of 0..255 values with its three draws -> [H, W, 3] of 0..255 values, not rounded."""
    h, s, v = rgb_to_hsv(np.asarray(frame, dtype=dtype) / dtype(255), dtype)
    h = h + dtype(hue)
    h = np.where(h >= 360, h - dtype(360), h)          # clip_hue: one wrap each way, in this order
    h = np.where(h < 0, h + dtype(360), h)
    s = np.clip(dtype(sat) * s, dtype(0), dtype(1))
    v = np.clip(dtype(val) * v, dtype(0), dtype(1))
    return hsv_to_rgb(h, s, v, dtype) * dtype(255)


def shift_frame(img, shift: int):
    """MultimodalDetection.shift: img_new[:, 0:W-shift] = img[:, shift:], zeros elsewhere."""
    out = np.zeros_like(img)
    if shift < img.shape[1]:
        out[:, :img.shape[1] - shift] = img[:, shift:]
    return out


def _normalise(x, dtype, mean, std):
    """the kernel's (v * scale - mean) * (1/std) in float32; the plain (v/255 - mean)/std in float64"""
    if mean is None:
        mean, std = np.zeros(x.shape[-1]), np.ones(x.shape[-1])
    if dtype is np.float32:
        m, inv = np.asarray(mean, np.float32), np.float32(1) / np.asarray(std, np.float32)
        return (x * np.float32(1.0 / 255.0) - m) * inv
    return (x / 255.0 - np.asarray(mean, np.float64)) / np.asarray(std, np.float64)


def prepare_colour(raw_u8, row, common_size, dtype=np.float64, mean=None, std=None):
    """uint8 [H, W, 3] + one table row (on, hue_deg, sat, val, shift_px) -> float64 [3, S, S]: shift, HSVAdjust, Normalizer (mean / std; None
    = depth's plain /255), letterbox.  Upstream's order is /255, shift, HSVAdjust: shifting the raw frame first is the same thing, a vacated
    pixel being 0 either way."""
    on, hue, sat, val, shift = (float(t) for t in row)
    x = np.asarray(raw_u8, dtype=dtype)
    if shift > 0:
        x = shift_frame(x, int(shift))
    if on != 0:
        x = hsv_adjust(x, hue, sat, val, dtype)
    x = _normalise(x, dtype, mean, std)
    return np.transpose(I.letterbox(x.astype(np.float64), common_size), (2, 0, 1))


def prepare_thermal(raw_u16, row, common_size, dtype=np.float64, ir_min=20800.0, ir_max=27000.0):
    """uint16 [H, W] + one table row -> float64 [1, S, S]: clamp, min-max stretch to 0..255 with round-half-even (of the UNSHIFTED frame),
    then the shift (zeros in the stretched frame, as upstream shifts after cv2.normalize), /255, letterbox.  The `on` column is ignored."""
    shift = int(row[4])
    t = np.clip(np.asarray(raw_u16).astype(dtype), dtype(ir_min), dtype(ir_max))
    mn, mx = t.min(), t.max()
    k = dtype(255) / (mx - mn) if mx > mn else dtype(0)
    t = np.rint((t - mn) * k)
    if shift > 0:
        t = shift_frame(t, shift)
    t = _normalise(t[:, :, None], dtype, None, None)[:, :, 0]
    return I.letterbox(t.astype(np.float64), common_size)[None]


# ---------------------------------------------------------------------------------------------- the GPU test's inputs
SHAPES = [(5, 7, 8), (37, 23, 16), (64, 48, 32)]          # (H, W, S): upscale, H > W, downscale

# the pixels at which the rule can go wrong: 17 of them, so the smallest frame (5 x 7, 18 special positions) holds each one
SPECIAL = np.array([
    (0, 0, 0), (255, 255, 255), (128, 128, 128), (1, 1, 1),                  # black, white, greys: S = 0, H = 0
    (255, 0, 0), (0, 255, 0), (0, 0, 255),                                   # the primaries: S = 1 (sat > 1 clips), V = 1 (val > 1 clips)
    (200, 200, 10), (10, 200, 200), (200, 10, 200), (255, 255, 0),           # two channels tie for the maximum
    (255, 0, 40), (250, 3, 20),                                              # hue in (330, 360): + 30 wraps past 360
    (255, 40, 0), (90, 12, 7),                                               # hue in (0, 30): - 30 wraps below 0
    (240, 100, 60), (30, 60, 20),                                            # bright / saturated enough to clip under 1.5, and one that is not
], dtype=np.uint8)

# rows (on, hue_deg, sat, val, shift_px): all off, HSV only, HSV + shift; the second table swaps the signs and the sides of 1
TABLES = {
    "up": np.array([[0, 0, 1, 1, 0], [1, 27.5, 1.4375, 1.3125, 0], [1, -28.25, 1 / 1.3, 1 / 1.2, 2]], dtype=np.float32),
    "down": np.array([[0, 0, 1, 1, 0], [1, -29.75, 1 / 1.45, 1.49, 0], [1, 29.9, 1.5, 1 / 1.5, 2]], dtype=np.float32),
}


def colour_frames(H, W, B=3, seed=0):
    """uint8 [B, H, W, 3]: every second pixel (row-major) walks SPECIAL, starting at another entry per sample; the rest is random."""
    rs = np.random.RandomState(seed * 1000 + H * 7 + W)
    x = rs.randint(0, 256, (B, H * W, 3)).astype(np.uint8)
    for b in range(B):
        pos = np.arange(0, H * W, 2)
        x[b, pos] = SPECIAL[(pos // 2 + 5 * b) % len(SPECIAL)]
    return x.reshape(B, H, W, 3)


def thermal_frames(H, W, B=3, seed=0):
    """uint16 [B, H, W] sensor counts on both sides of the [20800, 27000] clamp"""
    rs = np.random.RandomState(seed * 1000 + H * 11 + W)
    return rs.randint(15000, 30000, (B, H, W)).astype(np.uint16)


def colour_refs(frames, table, S, dtype, mean=None, std=None):
    return np.stack([prepare_colour(frames[b], table[b], S, dtype, mean, std) for b in range(len(frames))])


# fp32 distance of the restatement on the GPU test's own inputs (every shape, table, modality and sample), measured on the CPU by
# fp32_distance(): 1.002e-6, in units of the normalised output (|values| <= 2.64).  The GPU test allows the kernel four times that, 4.0e-6,
# or the floor of the existing letterbox tests (rtol 1e-5, atol 2e-5 rgb / 2e-6 depth, thermal) where that is wider.
# tests/test_augment_cpu.py repeats the measurement and holds this figure to it.
MEASURED_FP32_DISTANCE = 1.01e-6


def fp32_distance():
    """The largest |hsv_ref float32 - hsv_ref float64| over every colour case of the GPU test (shapes x tables x {rgb, depth} x samples)."""
    worst = 0.0
    for H, W, S in SHAPES:
        for name, tab in TABLES.items():
            for seed, (mean, std) in enumerate(((I.IMAGENET_MEAN, I.IMAGENET_STD), (None, None))):
                fr = colour_frames(H, W, seed=seed)
                worst = max(worst, float(np.abs(colour_refs(fr, tab, S, np.float32, mean, std) -
                                                colour_refs(fr, tab, S, np.float64, mean, std)).max()))
    return worst
