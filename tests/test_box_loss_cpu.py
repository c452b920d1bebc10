"""CPU: properties of the float64 restatement of the IoU-family box losses (tests/box_loss_ref.py), and the host side of cfg `box_loss` /
`box_loss_weight`: StepConfig's checks, train.py's keys, the facade's arguments, the header's declaration of mmd_focal_loss_box."""
import ctypes
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

import box_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "mm-distillnet.cfg")
D = torch.float64


def t(*v):
    return torch.tensor(v, dtype=D)


def loss(mode, p, g):
    """p, g: (cx, cy, w, h)"""
    return R.pair_loss(mode, *[t(x) for x in p], *[t(x) for x in g]).item()


@pytest.mark.parametrize("mode", R.MODES)
def test_identical_boxes_give_zero(mode):
    for box in ((10.0, 20.0, 8.0, 4.0), (100.5, 7.25, 1.0, 300.0)):
        assert abs(loss(mode, box, box)) <= 1e-8      # (the 1e-7 in the denominators)


def test_giou_range_and_limits():
    gen = torch.Generator().manual_seed(0)
    n = 4000
    c = torch.rand(4, n, generator=gen, dtype=D) * 200
    s = torch.rand(4, n, generator=gen, dtype=D) * 100 + 0.5
    L = R.pair_loss("giou", c[0], c[1], s[0], s[1], c[2], c[3], s[2], s[3])
    assert L.min().item() >= 0.0 and L.max().item() <= 2.0
    # far apart: the loss approaches 2; touching equal squares: IoU 0 and an enclosing box of twice the area: 1 + 0 = 1
    assert 1.99 < loss("giou", (0, 0, 1, 1), (1e4, 1e4, 1, 1)) <= 2.0
    assert loss("giou", (0, 0, 2, 2), (2, 0, 2, 2)) == pytest.approx(1.0, abs=1e-6)
    # half-overlapping equal squares by hand: I = 2, U = 6, C = 6 -> 1 - 1/3 + 0
    assert loss("giou", (0, 0, 2, 2), (1, 0, 2, 2)) == pytest.approx(2.0 / 3.0, abs=1e-6)


def test_diou_grows_with_centre_distance_of_disjoint_boxes():
    vals = [loss("diou", (0, 0, 4, 4), (d, 0.5 * d, 4, 4)) for d in (5.0, 8.0, 20.0, 100.0, 1000.0)]
    assert all(b > a for a, b in zip(vals, vals[1:])) and vals[0] > 1.0 and vals[-1] < 2.0
    # by hand: centres (0,0) and (6,0), 4 x 4 boxes: IoU 0, rho^2 = 36, enclosing 10 x 4 -> 1 + 36 / 116
    assert loss("diou", (0, 0, 4, 4), (6, 0, 4, 4)) == pytest.approx(1.0 + 36.0 / 116.0, abs=1e-6)


def test_ciou_equals_diou_for_equal_aspect_ratios_and_exceeds_it_otherwise():
    for p, g in (((3, 4, 6, 2), (5, 5, 12, 4)), ((0, 0, 5, 5), (40, 3, 1, 1))):
        assert loss("ciou", p, g) == pytest.approx(loss("diou", p, g), abs=1e-12)
    p, g = (3, 4, 6, 2), (5, 5, 4, 12)
    v = 4 / math.pi ** 2 * (math.atan(4 / 12) - math.atan(6 / 2)) ** 2
    d = loss("diou", p, g)
    iou = 1.0 - (d - (4 + 1) / (7.0 ** 2 + 12.0 ** 2 + 1e-7))      # enclosing box: x 0 .. 7, y -1 .. 11
    assert loss("ciou", p, g) == pytest.approx(d + v * v / (1 - iou + v + 1e-7), abs=1e-9)


def _anchors_and_boxes(seed, n):
    gen = torch.Generator().manual_seed(seed)
    ctr = torch.rand(n, 2, generator=gen, dtype=D) * 100 + 20
    half = torch.rand(n, 2, generator=gen, dtype=D) * 20 + 4
    anchors = torch.cat([ctr - half, ctr + half], 1)                          # y1, x1, y2, x2
    gc = ctr.flip(1) + (torch.rand(n, 2, generator=gen, dtype=D) - 0.5) * 30      # x, y
    gs = torch.rand(n, 2, generator=gen, dtype=D) * 40 + 3
    boxes = torch.cat([gc - 0.5 * gs, gc + 0.5 * gs], 1)                      # x1, y1, x2, y2
    reg = torch.randn(n, 4, generator=gen, dtype=D) * 0.4
    return anchors, boxes, reg


@pytest.mark.parametrize("mode", R.MODES)
def test_gradcheck_on_untied_inputs(mode):
    anchors, boxes, reg = _anchors_and_boxes(3, 24)
    tgt = R.target_of(boxes)
    alpha = None
    if mode == "ciou":      # the gradient holds alpha constant: so does the finite difference, at alpha's value in the unperturbed point
        dec = R.decode(reg, anchors)
        v = (4.0 / math.pi ** 2) * (torch.atan(tgt[2] / tgt[3]) - torch.atan(dec[2] / dec[3])) ** 2
        alpha = (R.pair_loss("ciou", *dec, *tgt) - R.pair_loss("diou", *dec, *tgt)) / v      # = ciou_alpha at this point
        assert (alpha > 0).all() and (alpha < 1).all()

    def f(r):
        return R.pair_loss(mode, *R.decode(r, anchors), *tgt, alpha=alpha)
    assert torch.autograd.gradcheck(f, (reg.clone().requires_grad_(True),), eps=1e-6, atol=1e-6, rtol=1e-5)


def test_decode_clamp_has_zero_gradient_and_degenerate_target_is_a_pixel():
    anchors, boxes, reg = _anchors_and_boxes(4, 6)
    reg[:, 2:] = R.LOG_MAX + 0.5
    r = reg.clone().requires_grad_(True)
    L = R.pair_loss("ciou", *R.decode(r, anchors), *R.target_of(boxes))
    L.sum().backward()
    assert torch.isfinite(L).all() and (r.grad[:, 2:] == 0).all() and (r.grad[:, :2] != 0).any()
    gcx, gcy, gw, gh = R.target_of(t([5.0, 7.0, 5.0, 9.0]))      # zero width
    assert (gcx.item(), gcy.item(), gw.item(), gh.item()) == (5.0, 8.0, 1.0, 2.0)


def test_reduction_over_images():
    """an image without boxes or without positives adds 0 and still counts in the mean; the weight scales; no box at all -> 0"""
    from oracle import effdet_ref as O
    anchors = O.anchors_for(128, 2)[0]
    gen = torch.Generator().manual_seed(1)
    reg = torch.randn(3, anchors.shape[0], 4, generator=gen) * 0.4
    ann = [np.array([[20, 30, 70, 90, 1], [60, 10, 120, 60, 0]], np.float32), np.zeros((0, 5), np.float32),
           np.array([[10, 10, 11.5, 11.5, 2]], np.float32)]      # (no anchor reaches IoU 0.5 with a 1.5-pixel box)
    one = R.box_loss("giou", reg[:1], anchors, ann[:1]).item()
    assert one > 0
    assert R.box_loss("giou", reg, anchors, ann).item() == pytest.approx(one / 3, rel=1e-12)
    assert R.box_loss("giou", reg, anchors, ann, box_weight=2.5).item() == pytest.approx(2.5 * one / 3, rel=1e-12)
    val, grad = R.box_loss_and_grad("giou", reg, anchors, [ann[1]] * 3)
    assert val == 0.0 and (grad == 0).all()
    val, grad = R.box_loss_and_grad("diou", reg, anchors, ann, grad_scale=0.5)
    assert (grad[1:] == 0).all() and (grad[0] != 0).any()


# ---------------------------------------------------------------- cfg keys, StepConfig, facade, header
def test_step_config_box_loss():
    from mm_distillnet_amd.step import BOX_LOSSES, StepConfig
    sc = StepConfig()
    assert sc.box_loss == "smooth_l1" and sc.box_weight == 1.0
    assert BOX_LOSSES == {"smooth_l1": 0, "giou": 1, "diou": 2, "ciou": 3}
    for name in ("giou", "diou", "ciou"):
        sc = StepConfig(box_loss=name, box_weight=2.5)
        assert sc.box_loss == name and sc.box_weight == 2.5
    for bad in ("iou", "GIoU", "", None, 1):
        with pytest.raises(ValueError, match="box_loss"):
            StepConfig(box_loss=bad)
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), "2", None, True):
        with pytest.raises(ValueError, match="box_weight"):
            StepConfig(box_loss="giou", box_weight=bad)
    with pytest.raises(ValueError, match="box_weight"):
        StepConfig(box_weight=2.0)
    with pytest.raises(ValueError, match="box_weight"):
        StepConfig(box_loss="smooth_l1", box_weight=0.5)


def test_train_cfg_keys():
    sys.path.insert(0, ROOT)
    import train
    cfg, _ = train.parse_config(["--config_file", CFG])
    sc = train.step_config(cfg)
    assert (sc.box_loss, sc.box_weight) == ("smooth_l1", 1.0)
    assert train.TR.box_loss_settings(cfg) == {"box_loss": "smooth_l1", "box_weight": 1.0}
    cfg, _ = train.parse_config(["--config_file", CFG, "--overwrite", '{"box_loss": "giou", "box_loss_weight": 2}'])
    sc = train.step_config(cfg)
    assert (sc.box_loss, sc.box_weight) == ("giou", 2.0)
    assert "box_loss" in train.__doc__ and "box_loss_weight" in train.__doc__


def test_unknown_name_is_refused_before_any_device_work(monkeypatch):
    """trainer.box_loss_settings and the facade raise on the host: no entry point is called"""
    sys.path.insert(0, ROOT)
    import train
    from mm_distillnet_amd import _lib, model, step
    called = []
    for mod in (_lib, model, step):
        monkeypatch.setattr(mod, "call", lambda name, *a: called.append(name))
    for ov in ({"box_loss": "iou"}, {"box_loss": "giou", "box_loss_weight": 0}, {"box_loss": "ciou", "box_loss_weight": "nan"},
               {"box_loss_weight": 2}):
        cfg, _ = train.parse_config(["--config_file", CFG, "--overwrite", json.dumps(ov)])
        with pytest.raises(ValueError, match="box_loss|box_weight"):
            train.TR.box_loss_settings(cfg)
        with pytest.raises(ValueError, match="box_loss|box_weight"):
            train.step_config(cfg)
        with pytest.raises(ValueError, match="box_loss|box_weight"):
            model.extract_criterions_from_config(cfg)
    with pytest.raises(ValueError, match="box_loss"):
        model.YetAnotherFocalLoss(box_loss="iou")
    crit = model.YetAnotherFocalLoss()
    assert (crit.box_loss, crit.box_weight) == ("smooth_l1", 1.0)
    cfg, _ = train.parse_config(["--config_file", CFG, "--overwrite", '{"box_loss": "diou", "box_loss_weight": 0.5}'])
    crit = model.extract_criterions_from_config(cfg)[0]
    assert (crit.box_loss, crit.box_weight) == ("diou", 0.5)
    assert not called


def test_header_declares_focal_loss_box():
    from mm_distillnet_amd import _lib
    sigs = _lib.parse_header()
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    base = [P, P, P, P, P, I, I, I, I, P, P, P, P, P, P, F, I, P]
    assert sigs["mmd_focal_loss"] == base + [P]                       # unchanged: existing callers pass it positionally
    assert sigs["mmd_focal_loss_box"] == base + [I, F, P]             # + box_mode, box_weight, then the stream
    text = open(_lib.HEADER).read()
    lines = text[:text.index("int mmd_focal_loss_box(")].rstrip("\n").split("\n")
    out = []
    while lines and lines[-1].startswith("//"):
        out.append(lines.pop()[2:].strip())
    c = " ".join(reversed(out))
    for piece in ("GIoU", "DIoU", "CIoU", "box_weight", "MMD_EINVAL, nothing is launched", "need no zeroing", "sticky", "clamped",
                  "log(1000/16)", "IoU = I / (U + 1e-7)", "(cw*ch - U) / (cw*ch + 1e-7)", "(cw^2 + ch^2 + 1e-7)",
                  "alpha = v / (1 - IoU + v + 1e-7)", "a constant in the gradient", "max(x2 - x1, 1)"):
        assert piece in c, piece


def test_focal_loss_box_rejects_bad_arguments_without_gpu():
    from mm_distillnet_amd import _lib
    dll = _lib.LIB.load()

    def rc(mode, weight, cls=8):
        p = 8          # never dereferenced: validation comes before any launch
        return dll.mmd_focal_loss_box(cls, p, p, p, p, 4, 2, 256, 20, p, p, p, p, None, None, 1.0, 0, None, mode, weight, None)
    for mode, weight in ((4, 1.0), (-1, 1.0), (1, 0.0), (2, -1.0), (3, float("nan")), (1, float("inf")), (0, 2.0)):
        assert rc(mode, weight) == -22, (mode, weight)
    assert rc(1, 1.0, cls=None) == -22
