"""GPU: the IoU-family box regression criteria of mmd_focal_loss_box (GIoU, DIoU, CIoU beside smooth-L1 in focal_loss_kernel's pass 1)
against the float64 restatement tests/box_loss_ref.py - loss and the full regression gradient - on seeded random scenes and on the edges of
the rule; against mmd_focal_loss for everything the modes share; the refusals; through DistillEngine (eager, captured, validation, the
default's launch) and train.py end to end.  Tolerance: tests/test_gpu_losses.py's for this kernel (loss rtol 2e-4, gradient within 2e-3 of
the reference's largest value)."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import box_loss_ref as R
from mm_distillnet_amd import _lib
from mm_distillnet_amd.step import BOX_LOSSES
from oracle import effdet_ref as O

call = _lib.call
DEV = "cuda"
S, B, NC = 128, 3, 20
F = np.float32


def anchors_cpu():
    a = O.anchors_for(S, 2)[0].float().contiguous()
    assert a.shape[0] == 3069 and a.shape[0] % 256 != 0      # the tail block runs
    return a


def scene(seed, nc=NC, nbox=(6, 5, 7)):
    """-> (cls [B,A,nc] probabilities, reg [B,A,4] ~ 0.4 N(0,1), annotations per image [n,5])"""
    gen = torch.Generator().manual_seed(seed)
    A = anchors_cpu().shape[0]
    cls = torch.sigmoid(torch.randn(B, A, nc, generator=gen) * 2 - 2)
    reg = torch.randn(B, A, 4, generator=gen) * 0.4
    ann = []
    for n in nbox:
        c = torch.rand(n, 2, generator=gen) * 90 + 19
        s = torch.rand(n, 2, generator=gen) * 60 + 8
        lab = torch.randint(0, nc, (n, 1), generator=gen).float()
        ann.append(torch.cat([c - 0.5 * s, c + 0.5 * s, lab], 1).numpy())
    return cls, reg, ann


def pack(ann, maxg, nbox_add=0):
    """annotations -> (boxes [B,maxg,5] with NaN behind each count: never read, nbox [B]); an image with more than maxg boxes keeps
    its true count (the kernel clamps it)"""
    boxes = torch.full((len(ann), maxg, 5), float("nan"))
    nbox = torch.zeros(len(ann), dtype=torch.int32)
    for i, a in enumerate(ann):
        a = np.asarray(a, dtype=F).reshape(-1, 5)
        k = min(len(a), maxg)
        boxes[i, :k] = torch.from_numpy(a[:k])
        nbox[i] = len(a) + nbox_add
    return boxes, nbox


def run(entry, cls, reg, ann, mode=None, weight=None, to_logit=0, gscale=1.0, maxg=16):
    """one call of `entry` on dirty workspaces and outputs -> (loss_out [2], dcls, dreg, any_boxes) on the host"""
    Bn, A, nc = cls.shape
    boxes, nbox = pack(ann, maxg)
    assign = torch.full((Bn * A,), -7777, dtype=torch.int32, device=DEV)
    npos = torch.full((Bn,), -7777, dtype=torch.int32, device=DEV)
    acc = torch.full((2 * Bn,), float("nan"), dtype=torch.float64, device=DEV)
    out = torch.full((2,), float("nan"), device=DEV)
    dcls = torch.full((Bn, A, nc), float("nan"), device=DEV)
    dreg = torch.full((Bn, A, 4), float("nan"), device=DEV)
    anyb = torch.zeros(1, dtype=torch.int32, device=DEV)
    extra = () if entry == "mmd_focal_loss" else (BOX_LOSSES[mode], float(weight))
    call(entry, cls.contiguous().to(DEV), reg.contiguous().to(DEV), anchors_cpu().to(DEV), boxes.to(DEV), nbox.to(DEV), maxg, Bn, A, nc,
         assign, npos, acc, out, dcls, dreg, gscale, to_logit, anyb, *extra)
    torch.cuda.synchronize()
    return out.cpu(), dcls.cpu(), dreg.cpu(), int(anyb.item())


def check(mode, out, dreg, reg, ann, weight=1.0, gscale=1.0, maxg=0, what=""):
    """loss rtol 2e-4, max |dreg - ref| <= 2e-3 max |ref| + 1e-9 against float64 -> the reference gradient"""
    ref_loss, ref_grad = R.box_loss_and_grad(mode, reg, anchors_cpu(), ann, weight, gscale, maxg)
    err = (dreg.double() - ref_grad).abs().max().item()
    top = ref_grad.abs().max().item()
    print(f"{what}{mode} w={weight} gs={gscale}: loss {out[0].item():.7g} ref {ref_loss:.7g} rel {abs(out[0].item() - ref_loss) / max(ref_loss, 1e-30):.2e}; "
          f"dreg err {err:.3e} of max {top:.3e} ({err / max(top, 1e-30):.2e})")
    assert torch.isfinite(dreg).all()
    np.testing.assert_allclose(out[0].item(), ref_loss, rtol=2e-4, atol=1e-9)
    assert err <= 2e-3 * top + 1e-9, (err, top)
    return ref_loss, ref_grad


# ---------------------------------------------------------------- against float64
@pytest.mark.parametrize("weight,gscale,to_logit", [(1.0, 1.0, 0), (2.5, 0.5, 1)])
@pytest.mark.parametrize("mode", R.MODES)
def test_against_float64(mode, weight, gscale, to_logit):
    cls, reg, ann = scene(11)
    out, dcls, dreg, anyb = run("mmd_focal_loss_box", cls, reg, ann, mode, weight, to_logit, gscale)
    ref_loss, ref_grad = check(mode, out, dreg, reg, ann, weight, gscale)
    assert anyb == 1 and ref_loss > 0
    npos = int((ref_grad != 0).any(-1).sum())
    assert npos >= 100, npos                                           # the scene has positives in every image
    assert (dreg[(ref_grad == 0).all(-1)] == 0).all()                  # and exact zeros everywhere else
    assert torch.isfinite(dcls).all()


@pytest.mark.parametrize("mode", R.MODES)
def test_three_classes_scalar_class_walk(mode):
    """NC = 3 (not a multiple of 4): pass 2 walks the classes one by one behind the new pass 1"""
    cls, reg, ann = scene(12, nc=3)
    out, dcls, dreg, _ = run("mmd_focal_loss_box", cls, reg, ann, mode, 1.0)
    check(mode, out, dreg, reg, ann)
    out0, dcls0, _, _ = run("mmd_focal_loss", cls, reg, ann)
    assert torch.equal(dcls, dcls0)
    np.testing.assert_allclose(out[1].item(), out0[1].item(), rtol=1e-6)


# ---------------------------------------------------------------- consistency with mmd_focal_loss
@pytest.mark.parametrize("to_logit,gscale", [(0, 1.0), (1, 0.5)])
def test_shared_parts_equal_focal_loss(to_logit, gscale):
    cls, reg, ann = scene(13)
    out0, dcls0, dreg0, any0 = run("mmd_focal_loss", cls, reg, ann, to_logit=to_logit, gscale=gscale)
    assert any0 == 1 and dcls0.abs().max() > 0 and dreg0.abs().max() > 0
    for mode, weight in (("smooth_l1", 1.0), ("giou", 1.0), ("diou", 2.5), ("ciou", 1.0)):
        out, dcls, dreg, anyb = run("mmd_focal_loss_box", cls, reg, ann, mode, weight, to_logit, gscale)
        assert torch.equal(dcls, dcls0), mode
        np.testing.assert_allclose(out[1].item(), out0[1].item(), rtol=1e-6)
        assert anyb == 1
        if mode == "smooth_l1":
            assert torch.equal(dreg, dreg0)
            np.testing.assert_allclose(out[0].item(), out0[0].item(), rtol=1e-6)
        else:
            assert not torch.equal(dreg, dreg0)
            assert torch.equal((dreg != 0).any(-1), (dreg0 != 0).any(-1))      # the same positives


# ---------------------------------------------------------------- edges
@pytest.mark.parametrize("mode", R.MODES)
def test_image_without_boxes_among_images_with_boxes(mode):
    cls, reg, ann = scene(14)
    ann[1] = np.zeros((0, 5), F)
    out, dcls, dreg, anyb = run("mmd_focal_loss_box", cls, reg, ann, mode, 2.5)
    check(mode, out, dreg, reg, ann, 2.5)
    assert anyb == 1 and (dreg[1] == 0).all() and (dreg[0] != 0).any() and (dreg[2] != 0).any()
    out0, dcls0, _, _ = run("mmd_focal_loss", cls, reg, ann)
    assert torch.equal(dcls, dcls0)


@pytest.mark.parametrize("mode", R.MODES)
def test_batch_without_boxes(mode):
    cls, reg, _ = scene(15)
    ann = [np.zeros((0, 5), F)] * B
    assert R.box_loss_and_grad(mode, reg, anchors_cpu(), ann)[0] == 0.0
    out, dcls, dreg, anyb = run("mmd_focal_loss_box", cls, reg, ann, mode, 2.5)
    assert out.tolist() == [0.0, 0.0] and (dcls == 0).all() and (dreg == 0).all() and anyb == 0


@pytest.mark.parametrize("mode", R.MODES)
def test_more_boxes_than_capacity_are_clamped(mode):
    cls, reg, ann = scene(16, nbox=(9, 3, 12))
    out, _, dreg, _ = run("mmd_focal_loss_box", cls, reg, ann, mode, 1.0, maxg=4)
    _, ref_grad = check(mode, out, dreg, reg, ann, maxg=4)
    _, ref_all = R.box_loss_and_grad(mode, reg, anchors_cpu(), ann)
    assert not torch.equal(ref_grad, ref_all)      # the clamp matters in this scene


def crafted(reg_of):
    """one 40 x 40 box per image on a 128^2 image; reg_of(anchor rows [n,4] float64, target (gcx, gcy, gw, gh)) -> reg [n,4] float64 for
    the box's positive anchors -> (cls, reg, ann, positives mask [B,A])"""
    cls, reg, _ = scene(17)
    ann = [np.array([[30, 40, 70, 80, 1]], F), np.array([[60.5, 20.25, 100.5, 61.75, 0]], F), np.array([[44, 44, 84, 84, 2]], F)]
    a = anchors_cpu()
    mask = torch.zeros(B, a.shape[0], dtype=torch.bool)
    for j in range(B):
        box = torch.from_numpy(ann[j])
        pos, _, _ = R.assign(a, box)
        assert int(pos.sum()) >= 4
        mask[j] = pos
        reg[j][pos] = reg_of(a[pos].double(), R.target_of(box.double())).float()
    return cls, reg, ann, mask


@pytest.mark.parametrize("mode", R.MODES)
def test_prediction_disjoint_from_target(mode):
    """centre offsets of +-6 anchor sizes: IoU is 0 for every positive, the penalty terms still pull"""
    gen = torch.Generator().manual_seed(2)

    def far(a, tgt):
        sign = (torch.randint(0, 2, (a.shape[0], 2), generator=gen) * 2 - 1).double()
        return torch.cat([6.0 * sign, torch.randn(a.shape[0], 2, generator=gen, dtype=torch.float64) * 0.2], 1)
    cls, reg, ann, mask = crafted(far)
    for j in range(B):
        r = reg[j][mask[j]].double()
        L = R.pair_loss("giou", *R.decode(r, anchors_cpu()[mask[j]].double()), *R.target_of(torch.from_numpy(ann[j]).double()))
        assert (L > 1.0).all()      # 1 - 0 + a positive penalty: disjoint
    out, _, dreg, _ = run("mmd_focal_loss_box", cls, reg, ann, mode, 1.0)
    _, ref_grad = check(mode, out, dreg, reg, ann)
    assert out[0].item() > 1.0
    assert (dreg[mask][:, :2] != 0).any(-1).all() and (ref_grad[mask][:, :2] != 0).any(-1).all()


@pytest.mark.parametrize("mode", R.MODES)
def test_prediction_contains_target(mode):
    def big(a, tgt):      # centred near the target, twice its size and more
        gcx, gcy, gw, gh = tgt
        ah, aw = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
        acy, acx = a[:, 0] + 0.5 * ah, a[:, 1] + 0.5 * aw
        return torch.stack([(gcy + 1.5 - acy) / ah, (gcx - 2.0 - acx) / aw, torch.log(2.2 * gh / ah), torch.log(2.6 * gw / aw)], 1)
    cls, reg, ann, mask = crafted(big)
    out, _, dreg, _ = run("mmd_focal_loss_box", cls, reg, ann, mode, 1.0)
    check(mode, out, dreg, reg, ann)
    assert (dreg[mask][:, 2:] > 0).all()      # shrinking the prediction lowers the loss


@pytest.mark.parametrize("mode", R.MODES)
def test_size_outputs_beyond_the_decode_clamp(mode):
    def huge(a, tgt):
        n = a.shape[0]
        return torch.cat([torch.full((n, 2), 0.1, dtype=torch.float64), torch.full((n, 1), R.LOG_MAX + 0.5, dtype=torch.float64),
                          torch.full((n, 1), 9.0, dtype=torch.float64)], 1)
    cls, reg, ann, mask = crafted(huge)
    out, _, dreg, _ = run("mmd_focal_loss_box", cls, reg, ann, mode, 1.0)
    check(mode, out, dreg, reg, ann)
    assert math.isfinite(out[0].item()) and (dreg[mask][:, 2:] == 0).all()
    # (the huge prediction contains its target: GIoU does not depend on its centre there, the centre-distance term of the others does)
    assert ((dreg[mask][:, :2] != 0).any(-1).all()) == (mode != "giou")


@pytest.mark.parametrize("mode", R.MODES)
def test_zero_width_pseudo_label(mode):
    """x2 == x1: such a box has IoU 0 with every anchor, so the assignment never makes it a positive's target; it must not disturb the
    image's other box, and an image that has nothing else adds 0 (the clamp on a positive's target: the next test)"""
    cls, reg, ann = scene(18)
    ann[0] = np.array([[50, 30, 50, 70, 1], [20, 60, 80, 110, 0]], F)
    ann[1] = np.array([[64, 40, 64, 41, 3]], F)      # no extent to speak of: no positive anchor, the image adds 0
    out, _, dreg, _ = run("mmd_focal_loss_box", cls, reg, ann, mode, 1.0)
    check(mode, out, dreg, reg, ann)
    assert (dreg[1] == 0).all() and (dreg[0] != 0).any()


@pytest.mark.parametrize("mode", R.MODES)
def test_thin_pseudo_label_under_the_pixel_clamp(mode):
    """the 1-pixel clamp on a positive's target: a box has to cover half an anchor to be one, so the anchors are a scaled-down grid whose
    smallest are 1.4 pixels wide, and the box is 0.9 wide"""
    a = (anchors_cpu() / 16.0).contiguous()
    box = np.array([[4.05, 2.9, 4.95, 5.5, 1]], F)
    pos, _, _ = R.assign(a, torch.from_numpy(box))
    assert int(pos.sum()) == 2
    cls, reg, _ = scene(19)
    reg = reg[:1].repeat(B, 1, 1)      # (the same image three times: the batch's loss is one image's)
    ann = [box, box, box]
    Bn, A, nc = cls.shape
    boxes, nbox = pack(ann, 4)
    out = torch.full((2,), float("nan"), device=DEV)
    dreg = torch.full((Bn, A, 4), float("nan"), device=DEV)
    call("mmd_focal_loss_box", cls.to(DEV), reg.to(DEV), a.to(DEV), boxes.to(DEV), nbox.to(DEV), 4, Bn, A, nc,
         torch.empty(Bn * A, dtype=torch.int32, device=DEV), torch.empty(Bn, dtype=torch.int32, device=DEV),
         torch.empty(2 * Bn, dtype=torch.float64, device=DEV), out, None, dreg, 1.0, 0, None, BOX_LOSSES[mode], 1.0)
    torch.cuda.synchronize()
    ref_loss, ref_grad = R.box_loss_and_grad(mode, reg, a, ann)
    unclamped = R.pair_loss(mode, *R.decode(reg[0].double()[pos], a[pos].double()),
                            *[t if i != 2 else torch.full_like(t, 0.9) for i, t in enumerate(R.target_of(torch.from_numpy(box).double()))])
    assert abs(unclamped.mean().item() - ref_loss) > 1e-3 * ref_loss      # the clamp changes this loss
    np.testing.assert_allclose(out[0].item(), ref_loss, rtol=2e-4)
    err = (dreg.cpu().double() - ref_grad).abs().max().item()
    assert err <= 2e-3 * ref_grad.abs().max().item() + 1e-9


@pytest.mark.parametrize("mode", R.MODES)
def test_prediction_equal_to_target(mode):
    """the decode inverted in float64: loss ~ 0 (fp32 rounding of reg), gradient finite (the max / min ties make it a subgradient choice)"""
    def exact(a, tgt):
        gcx, gcy, gw, gh = tgt
        ah, aw = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
        acy, acx = a[:, 0] + 0.5 * ah, a[:, 1] + 0.5 * aw
        return torch.stack([(gcy - acy) / ah, (gcx - acx) / aw, torch.log(gh / ah), torch.log(gw / aw)], 1)
    cls, reg, ann, mask = crafted(exact)
    out, _, dreg, _ = run("mmd_focal_loss_box", cls, reg, ann, mode, 1.0)
    print(mode, "loss at prediction == target", out[0].item())
    assert abs(out[0].item()) <= 1e-5
    assert torch.isfinite(dreg).all()


@pytest.mark.parametrize("mode", R.MODES)
def test_negative_and_ignored_anchors_have_zero_gradient(mode):
    cls, reg, ann = scene(20)
    a = anchors_cpu()
    out, _, dreg, _ = run("mmd_focal_loss_box", cls, reg, ann, mode, 1.0)
    n_ign = 0
    for j in range(B):
        pos, _, ign = R.assign(a, torch.from_numpy(ann[j]))
        n_ign += int(ign.sum())
        assert (dreg[j][~pos] == 0).all() and (dreg[j][pos] != 0).any(-1).all()
    assert n_ign > 0      # the ignore band is populated


# ---------------------------------------------------------------- refusals
def test_rejections_leave_outputs_alone():
    cls, reg, ann = scene(21)
    Bn, A, nc = cls.shape
    boxes, nbox = pack(ann, 16)
    dll = _lib.LIB.load()
    t = {k: v.to(DEV) for k, v in dict(cls=cls, reg=reg, anchors=anchors_cpu(), boxes=boxes, nbox=nbox).items()}
    assign = torch.full((Bn * A,), -7777, dtype=torch.int32, device=DEV)
    npos = torch.full((Bn,), -7777, dtype=torch.int32, device=DEV)
    acc = torch.full((2 * Bn,), 5.0, dtype=torch.float64, device=DEV)
    out = torch.full((2,), 7.0, device=DEV)
    dcls = torch.full((Bn, A, nc), 7.0, device=DEV)
    dreg = torch.full((Bn, A, 4), 7.0, device=DEV)
    anyb = torch.zeros(1, dtype=torch.int32, device=DEV)
    p = lambda x: x.data_ptr()      # noqa: E731
    for mode, weight in ((4, 1.0), (1, 0.0), (2, float("nan")), (0, 2.0), (-1, 1.0), (3, float("inf")), (3, -2.0)):
        rc = dll.mmd_focal_loss_box(p(t["cls"]), p(t["reg"]), p(t["anchors"]), p(t["boxes"]), p(t["nbox"]), 16, Bn, A, nc, p(assign), p(npos),
                                    p(acc), p(out), p(dcls), p(dreg), 1.0, 0, p(anyb), mode, weight, _lib.stream_ptr())
        assert rc == -22, (mode, weight)
        with pytest.raises(RuntimeError, match="mmd_focal_loss_box failed with status -22"):
            call("mmd_focal_loss_box", t["cls"], t["reg"], t["anchors"], t["boxes"], t["nbox"], 16, Bn, A, nc, assign, npos, acc, out, dcls, dreg,
                 1.0, 0, anyb, mode, weight)
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (dcls == 7.0).all() and (dreg == 7.0).all() and (acc == 5.0).all()
    assert (assign == -7777).all() and (npos == -7777).all() and anyb.item() == 0


# ---------------------------------------------------------------- the PyTorch facade
def test_facade_criterion():
    from mm_distillnet_amd.model import YetAnotherFocalLoss
    cls, reg, ann = scene(22)
    anchors = anchors_cpu().to(DEV)[None]
    r = reg.to(DEV).requires_grad_(True)
    crit = YetAnotherFocalLoss(box_loss="ciou", box_weight=2.5)
    lr, lc = crit((cls.to(DEV), r, anchors), ann)
    (lr.sum() * 0.5).backward()
    ref_loss, ref_grad = R.box_loss_and_grad("ciou", reg, anchors_cpu(), ann, 2.5, 0.5)
    np.testing.assert_allclose(lr.item(), ref_loss, rtol=2e-4)
    assert (r.grad.cpu().double() - ref_grad).abs().max().item() <= 2e-3 * ref_grad.abs().max().item() + 1e-9
    l0, c0 = YetAnotherFocalLoss()((cls.to(DEV), reg.to(DEV), anchors), ann)
    out0, _, _, _ = run("mmd_focal_loss", cls, reg, ann, maxg=max(len(a) for a in ann))
    np.testing.assert_allclose(l0.item(), out0[0].item(), rtol=1e-6)      # the default: mmd_focal_loss's smooth-L1
    np.testing.assert_allclose(lc.item(), c0.item(), rtol=1e-6)


# ---------------------------------------------------------------- through the engine
OBJECTS = {0: [((10, 12, 50, 54), 1), ((60, 8, 110, 60), 0), ((20, 70, 70, 120), 1)], 1: [((64, 60, 120, 118), 0), ((5, 5, 50, 50), 1)]}


def engine(**kw):
    from mm_distillnet_amd.step import DistillEngine, StepConfig
    from helpers import make_state
    from test_gpu_step import MODS, teacher_states
    teachers = teacher_states(2, MODS)
    spec_s, st_s = make_state(2, 8, 24, "audio")
    e = DistillEngine(spec_s, {k: v[0] for k, v in teachers.items()}, DEV, StepConfig(image_size=S, **kw))
    e.load(st_s, {k: v[1] for k, v in teachers.items()})
    return e


def injected(eng):
    """the same objects from all three teachers -> the engine's teacher_labels"""
    per = [[np.array([list(box) + [0.9 - 0.1 * t, lb] for box, lb in OBJECTS[b]], F).reshape(-1, 6) for b in (0, 1)] for t in range(3)]
    return eng.labels_from_rows(per, eng.student.anchors(S).shape[0])


def reference_of(eng, out, mode, weight=1.0):
    nb = out["nbox"].cpu().tolist()
    ann = [out["boxes"][i, :nb[i]].cpu().numpy() for i in range(len(nb))]
    reg = out["reg_s"].detach().cpu().reshape(len(nb), -1, 4)
    assert sum(nb) > 0
    return R.box_loss(mode, reg, eng.student.anchors(S).cpu(), ann, weight).item()


def engine_batch():
    from mm_distillnet_amd.synth import synth_inputs
    return {k: v.to(DEV) for k, v in synth_inputs(2, S, seed=5).items()}


def test_engine_eager_step_and_validation():
    eng = engine(box_loss="giou")
    batch = engine_batch()
    ds = eng.make_drop_scale(2, torch.Generator(device=DEV).manual_seed(1))
    out = eng.step_body(batch, ds, teacher_labels=injected(eng))
    torch.cuda.synchronize()
    eng.check_overflow()
    ref = reference_of(eng, out, "giou")
    print("engine giou: reg", out["reg"].item(), "ref", ref)
    assert ref > 0 and torch.isfinite(eng.student.ps.grad).all() and eng.student.ps.grad.abs().max() > 0
    np.testing.assert_allclose(out["reg"].item(), ref, rtol=2e-4)
    # train=False validation: the same criterion on the eval-mode student
    reg_v, cls_v, _ = eng.eval_losses(batch, teacher_labels=injected(eng))
    ref_v = reference_of(eng, eng.out, "giou")
    np.testing.assert_allclose(reg_v, ref_v, rtol=2e-4)
    assert np.isfinite(cls_v)
    # and it is not smooth-L1's number
    eng0 = engine()
    reg0, _, _ = eng0.eval_losses(batch, teacher_labels=injected(eng0))
    assert abs(reg0 - reg_v) > 1e-3 * abs(reg_v)


def test_engine_graph_replay_matches_eager():
    """test_gpu_step.py::test_graph_replay_matches_eager with box_loss = giou and a weight: same labels and losses, gradients equal up to
    the run-to-run noise of the backward's fp32 atomics"""
    batch = engine_batch()
    eng_a, eng_b = engine(box_loss="giou", box_weight=2.5), engine(box_loss="giou", box_weight=2.5)
    ds = eng_a.make_drop_scale(2, torch.Generator(device=DEV).manual_seed(1))
    eng_b.capture(batch, teacher_labels=injected(eng_b))
    oa = eng_a.step_body(batch, ds, teacher_labels=injected(eng_a))
    eng_b.set_drop_scale(ds)
    eng_b.g_main.replay()
    torch.cuda.synchronize()
    ob = eng_b.out
    assert oa["nbox"].tolist() == ob["nbox"].tolist() and sum(oa["nbox"].tolist()) > 0
    for k in ("reg", "cls", "kd"):
        np.testing.assert_allclose(oa[k].cpu().numpy(), ob[k].cpu().numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(ob["reg"].item(), reference_of(eng_b, ob, "giou", 2.5), rtol=2e-4)
    ga, gb = eng_a.student.ps.grad, eng_b.student.ps.grad
    assert torch.isfinite(gb).all()
    assert (ga - gb).abs().max().item() <= 2e-3 * ga.abs().max().item()
    eng_a.optimizer_body(); eng_b.g_opt.replay()
    torch.cuda.synchronize()
    assert eng_a.adam_main[0].item() == eng_b.adam_main[0].item() == 1.0
    assert eng_b.head_active.item() == 1


def test_engine_default_issues_focal_loss_only(monkeypatch):
    from mm_distillnet_amd import step
    names = []

    def recording(name, *args):
        names.append(name)
        return _lib.call(name, *args)
    monkeypatch.setattr(step, "call", recording)
    batch = engine_batch()
    eng = engine()
    ds = eng.make_drop_scale(2, torch.Generator(device=DEV).manual_seed(1))
    eng.step_body(batch, ds, teacher_labels=injected(eng))
    eng.eval_losses(batch, teacher_labels=injected(eng))
    torch.cuda.synchronize()
    assert names.count("mmd_focal_loss") == 2 and "mmd_focal_loss_box" not in names
    names.clear()
    eng = engine(box_loss="diou")
    eng.step_body(batch, ds, teacher_labels=injected(eng))
    torch.cuda.synchronize()
    assert names.count("mmd_focal_loss_box") == 1 and "mmd_focal_loss" not in names


# ---------------------------------------------------------------- train.py end to end
def test_train_main_box_loss(tmp_path, monkeypatch):
    """train.py --overwrite '{"box_loss": "ciou"}' end to end beside the default: both finish with finite losses, the regression scalars
    differ"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.chdir(tmp_path)
    sys.path.insert(0, root)
    import train
    cfgf = os.path.join(root, "configs", "mm-distillnet.cfg")
    reg = {}
    for name, extra in (("ciou", ', "box_loss": "ciou"'), ("l1", "")):
        ov = ('{"image_size": 128, "batch_size": 2, "synthetic_length": 8, "num_epoches": 1, "exp_name": "exp_%s", "resume": "False", '
              '"num_workers": 0, "no_validation": "True", "synthetic_cls_bias": -1.0%s}' % (name, extra))
        # (synthetic_cls_bias: the stand-in teachers emit pseudo-labels; at the default they emit none and both losses would be 0)
        loss = train.main(["--config_file", cfgf, "--overwrite", ov, "--max_steps", "3"])
        assert np.isfinite(loss)
        logs = json.load(open(tmp_path / f"exp_{name}" / "all_logs.0.json"))
        reg[name] = [v for _, _, v in logs[f"exp_{name}/Train_/Regression_loss"]]
    print("Train_/Regression_loss", reg)
    assert reg["ciou"] and len(reg["ciou"]) == len(reg["l1"]) and all(np.isfinite(v) for v in reg["ciou"] + reg["l1"])
    assert any(v != 0.0 for v in reg["ciou"]) and all(a != b for a, b in zip(reg["ciou"], reg["l1"]) if a != 0.0 or b != 0.0)
