"""Float64 restatement of the IoU-family box regression losses of mmd_focal_loss_box (test infrastructure only).

Written from the papers: GIoU - Rezatofighi et al., "Generalized Intersection over Union", CVPR 2019; DIoU / CIoU - Zheng et al.,
"Distance-IoU Loss", AAAI 2020.  The predicted box is BBoxTransform's decode of the regression output on its anchor, the target the
assigned pseudo-label with the 1-pixel clamp of the smooth-L1 targets.  Differentiable torch ops, so autograd yields the gradient; the
anchor assignment is the oracle's (oracle/losses_ref.py calc_iou, first maximum, 0.5 / 0.4), evaluated in the inputs' fp32 as the kernel
evaluates it.
"""
from __future__ import annotations

import math
from typing import List

import numpy as np
import torch

from oracle.losses_ref import calc_iou

MODES = ("giou", "diou", "ciou")
EPS = 1e-7
LOG_MAX = math.log(1000.0 / 16.0)      # BBoxTransform's clamp on dh / dw


def decode(reg: torch.Tensor, anchors: torch.Tensor):
    """reg [N,4] (dy, dx, dh, dw) on anchors [N,4] (y1, x1, y2, x2) -> centre / size (pcx, pcy, pw, ph)"""
    ah = anchors[:, 2] - anchors[:, 0]
    aw = anchors[:, 3] - anchors[:, 1]
    acy = anchors[:, 0] + 0.5 * ah
    acx = anchors[:, 1] + 0.5 * aw
    pcy = reg[:, 0] * ah + acy
    pcx = reg[:, 1] * aw + acx
    ph = torch.exp(torch.clamp(reg[:, 2], max=LOG_MAX)) * ah
    pw = torch.exp(torch.clamp(reg[:, 3], max=LOG_MAX)) * aw
    return pcx, pcy, pw, ph


def target_of(box: torch.Tensor):
    """box [N,4+] (x1, y1, x2, y2) -> (gcx, gcy, gw, gh): the raw centre, extents clamped to one pixel"""
    gw = box[:, 2] - box[:, 0]
    gh = box[:, 3] - box[:, 1]
    gcx = box[:, 0] + 0.5 * gw
    gcy = box[:, 1] + 0.5 * gh
    return gcx, gcy, torch.clamp(gw, min=1.0), torch.clamp(gh, min=1.0)


def ciou_alpha(iou: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    return (v / (1.0 - iou + v + EPS)).detach()      # a constant in the gradient


def pair_loss(mode: str, pcx, pcy, pw, ph, gcx, gcy, gw, gh, alpha=None) -> torch.Tensor:
    """loss per pair of boxes given as centre / size.  alpha (ciou): the trade-off weight held at a given value, for a finite-difference
    check of the gradient, which treats it as a constant; None: ciou_alpha of these boxes"""
    if mode not in MODES:
        raise ValueError(mode)
    px1, px2, py1, py2 = pcx - 0.5 * pw, pcx + 0.5 * pw, pcy - 0.5 * ph, pcy + 0.5 * ph
    gx1, gx2, gy1, gy2 = gcx - 0.5 * gw, gcx + 0.5 * gw, gcy - 0.5 * gh, gcy + 0.5 * gh
    iw = torch.clamp(torch.minimum(px2, gx2) - torch.maximum(px1, gx1), min=0.0)
    ih = torch.clamp(torch.minimum(py2, gy2) - torch.maximum(py1, gy1), min=0.0)
    inter = iw * ih
    union = pw * ph + gw * gh - inter
    iou = inter / (union + EPS)
    cw = torch.maximum(px2, gx2) - torch.minimum(px1, gx1)
    ch = torch.maximum(py2, gy2) - torch.minimum(py1, gy1)
    if mode == "giou":
        return 1.0 - iou + (cw * ch - union) / (cw * ch + EPS)
    loss = 1.0 - iou + ((pcx - gcx) ** 2 + (pcy - gcy) ** 2) / (cw ** 2 + ch ** 2 + EPS)
    if mode == "ciou":
        v = (4.0 / math.pi ** 2) * (torch.atan(gw / gh) - torch.atan(pw / ph)) ** 2
        loss = loss + (ciou_alpha(iou, v) if alpha is None else alpha) * v
    return loss


def assign(anchors: torch.Tensor, box: torch.Tensor):
    """the oracle's rule -> (positive mask [A], box index [A], ignore mask [A])"""
    iou = calc_iou(anchors, box[:, :4])
    iou_max, iou_arg = torch.max(iou, dim=1)
    return iou_max >= 0.5, iou_arg, (iou_max >= 0.4) & (iou_max < 0.5)


def box_loss(mode: str, reg: torch.Tensor, anchors: torch.Tensor, annotations: List[np.ndarray], box_weight: float = 1.0,
             maxg: int = 0) -> torch.Tensor:
    """reg [B,A,4] (any float dtype; computed in float64), anchors [A,4] fp32, annotations: per image [n,5] (x1,y1,x2,y2,label); maxg > 0
    keeps the first maxg boxes of an image -> loss [1] = mean over the B images of box_weight * sum_pos L / npos (0 for an image
    without boxes or without positive anchors; 0 for a batch without boxes)."""
    B = reg.shape[0]
    anchors = anchors.float()
    a64 = anchors.double()
    per_image = []
    for j in range(B):
        ann = annotations[j]
        box = torch.from_numpy(np.asarray(ann, dtype=np.float32).reshape(-1, 5)) if np.size(ann) else torch.zeros(0, 5)
        if maxg > 0:
            box = box[:maxg]
        zero = reg[j].double().sum() * 0.0
        if box.shape[0] == 0:
            per_image.append(zero)
            continue
        pos, arg, _ = assign(anchors, box)
        if int(pos.sum()) == 0:
            per_image.append(zero)
            continue
        r = reg[j].double()[pos]
        loss = pair_loss(mode, *decode(r, a64[pos]), *target_of(box[arg[pos]].double()))
        per_image.append(float(box_weight) * loss.sum() / float(pos.sum()))
    return torch.stack(per_image).mean(dim=0, keepdim=True)


def box_loss_and_grad(mode, reg, anchors, annotations, box_weight=1.0, grad_scale=1.0, maxg=0):
    """-> (loss float, grad_scale * d loss / d reg as float64 [B,A,4])"""
    r = reg.detach().double().clone().requires_grad_(True)
    loss = box_loss(mode, r, anchors, annotations, box_weight, maxg)
    (loss.sum() * grad_scale).backward()
    return float(loss.item()), r.grad
