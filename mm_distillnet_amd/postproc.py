"""Detections from a net's head outputs on the device: decode, clip, threshold, class filter and NMS (csrc/postproc.hip), shared by the
distillation step's pseudo-labels (`DistillEngine._pseudo_labels`) and the audio-only detector (`detector.AudioDetector`), and the weighted
box fusion of several sources' detections (`wbf_merge`: the step's cfg `label_merge = wbf`, or saved teacher detections).

  EfficientDet_post_processing / logits_to_ground_truth   src/utils/utils.py:144-324
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib

call = _lib.call


def valid_class_mask(prediction_ids) -> int:
    """bit i set = prediction id i passes the class filter (src/utils/utils.py:285-323)"""
    mask = 0
    for i in prediction_ids:
        mask |= 1 << int(i)
    return mask


def nms_workspace(ws, B: int, nmax: int):
    """the chunked exact-greedy NMS path's workspace for lists of up to nmax rows per image (None: not needed)"""
    n = int(_lib.LIB.load().mmd_nms_ws_floats(nmax))
    return ws.alloc((B * n,)) if n else None


def decode_nms(ws, net, cls, reg, B: int, A: int, S: int, cap: int, conf_threshold: float, valid_mask: int, label_map: torch.Tensor,
               nms_threshold: float, inclusive: bool, overflow: torch.Tensor):
    """cls [B,A,NC] / reg [B,A,4] of `net` at image size S -> (rows [B,cap,6] (x1, y1, x2, y2, score, label), count [B]) in the bump
    arena `ws`; a list longer than cap rows sets the sticky `overflow` flag."""
    nc = net.spec.num_classes
    score = ws.alloc((B * A,)); clsid = ws.alloc((B * A,), torch.uint8); flags = ws.alloc((B * A,), torch.uint8)
    over = ws.alloc((B, cap)); cand = ws.alloc((B, cap, 6))
    n_over = ws.alloc((B,), torch.int32); n_keep = ws.alloc((B,), torch.int32)
    call("mmd_decode_filter", cls, reg, net.anchors(S), B, A, nc, float(conf_threshold), valid_mask, float(S),
         score, clsid, flags, over, cand, n_over, n_keep, overflow, cap)
    rows = ws.alloc((B, cap, 6)); cnt = ws.alloc((B,), torch.int32)
    mask_ws = ws.alloc((B * 1024 * 16,), torch.int64)      # per net: the step's teachers run concurrently
    call("mmd_nms_teacher", cand, n_keep, over, label_map, float(nms_threshold),
         1 if inclusive else 0, float(S), B, rows, cnt, mask_ws, overflow, cap, nms_workspace(ws, B, cap))
    return rows, cnt


LABEL_MERGES = ("nms", "wbf")


def wbf_merge(ws, rows_list, cnt_list, B: int, cap: int, iou: float, inclusive: bool, max_boxes: int, min_votes: int,
              overflow: torch.Tensor, merge01: bool = False):
    """Weighted box fusion of 1..4 sources' detections (csrc/postproc.hip pp_wbf_kernel; the rule: include/mmdistill.h mmd_wbf_merge_n):
    rows_list[s] [B, cap, 6] (x1, y1, x2, y2, score, label) with cnt_list[s] [B] int32, e.g. what `decode_nms` returns per teacher or
    saved teacher detections -> (boxes [B, max_boxes, 5] (fused x1, y1, x2, y2, label), nbox [B], aux [B, max_boxes, 3] (mean member
    score, members, distinct sources)) in the bump arena `ws`.  Only clusters that at least min_votes sources contributed to come out;
    more than max_boxes of them, or more than 1024 rows in one image, set the sticky `overflow` flag."""
    ns = len(rows_list)
    if not 1 <= ns <= 4 or len(cnt_list) != ns:
        raise ValueError(f"wbf_merge: 1 to 4 sources with one count array each, got {ns} and {len(cnt_list)}")
    if not 1 <= int(min_votes) <= ns:
        raise ValueError(f"wbf_merge: min_votes {min_votes!r} is not between 1 and the {ns} sources")
    G = int(max_boxes)
    boxes = ws.alloc((B, G, 5)); nbox = ws.alloc((B,), torch.int32); aux = ws.alloc((B, G, 3))
    vp = ctypes.c_void_p
    srcs = (vp * ns)(*[_lib._ptr(t) for t in rows_list]); cnts = (vp * ns)(*[_lib._ptr(t) for t in cnt_list])
    call("mmd_wbf_merge_n", srcs, cnts, ns, float(iou), 1 if inclusive else 0, B, boxes, nbox, G, aux, int(min_votes), overflow,
         1 if merge01 else 0, cap)
    return boxes, nbox, aux
