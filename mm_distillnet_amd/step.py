"""One distillation step of MM-DistillNet on the HIP engine, capturable as a single hipGraph.

Mirrors the reference's per-step path:
  ModelWithNMSLoss(.Augmented).forward  src/optimization/train_methods.py:310-422 / 436-517
  (ModelWithNMSKDListLoss for kd_mode="list": :84-162)
  loss mixing + backward + step         src/optimization/traditional.py:171-190
with every per-image host loop and `.cpu()` sync replaced by device kernels: teachers' pseudo-labels
(decode, class filter, NMS), the cross-teacher merge + NMS, the focal/smooth-L1 and MTA losses with
their gradients, the student backward, gradient all-reduce (RCCL, student gradients only) and Adam.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import numbers
import os

from dataclasses import dataclass
from typing import Any, Dict, List, NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from .arch import NetSpec, make_spec
from .engine import Net, Feat, NONE, SWISH, pack_nets
from .postproc import LABEL_MERGES, decode_nms, nms_workspace, valid_class_mask, wbf_merge
from .store import Arena

call = _lib.call
TEACHER_ORDER = ("rgb", "depth", "thermal")     # ModuleDict insertion order in train.py:123-135
OPT_MODES = {"Adam": 0, "AdamW": 1, "SGD": 2}
KD_LOSSES = ("MTALoss", "AttentionLoss", "None")
BOX_LOSSES = {"smooth_l1": 0, "giou": 1, "diou": 2, "ciou": 3}      # cfg `box_loss` -> box_mode of mmd_focal_loss_box


def check_box_loss(name, weight) -> None:
    """The box regression criterion's two settings, checked on the host (StepConfig, trainer.box_loss_settings, the model.py facade)"""
    if not isinstance(name, str) or name not in BOX_LOSSES:
        raise ValueError(f"box_loss {name!r}: one of {' | '.join(BOX_LOSSES)}")
    if isinstance(weight, bool) or not isinstance(weight, numbers.Real) or not math.isfinite(weight) or not weight > 0:
        raise ValueError(f"box_weight {weight!r}: a finite weight > 0")
    if name == "smooth_l1" and weight != 1:
        raise ValueError(f"box_weight {weight!r} with box_loss smooth_l1: upstream's criterion has no weight (1 only)")


class TeacherPass(NamedTuple):
    """One frozen-net forward of a step that runs on its own (outside the pack)."""
    mod: str                        # the batch entry it reads, or "augmentation" (the KD-list variant's second RGB pass, which reads `x`)
    net: Net
    stream_idx: int                 # its side stream: the teacher's position in ModuleDict order (the second RGB pass: the RGB teacher's)
    label_idx: int                  # its entry of injected teacher_labels = its place among the sources (the second RGB pass: the last)
    x: Optional[torch.Tensor]       # the second RGB pass' input; None: the teacher's own modality


class TeacherOut(NamedTuple):
    """What one pseudo-label source hands the losses; a step holds one per source, in source order (the teachers in ModuleDict order, then
    the second RGB pass)."""
    rows: torch.Tensor              # [B, cap, 6] (x1, y1, x2, y2, score, label)
    cnt: torch.Tensor               # [B] int32
    att: Optional[list]             # per pyramid level its attention map; None with kd_loss = None


class TeacherRun(NamedTuple):
    """What every teacher leg of one step reads."""
    batch: Dict[str, torch.Tensor]
    audio: torch.Tensor             # the student's input (after the audio merge)
    B: int
    A: int
    aug: bool
    use_kd: bool
    labels: Optional[List[tuple]]   # injected teacher_labels, else the teachers decode their own
    fork_event: Any                 # recorded on `main` before the student forward; None: no side streams, every leg runs on `main`
    main: Any


class EvalRecord(NamedTuple):
    """The evaluation record between begin_eval and end_eval: up to max_images images, max_rows predictions (of images that have ground
    truth) and max_gt ground-truth boxes over the whole evaluation.  One int32 buffer `buf` (12 bytes per row, 12 per image, 4 per box):
    cursor[3] + overflow | tp mask [max_rows] | (score, class) `rows` [max_rows, 2] | (sum dx, sum dy, n) `cd` [max_images, 3] | `gt` class
    [max_gt]; the other tensor fields are views of it."""
    buf: torch.Tensor
    cursor: torch.Tensor
    overflow: torch.Tensor
    tp: torch.Tensor
    rows: torch.Tensor
    cd: torch.Tensor
    gt: torch.Tensor
    max_rows: int
    max_images: int
    max_gt: int

    def capacity_message(self) -> str:
        return ("evaluation record capacity exceeded (begin_eval max_images = %d, max_rows = %d, max_gt = %d)"
                % (self.max_images, self.max_rows, self.max_gt))


class CapturedStep(NamedTuple):
    """One captured step variant: its static inputs, the graphs (g_tail None when the backward is not split) and the outputs they write."""
    static: Dict[str, torch.Tensor]
    g_main: Any
    g_tail: Any
    g_opt: Any
    out: Dict[str, Any]


def smallest_level_rows(S: int, B: int) -> int:
    """rows per net on the smallest pyramid level (S/128 squared pixels per image)"""
    return B * (S // 128) ** 2


def pack_eligible(S: int, B: int, G: int, aug: bool, node_whole: bool, pack: bool) -> bool:
    """Do the G frozen teachers of a step at S^2, batch B, run as ONE pack forward?  pack: the engine holds a pack (DistillEngine.pack);
    node_whole: every BiFPN node of the smallest level runs on the whole-node kernel (DistillEngine._node_whole).

    The pack runs every layer of all the frozen teachers as ONE launch over G x B images with per-group weights, on one side stream.  It needs
    whole 128-row tiles per group on every pyramid level (the smallest, S/128 squared, decides) and no per-teacher feature surgery (the
    augmented variant averages images 0 / 1 of each teacher's maps).
    The smallest level needs whole 32-row tiles per net only - the heads run a level that misses the 128-row tiles as plain launches on the
    skinny kernel, engine.Net._head - so D4 / 768^2 at B = 8, 288 rows per net on its 6 x 6 level, packs too.
    The 32-row relaxation holds only where EVERY per-net launch on that level is covered - the heads split it off themselves, the BiFPN nodes
    only on the whole-node kernel, which has no row-tile constraint; a width without one (88 / 288 / 384: D1, D5 - D7), the wide form past
    its row cap or a net with the `FUSE_NODE` test hook off send that level's nodes through mmd_pwconv_fwd, whose 64- / 128-row kernels
    refuse a tile that straddles two nets: those geometries keep the whole-128-row-tile rule, i.e. run one net per stream as before."""
    rows_small = smallest_level_rows(S, B)
    return bool(pack and G > 1 and not aug and S % 128 == 0 and
                (rows_small % 128 == 0 or (rows_small % 32 == 0 and node_whole)))


@dataclass
class StepConfig:
    image_size: int = 512
    conf_threshold: float = 0.3
    nms_threshold: float = 0.5
    merge_iou: float = 0.5
    T: float = 9.0
    p: float = 2.0
    w_main: float = 1.0
    w_kd: float = 0.005
    lr: float = 1e-4
    b1: float = 0.9
    b2: float = 0.999
    eps: float = 1e-8
    grad_clip: float = -1.0
    optimizer: str = "Adam"            # cfg `optimizer`: SGD | Adam | AdamW (src/optimization/train_methods.py:808-836)
    momentum: float = 0.0              # SGD
    weight_decay: float = 0.0          # SGD: cfg weight_decay; AdamW: torch's default 1e-2 (the reference passes none)
    kd_mode: str = "pairwise"          # "pairwise" = ModelWithNMSLoss(.Augmented); "list" = ModelWithNMSKDListLoss
    kd_loss: str = "MTALoss"           # cfg `kd_loss`: MTALoss | AttentionLoss (src/loss/AttentionLoss.py, p = 2 whatever `p` says) | None
    valid_prediction_ids: tuple = (6,)  # VOC id of "car" (src/datasets/BaseDataset.py:141-165)
    label_map: Optional[List[int]] = None
    inclusive_nms: bool = False
    max_boxes: int = 0                 # merged pseudo-labels per image handed to the focal loss; 0 = sized for the worst case
    cand_cap: int = 0                  # rows per image of the candidate / pseudo-label arrays; 0 = every anchor (the reference
                                       # has no cap, src/utils/utils.py:179-205), so nothing can overflow
    augment: bool = False              # cfg audio_augmentation_merge (ModelWithNMSLossAugmented.forward augment=True)
    seed: int = 0                      # cfg `seed` (train.py:120 make_reproducible_run): keys the device-side drop-connect draws
    precision: str = "fp32"            # "bf16": 1x1-conv GEMMs of every net on the bf16 MFMA (fp32 accumulate, fp32 tensors)
    ema_decay: float = 0.0             # extension key: 0 = off; 0 < d < 1: an exponential moving average of the student's weights and BatchNorm
                                       # running statistics rides behind every optimizer launch (csrc/optim.hip mmd_ema_update; 0.9998 is
                                       # the EfficientDet recipe's)
    ema_warmup: bool = True            # d = min(ema_decay, (1 + n) / (10 + n)) at the n-th update (n from 0)
    label_merge: str = "nms"           # extension key: how the teachers' boxes become the pseudo-labels.  "nms": upstream's class-agnostic
                                       # NMS over their concatenation; "wbf": weighted box fusion (csrc/postproc.hip pp_wbf_kernel) at the
                                       # same merge_iou / inclusive_nms - overlapping boxes of one label are averaged, weights = scores
    label_merge_votes: int = 1         # wbf: a fused box needs members from at least this many distinct sources (1 .. number of sources)
    box_loss: str = "smooth_l1"        # extension key: the box regression criterion.  "smooth_l1": upstream's, on (dy, dx, dh, dw); "giou" |
                                       # "diou" | "ciou": an IoU-family loss between the decoded prediction and the pseudo-label, computed per
                                       # positive anchor inside the focal launch (csrc/loss.hip mmd_focal_loss_box)
    box_weight: float = 1.0            # giou / diou / ciou: weight of the regression loss and its gradient (smooth_l1: 1 only)

    def __post_init__(self):
        check_box_loss(self.box_loss, self.box_weight)
        if self.label_merge not in LABEL_MERGES:
            raise ValueError(f"label_merge {self.label_merge!r}: one of {' | '.join(LABEL_MERGES)}")
        v = self.label_merge_votes
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 1 <= v <= 4:
            raise ValueError(f"label_merge_votes {v!r}: an integer between 1 and the number of sources (at most 4)")
        if self.label_merge == "wbf" and not self.conf_threshold > 0:
            # the fusion's weights are the scores: a row of score 0 would pull nothing and still count as a member and a vote
            raise ValueError(f"label_merge wbf needs conf_threshold > 0 (got {self.conf_threshold!r}): the scores are the fusion's weights")
        d = self.ema_decay
        if isinstance(d, bool) or not isinstance(d, numbers.Real) or not (d == 0 or 0.0 < d < 1.0):
            raise ValueError(f"ema_decay {d!r}: 0 (off) or a decay with 0 < d < 1")
        if not isinstance(self.ema_warmup, bool):
            raise ValueError(f"ema_warmup {self.ema_warmup!r}: True or False")


class DistillEngine:
    def __init__(self, student_spec: NetSpec, teacher_specs: Dict[str, NetSpec], device, cfg: StepConfig,
                 world_size: int = 1, process_group=None):
        if cfg.kd_loss not in KD_LOSSES:
            raise Exception(f"Unsupported kd_loss {cfg.kd_loss} on the HIP path")
        if cfg.kd_loss == "AttentionLoss" and cfg.kd_mode == "list":
            # upstream's ModelWithNMSKDListLoss hands AttentionLoss a per-teacher LIST per level: at_loss fails at the first step
            # (AttributeError: 'list' object has no attribute 'shape')
            raise Exception("kd_loss AttentionLoss does not run with the kdlist train methods (upstream fails on the teachers' list)")
        n_src = sum(1 for m in TEACHER_ORDER if m in teacher_specs)
        if cfg.label_merge == "wbf" and cfg.label_merge_votes > n_src:
            raise ValueError(f"label_merge_votes {cfg.label_merge_votes} exceeds the {n_src} teachers whose boxes are fused")
        self.cfg = cfg
        self.device = device
        self.world_size = world_size
        self.pg = process_group
        self.student = Net(student_spec, device, trainable=True, precision=cfg.precision)
        # (a common stem slot lines the teachers' parameter layouts up behind their stems: the pack mode below)
        slot = max(s.stem_out * ((s.in_channels * 9 + 3) // 4 * 4) for s in teacher_specs.values())
        self.teachers: Dict[str, Net] = {m: Net(teacher_specs[m], device, trainable=False, precision=cfg.precision, stem_slot=slot)
                                         for m in TEACHER_ORDER if m in teacher_specs}
        # Teacher pack: the frozen teachers share one body architecture, so each layer of all of them runs as ONE launch over
        # 3 x B images with per-group weights instead of three launches on three streams (fewer, fatter launches beside the student's
        # chain: tools/dev/diag_phases.py proxy - student forward + a frozen net at batch 3B 7.28 ms against 8.41 with three nets on three
        # streams).  MMD_NO_PACK=1: one net per stream
        tl = list(self.teachers.values())
        self.pack = (len(tl) > 1 and not os.environ.get("MMD_NO_PACK") and str(device).startswith("cuda")
                     and pack_nets(tl))
        ps = self.student.ps
        n = ps.n_params
        self.exp_avg = torch.zeros(n, device=device)
        self.exp_avg_sq = torch.zeros(n, device=device)
        self.adam_main = torch.zeros(4, device=device)
        self.adam_head = torch.zeros(4, device=device)
        if cfg.optimizer not in OPT_MODES:
            raise Exception(f"Unsupported optimizer {cfg.optimizer}")
        self.opt_mode = OPT_MODES[cfg.optimizer]
        self.lr = float(cfg.lr)
        # device-side hyper-parameters [lr, beta1, beta2, eps, weight_decay, momentum]: a captured graph sees scheduler updates
        self.hyper = torch.tensor([cfg.lr, cfg.b1, cfg.b2, cfg.eps, cfg.weight_decay, cfg.momentum], device=device)
        self.head_active = torch.zeros(1, dtype=torch.int32, device=device)
        # cfg ema_decay > 0: the averaged copies of (flat, rmean, rvar) and [updates so far, decay of the last update] on the device; one
        # launch behind the optimizer's keeps them up to date (optimizer_body).  Off: no buffer, no launch
        self.ema_flat = self.ema_rmean = self.ema_rvar = self.ema_state = self._ema_scratch = None
        if cfg.ema_decay > 0:
            self.ema_flat, self.ema_rmean, self.ema_rvar = ps.flat.clone(), ps.rmean.clone(), ps.rvar.clone()
            self.ema_state = torch.zeros(2, device=device)
        self.overflow = torch.zeros(1, dtype=torch.int32, device=device)
        self.ws = Arena(device, 256 << 20)        # loss / pseudo-label workspaces (bump, reset per step)
        self.head_ranges = self._head_ranges()
        nc = student_spec.num_classes
        lm = cfg.label_map if cfg.label_map is not None else list(range(nc))
        self.label_map = torch.tensor(lm, dtype=torch.int32, device=device)
        self.valid_mask = valid_class_mask(cfg.valid_prediction_ids)
        self.cap = int(cfg.cand_cap)     # 0: set to the anchor count at the first step
        self._eval: Optional[EvalRecord] = None
        self._merge_aux = None             # label_merge = wbf: the last merge's [B, G, 3] (mean score, members, sources) per fused box
        self._graphs: Dict[str, CapturedStep] = {}       # by step variant ("plain" / "aug")
        self.on_gpu = torch.cuda.is_available() and str(device).startswith("cuda")
        self.concurrent_teachers = True    # the teachers on side streams beside the student; a step of an engine off the GPU turns it off
        self.side_streams: List = []
        self.static: Dict[str, torch.Tensor] = {}
        self.out: Dict[str, torch.Tensor] = {}
        self.n_skip = sum(1 for b in student_spec.blocks if b.skip)
        # data-parallel gradient exchange overlapped with the backward: the backward is issued (and captured) in two
        # segments split before backbone block `ar_split`; the gradients of everything behind it (heads, BiFPN, blocks >=
        # ar_split: ~98 % of the buffer, they sit at the tail of the conv region) are reduced on RCCL's stream while
        # the high-resolution early blocks - about half of the backward's time - still run
        self.ar_split: Optional[int] = self._default_split() if world_size > 1 else None
        env = os.environ.get("MMD_AR_SPLIT")
        if env is not None:
            self.ar_split = None if env in ("", "none", "-1") else int(env)
        self._ar_work = None
        self.force_ar = False        # dev aid: issue the collectives on a one-rank group (bench.py MMD_FORCE_DP)
        # MMD_COMM=rccl: the exchange goes through the C ABI's own RCCL communicator (mmd_comm_*: csrc/comm.hip) on a side HIP stream
        # instead of torch.distributed's ProcessGroupNCCL (same library underneath); default: torch.distributed
        self.comm = None
        self.comm_stream = None
        self.keep = torch.tensor([1.0 - b.drop_rate for b in student_spec.blocks if b.skip], device=device).view(-1, 1)
        # device-side drop-connect draws: Philox key (cfg seed, rank-specific like a per-rank torch seed) and [draw counter, injected flag]
        self.drop_seed = (int(getattr(cfg, "seed", 0)) * 0x9E3779B97F4A7C15 + 0xD1B54A32D192ED03 * (1 + int(os.environ.get("RANK", "0")))) % (1 << 64)
        self.drop_state = torch.zeros(2, dtype=torch.int64, device=device)
        self._drop_injected = False

    # ------------------------------------------------------------------
    def _head_ranges(self):
        """[begin,end) float ranges of the regressor/classifier parameters in the flat buffer."""
        ps = self.student.ps
        conv = [e for e in ps.entries.values() if e.key.startswith(("regressor", "classifier"))]
        b0 = min(e.off for e in conv)
        e0 = ps.n_conv
        bn = [n for n in ps.bn_names if n.startswith(("regressor", "classifier"))]
        lo = min(ps.bn_off[n] for n in bn)
        hi = max(ps.bn_off[n] + ((ps.bn_c[n] + 3) // 4 * 4) for n in bn)
        # heads' conv weights must be the tail of the conv region and their BN channels contiguous
        assert all(e.off >= b0 for e in conv) and all(
            (not k.startswith(("regressor", "classifier"))) or ps.entries[k].off >= b0 for k in ps.order)
        return (b0, e0, ps.gamma_off + lo, ps.gamma_off + hi, ps.beta_off + lo, ps.beta_off + hi)

    def _block_off(self, k: int) -> int:
        ps = self.student.ps
        q = f"backbone_net.model._blocks.{k}."
        return min(e.off for key, e in ps.entries.items() if key.startswith(q))

    def _default_split(self) -> int:
        """First backbone block with more than 2 % of the conv parameters in front of it (D2: block 8, the 64x64 -> 32x32
        stage; the blocks before it own 1.6 % of the gradients and roughly half of the backward's kernel time)."""
        ps = self.student.ps
        k = 1
        for b in self.student.spec.blocks[1:]:
            if self._block_off(b.idx) > 0.02 * ps.n_conv:
                break
            k = b.idx
        return k

    def grad_buckets(self):
        """[(begin, end)] float ranges of the flat gradient buffer per all-reduce phase.  Phase 0 is complete when the
        first backward segment ends, phase 1 (early backbone blocks + all BatchNorm gammas/betas) when the backward ends."""
        ps = self.student.ps
        if self.ar_split is None:
            return [[], [(0, ps.n_params)]]
        o = self._block_off(self.ar_split)
        assert o % 4 == 0
        return [[(o, ps.n_conv)], [(0, o), (ps.n_conv, ps.n_params)]]

    def load(self, student_state, teacher_states: Dict[str, dict]):
        self.student.load_state(student_state)
        for m, net in self.teachers.items():
            net.load_state(teacher_states[m])
        self.reset_ema()

    # ------------------------------------------------------------------ weight averaging (cfg ema_decay)
    def _ema_pairs(self):
        ps = self.student.ps
        return ((ps.flat, self.ema_flat), (ps.rmean, self.ema_rmean), (ps.rvar, self.ema_rvar))

    def reset_ema(self):
        """Start the average again from the live weights, with 0 updates: whoever writes the student's state (load, a broadcast from
        rank 0, a resume from a checkpoint without an average) calls it.  A no-op with ema_decay = 0."""
        if self.ema_flat is None:
            return
        for live, ema in self._ema_pairs():
            ema.copy_(live)
        self.ema_state.zero_()

    def ema_updates(self) -> int:
        return int(self.ema_state[0].item())

    def _ema_exchange(self):
        """contents of (flat, rmean, rvar) <-> the averaged copies, by device copies through one scratch buffer: no pointer moves, so
        the captured graphs stay valid"""
        if self._ema_scratch is None:
            self._ema_scratch = torch.empty_like(self.ema_flat)
        for live, ema in self._ema_pairs():
            tmp = self._ema_scratch[:live.numel()]
            tmp.copy_(live); live.copy_(ema); ema.copy_(tmp)

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block the student computes with the averaged weights and running statistics (validation, export); the live ones
        wait in the EMA buffers and come back on exit, bit for bit.  No training step may run inside."""
        if self.ema_flat is None:
            raise RuntimeError("ema_weights: the engine keeps no averaged weights (cfg ema_decay = 0)")
        self._ema_exchange()
        self.student.refresh()
        try:
            yield self
        finally:
            self._ema_exchange()
            self.student.refresh()

    def set_lr(self, lr: float):
        self.lr = float(lr)            # host copy in double (checkpoints carry it; the device copy is its fp32 rounding)
        self.hyper[0] = lr

    def make_drop_scale(self, batch: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """mask/keep per skip block and sample: floor(keep + U[0,1)) / keep (src/YetAnotherEfficientNet.py:173-182).  Host-driven form
        (torch's generator): tests and callers that inject their own masks; the training loop draws on the device, draw_drop_scale."""
        u = torch.rand(self.n_skip, batch, device=self.device, generator=generator)
        return torch.floor(self.keep + u) / self.keep

    def draw_drop_scale(self, out: torch.Tensor):
        """The same draw as ONE HIP launch (csrc/optim.hip drop_scale_kernel: Philox4x32-10, device-side draw counter): captured at the
        head of g_main, so a replayed step issues no ATen launches.  A caller-injected mask (set_drop_scale) is left alone."""
        call("mmd_drop_scale", out, self.keep, self.n_skip, out.shape[1], self.drop_seed, self.drop_state)

    def set_drop_scale(self, drop_scale: Optional[torch.Tensor]):
        """inject (tensor) or release (None) the masks of the captured step: an injected mask survives the graph's own draw."""
        inject = drop_scale is not None
        if inject:
            self.static["drop_scale"].copy_(drop_scale)
        if inject != self._drop_injected:
            self.drop_state[1] = 1 if inject else 0
            self._drop_injected = inject

    # ------------------------------------------------------------------
    def _caps(self, A: int):
        if self.cap <= 0:
            self.cap = A
        return self.cap

    def _begin_workspace(self, B: int):
        """Start the step workspace afresh; the NMS kernels' mask words come first in it."""
        self.ws.reset()
        self.mask_ws = self.ws.alloc((B * 1024 * 16,), torch.int64)

    def _merge(self, rows_t, cnt_t, B: int, augment: bool):
        """cross-teacher concat + NMS (cfg label_merge = nms, upstream's) or weighted box fusion (wbf) -> (boxes [B,G,5], nbox [B], G).
        Up to 4 sources: the teachers in ModuleDict order, then the "augmentation" pass of ModelWithNMSKDListLossAugmented.  Leaves the
        fusion's per-box record in self._merge_aux (None after an NMS)."""
        nt, cap = len(rows_t), self.cap
        nmax = nt * cap * (2 if (augment and B >= 2) else 1)
        G = self.cfg.max_boxes if self.cfg.max_boxes > 0 else nmax
        self._merge_aux = None
        if self.cfg.label_merge == "wbf":
            # (a fused list is never longer than the gathered one, so G holds it whenever it held the NMS's)
            boxes, nbox, self._merge_aux = wbf_merge(self.ws, rows_t, cnt_t, B, cap, self.cfg.merge_iou, self.cfg.inclusive_nms, G,
                                                     self.cfg.label_merge_votes, self.overflow, merge01=augment)
            return boxes, nbox, G
        boxes = self.ws.alloc((B, G, 5)); nbox = self.ws.alloc((B,), torch.int32)
        vp = ctypes.c_void_p
        srcs = (vp * nt)(*[t.data_ptr() for t in rows_t]); cnts = (vp * nt)(*[t.data_ptr() for t in cnt_t])
        call("mmd_nms_merge_n", srcs, cnts, nt, float(self.cfg.merge_iou), 1 if self.cfg.inclusive_nms else 0, B, boxes, nbox, G,
             self.mask_ws, self.overflow, 1 if augment else 0, cap, nms_workspace(self.ws, B, nmax))
        return boxes, nbox, G

    def merge_labels(self, rows_t: List[torch.Tensor], cnt_t: List[torch.Tensor], augment: bool = False):
        """The step's cross-teacher merge alone, as cfg `label_merge` sets it: per source rows [B, cap, 6] (x1, y1, x2, y2, score, label)
        and counts [B] int32 on the device (`labels_from_rows` makes them from host arrays) -> (boxes [B, G, 5], nbox [B], aux), aux
        [B, G, 3] = (mean member score, members, distinct sources) per fused box with `wbf`, None with `nms`.  The results lie in the
        step workspace, which this call starts afresh like a step does: read them before the next step, and a step's outputs before it."""
        if not rows_t or len(rows_t) != len(cnt_t):
            raise ValueError("merge_labels: one count array per source")
        B, cap = int(rows_t[0].shape[0]), int(rows_t[0].shape[1])
        self._caps(cap)
        if any(tuple(r.shape) != (B, self.cap, 6) for r in rows_t):
            raise ValueError(f"merge_labels: every source is [B, {self.cap}, 6] (the engine's candidate capacity)")
        self._begin_workspace(B)
        boxes, nbox, _ = self._merge(list(rows_t), list(cnt_t), B, bool(augment))
        return boxes, nbox, self._merge_aux

    def _pseudo_labels(self, net: Net, cls, reg, B: int, A: int, S: int):
        return decode_nms(self.ws, net, cls, reg, B, A, S, self._caps(A), self.cfg.conf_threshold, self.valid_mask, self.label_map,
                          self.cfg.nms_threshold, self.cfg.inclusive_nms, self.overflow)

    def _att_p(self) -> float:
        """exponent of the attention maps: cfg `p` for MTALoss; AttentionLoss is built with its default p = 2 upstream (src/utils/utils.py)"""
        return 2.0 if self.cfg.kd_loss == "AttentionLoss" else float(self.cfg.p)

    def _attention(self, net: Net):
        """Spatial attention maps a[b, j] = mean_c f^p of the five BiFPN outputs of `net` in ONE launch: the final cell writes
        them into one pyramid row buffer (engine._bifpn), so the maps are row slices of one vector.  -> (all, [per level])"""
        pyr, fcat = net._pyr, net._fcat
        a = self.ws.alloc((pyr.total,))
        call("mmd_mta_attention", fcat, a, pyr.total, fcat.shape[1], self._att_p())
        return a, pyr.levels(a)

    def labels_from_rows(self, per_teacher: List[List], A: int) -> List[tuple]:
        """Host pseudo-labels -> the device form `step_body(teacher_labels=...)` takes: per teacher a list of B arrays [n,6]
        (x1, y1, x2, y2, score, class: what `logits_to_ground_truth(include_scores=True)` returns,
        src/utils/utils.py:234-324) -> (rows [B, cap, 6] fp32, count [B] int32)."""
        self._caps(A)
        out = []
        for lab in per_teacher:
            B = len(lab)
            rows = torch.zeros(B, self.cap, 6)
            cnt = torch.zeros(B, dtype=torch.int32)
            for i, a in enumerate(lab):
                a = np.asarray(a, dtype=np.float32).reshape(-1, 6)
                if a.shape[0] > self.cap:
                    raise ValueError("more pseudo-labels than the candidate arena holds")
                rows[i, :a.shape[0]] = torch.from_numpy(a)
                cnt[i] = a.shape[0]
            out.append((rows.to(self.device), cnt.to(self.device)))
        return out

    def step_body(self, batch: Dict[str, torch.Tensor], drop_scale: Optional[torch.Tensor], teacher_labels: Optional[List[tuple]] = None,
                  train: bool = True):
        """Issues the whole step on the current stream.  batch tensors are NCHW fp32 on device.
        teacher_labels (optional): per teacher (rows [B, cap, 6], count [B]) pseudo-labels computed elsewhere (cached labels of the
        frozen teachers, or a reference run's labels in the parity tests); the teachers' own decode + NMS is then skipped, their
        forward still feeds the MTA loss.
        train=False: the losses of `validate()` (src/optimization/train_methods.py:1083-1185): eval-mode student (running
        BatchNorm statistics, no drop-connect), same pseudo-labels and loss terms, no backward."""
        cfg = self.cfg
        B = batch["audio"].shape[0]
        # validate() upstream calls model(..., validate=True) with `augment` left at its default False
        # (src/optimization/train_methods.py:1083-1185): the validation losses never see the audio merge / feature averaging / label merge
        aug = bool(cfg.augment and train)
        use_kd = cfg.kd_loss != "None"          # kd_loss = None: no attention maps, no KD term, no feature gradient (loss_kd = zeros upstream)
        aug_pass = cfg.kd_mode == "list" and batch.get("aug_rgb") is not None      # the KD-list variant's second RGB pass: one more source
        self._begin_workspace(B)
        fork_event = self._fork()
        audio, cls_s, reg_s, feats_s = self._student_forward(batch, drop_scale, train, aug)
        A = cls_s.shape[1]
        self._caps(A)
        a_s, da_all, kd = self._kd_buffers(use_kd, len(self.teachers) + (1 if aug_pass else 0), len(feats_s))
        run = TeacherRun(batch, audio, B, A, aug, use_kd, teacher_labels, fork_event, torch.cuda.current_stream())
        outs = self._run_teachers(run, self._teacher_passes(batch, aug_pass))
        self._join_teachers(run)
        if use_kd:
            self._kd_losses(outs, a_s, da_all, feats_s, kd, B)
        d_all = self._kd_feature_grad(da_all, feats_s) if train and use_kd else None
        rows_t, cnt_t = [o.rows for o in outs], [o.cnt for o in outs]
        boxes, nbox, G = self._merge(rows_t, cnt_t, B, aug)      # cross-teacher merge -> annotations
        main, dcls, dreg = self._main_loss(cls_s, reg_s, boxes, nbox, G, B, train)
        if train:
            self._start_backward(dcls, dreg, d_all, len(feats_s))
        self.out = {"reg": main[0:1], "cls": main[1:2], "kd": kd, "boxes": boxes, "nbox": nbox, "label_aux": self._merge_aux,
                    "cls_s": cls_s, "reg_s": reg_s, "feats_s": feats_s, "rows_t": rows_t, "cnt_t": cnt_t}
        return self.out

    def _fork(self):
        """-> the event the teachers' side streams start behind, recorded before the student forward is enqueued; None: no side streams
        (`concurrent_teachers` off, which an engine off the GPU sets here for good)."""
        if not self.on_gpu:
            self.concurrent_teachers = False
        return torch.cuda.current_stream().record_event() if self.concurrent_teachers else None

    def _student_forward(self, batch, drop_scale, train: bool, aug: bool):
        """-> (audio, cls_s, reg_s, feats_s): the student's input as it ran (after the audio merge) and its outputs."""
        st = self.student
        st.begin_step()
        audio = batch["audio"]
        B = audio.shape[0]
        if aug and B >= 2:      # merge_batch_0_1: image 1 <- log10(a0^10 + a1^10), out of place
            merged = st._alloc(*audio.shape)
            call("mmd_audio_merge01", audio, merged, audio[0].numel(), B)
            audio = merged
        st.mark_block, st.mark_event = int(os.environ.get("MMD_PACK_STAGGER", "-1")), None      # (dev: hold the teacher pack until the student passed block k)
        cls_s, reg_s, feats_s = st.forward(audio, train=train, drop_scale=drop_scale if train else None)
        return audio, cls_s, reg_s, feats_s

    def _kd_buffers(self, use_kd: bool, nt: int, nlv: int):
        """-> (a_s, da_all, kd): the student's attention maps per level, the gradient w.r.t. them (both None without a KD term) and the
        zeroed KD loss terms of nt sources - allocated before any teacher runs."""
        st = self.student
        a_s = da_all = None
        if use_kd:
            _, a_s = self._attention(st)
            # gradient w.r.t. the student's maps, one vector over the pyramid rows (zeroed: MTA teachers accumulate into it
            # with atomics, and the padding rows of a pyramid must read as zero in the backward)
            da_all = self.ws.alloc((st._pyr.total,))
            call("mmd_memset_async", da_all, 0, da_all.numel() * 4)
        kd = self.ws.alloc((nt if self.cfg.kd_mode == "pairwise" else 1, nlv))
        call("mmd_memset_async", kd, 0, kd.numel() * 4)
        return a_s, da_all, kd

    # ---- the frozen teachers: independent of each other and of the student forward, so they are issued on side streams (parallel branches
    # of the captured graph) and their many small kernels fill the chip together
    def _teacher_passes(self, batch, aug_pass: bool) -> List[TeacherPass]:
        passes = [TeacherPass(mod, net, ti, ti, None) for ti, (mod, net) in enumerate(self.teachers.items())]
        if aug_pass:
            # ModelWithNMSKDListLossAugmented.forward(augment=True) (src/optimization/train_methods.py:73-110): the RGB teacher once more,
            # on `label` = RGB frames of the recordings whose audio was mixed into this batch; its pseudo-labels are concatenated after
            # the teachers' and its features join the MTA list.  Same net object, same side stream: the second pass starts after the
            # first one's labels / attention maps have been taken (stream order), so it may reuse the net's arena.
            if "rgb" not in self.teachers:
                raise ValueError("the augmentation pass runs the RGB teacher")
            rgb = list(self.teachers).index("rgb")
            passes.append(TeacherPass("augmentation", self.teachers["rgb"], rgb, len(self.teachers), batch["aug_rgb"]))
        return passes

    def _stagger_block(self) -> int:
        """Staggered teachers: the frozen nets have the same layer sequence, so three streams started together run in lockstep - three
        MFMA-bound GEMMs at once, then three HBM-bound depthwise convs at once.  Teacher i+1 therefore starts once teacher i is past
        the high-resolution stages (its second stride-2 block: D2 block 5): 20.3-20.7 -> 19.9-20.1 ms/step in alternating runs
        (profiles/r02_notes.md).  MMD_STAGGER=<block> overrides, -1 disables.  Holding teacher 0 behind the student as well measured
        slower (20.3-20.5)."""
        s2 = [b.idx for b in next(iter(self.teachers.values())).spec.blocks if b.stride == 2]
        return int(os.environ.get("MMD_STAGGER", str(s2[1] if len(s2) > 1 else -1)))

    def _node_whole(self, B: int) -> bool:
        """pack_eligible's `node_whole`: do the BiFPN nodes of the teachers' smallest level run on the whole-node kernel?"""
        net = next(iter(self.teachers.values()))
        rows = len(self.teachers) * smallest_level_rows(self.cfg.image_size, B)
        return bool(net.FUSE_NODE and net.ps.flat.is_cuda and
                    _lib.LIB.load().mmd_bifpn_node_fused_supported(net.spec.fpn_w) == 1 and
                    (net.spec.fpn_w <= 160 or rows <= net.NODE_FUSE_WIDE_MAXROWS))

    def _run_teachers(self, run: TeacherRun, passes: List[TeacherPass]) -> List[TeacherOut]:
        """The pack (where the geometry allows one) and every pass outside it -> one TeacherOut per source, in source order."""
        G = len(self.teachers)
        if run.fork_event is not None and not self.side_streams:
            self.side_streams = [torch.cuda.Stream() for _ in self.teachers]
        outs: List[TeacherOut] = []
        if pack_eligible(self.cfg.image_size, run.B, G, run.aug, self._node_whole(run.B), self.pack):
            npk = min(G, max(2, int(os.environ.get("MMD_PACK_SPLIT", G))))      # (dev: pack the first npk teachers, the others on their own streams)
            outs += self._run_pack(run, npk)
            passes = [p for p in passes if p.x is not None or p.stream_idx >= npk]      # (the KD-list variant's extra RGB pass still runs on its own)
        stagger, prev_net = self._stagger_block(), None
        for p in passes:
            outs.append(self._run_teacher(run, p, stagger, prev_net))
            if p.x is None:
                prev_net = p.net
        return outs

    def _side_stream(self, run: TeacherRun, idx: int):
        return run.main if run.fork_event is None else self.side_streams[idx]

    def _run_pack(self, run: TeacherRun, npk: int) -> List[TeacherOut]:
        """The first npk teachers as one pack forward on side stream 0, behind the fork (and the student's MMD_PACK_STAGGER block)."""
        B, st = run.B, self.student
        nets = list(self.teachers.values())[:npk]
        net0 = nets[0]
        side = self._side_stream(run, 0)
        if run.fork_event is not None:
            side.wait_event(run.fork_event)
            if st.mark_event is not None:
                side.wait_event(st.mark_event)
        with torch.cuda.stream(side):
            net0.begin_step()
            cls_p, reg_p, feats_p = net0.forward([run.batch[m] for m in list(self.teachers)[:npk]], train=False, pack=nets)
            if run.labels is None:
                rows_p, cnt_p = self._pseudo_labels(net0, cls_p, reg_p, npk * B, run.A, self.cfg.image_size)
            if run.use_kd:
                _, a_lv = self._attention(net0)
        outs = []
        for gi in range(npk):
            rows, cnt = run.labels[gi] if run.labels is not None else (rows_p[gi * B:(gi + 1) * B], cnt_p[gi * B:(gi + 1) * B])
            att = [a_lv[l][gi * B * f.H * f.W:(gi + 1) * B * f.H * f.W] for l, f in enumerate(feats_p)] if run.use_kd else None
            outs.append(TeacherOut(rows, cnt, att))
        return outs

    def _run_teacher(self, run: TeacherRun, p: TeacherPass, stagger: int, prev_net: Optional[Net]) -> TeacherOut:
        """One net on its side stream: behind the fork and, staggered, behind the previous teacher's `stagger` block."""
        net, B = p.net, run.B
        side = self._side_stream(run, p.stream_idx)
        # (the second RGB pass waits on neither event: it runs on the first RGB pass' stream, behind it in stream order)
        if run.fork_event is not None and p.x is None:
            side.wait_event(run.fork_event)
            if stagger >= 0 and prev_net is not None and prev_net.mark_event is not None:
                side.wait_event(prev_net.mark_event)
            net.mark_block, net.mark_event = stagger, None
        with torch.cuda.stream(side):
            net.begin_step()
            cls_t, reg_t, feats_t = net.forward(p.x if p.x is not None else (run.audio if p.mod == "audio" else run.batch[p.mod]), train=False)
            if run.aug and B >= 2 and run.use_kd:      # average_batch_0_1 on the (already consumed by the heads) feature maps
                for f in feats_t:
                    call("mmd_avg_image01", f.z, f.H * f.W * f.C)
            if run.labels is not None:
                rows, cnt = run.labels[p.label_idx]
            else:
                rows, cnt = self._pseudo_labels(net, cls_t, reg_t, B, run.A, self.cfg.image_size)
            att = self._attention(net)[1] if run.use_kd else None
        return TeacherOut(rows, cnt, att)

    def _join_teachers(self, run: TeacherRun):
        if run.fork_event is not None:
            for side in self.side_streams:
                run.main.wait_stream(side)

    def _kd_losses(self, outs: List[TeacherOut], a_s, da_all, feats_s, kd, B: int):
        """every (level, teacher) KD term of the step in one launch (pairwise: nt x 5 losses; list: 5)"""
        cfg, nt, nlv = self.cfg, len(outs), len(feats_s)
        vp = ctypes.c_void_p
        p_as = (vp * nlv)(*[t.data_ptr() for t in a_s])
        p_at = (vp * (nt * nlv))(*[o.att[l].data_ptr() for o in outs for l in range(nlv)])
        p_da = (vp * nlv)(*[t.data_ptr() for t in self.student._pyr.levels(da_all)])
        hw = (ctypes.c_int * nlv)(*[f.H * f.W for f in feats_s])
        if cfg.kd_loss == "AttentionLoss":
            call("mmd_at_loss_multi", p_as, p_at, p_da, hw, nlv, nt, B, kd, float(cfg.w_kd), self.ws.alloc((nt * nlv * B,)))
        else:
            call("mmd_mta_kl_multi", p_as, p_at, p_da, hw, nlv, nt, 0 if cfg.kd_mode == "pairwise" else 1, B, float(cfg.T), kd,
                 float(cfg.w_kd))

    def _kd_feature_grad(self, da_all, feats_s):
        """one launch for d attention / d f -> the KD gradient w.r.t. the student's BiFPN outputs, one pyramid row buffer"""
        st = self.student
        d_all = st._alloc(st._pyr.total, feats_s[0].C)
        call("mmd_mta_attention_bwd", st._fcat, da_all, d_all, st._pyr.total, feats_s[0].C, self._att_p(), 0)
        return d_all

    def _main_loss(self, cls_s, reg_s, boxes, nbox, G: int, B: int, train: bool):
        """focal + box regression loss with gradients w.r.t. (pre-sigmoid) classifier logits and regression -> (main [2] = (reg, cls), dcls, dreg)"""
        cfg, st = self.cfg, self.student
        A, nc = cls_s.shape[1], st.spec.num_classes
        assign = self.ws.alloc((B * A,), torch.int32); npos = self.ws.alloc((B,), torch.int32)
        acc = self.ws.alloc((2 * B,), torch.float64); main = self.ws.alloc((2,))
        dcls = st._alloc(B, A, nc); dreg = st._alloc(B, A, 4)
        any_boxes = self.head_active if train else self.ws.alloc((1,), torch.int32)
        args = (cls_s, reg_s, st.anchors(cfg.image_size), boxes, nbox, G, B, A, nc, assign, npos, acc, main, dcls, dreg,
                float(cfg.w_main), 1, any_boxes)
        if cfg.box_loss == "smooth_l1":
            call("mmd_focal_loss", *args)
        else:      # the same launches with an IoU-family criterion in the regression slot
            call("mmd_focal_loss_box", *args, BOX_LOSSES[cfg.box_loss], float(cfg.box_weight))
        return main, dcls, dreg

    def _start_backward(self, dcls, dreg, d_all, nlv: int):
        """zero the gradients, then the student's backward up to block `ar_split` (all of it when the backward is not split)"""
        if _lib.dev_switch("MMD_DEV_NO_BWD"):      # (MMD_DEV_NO_BWD=1: timing experiment - forward + losses only)
            return
        st = self.student
        call("mmd_memset_async", st.ps.grad, 0, st.ps.grad.numel() * 4)
        dfe = st._pyr.levels(d_all) if d_all is not None else [None] * nlv
        st.backward(dcls, dreg, dfe, stop_before=self.ar_split, dfeat_pyr=d_all)

    def backward_tail(self):
        """Second backward segment (backbone blocks < ar_split + stem); a no-op when the backward is not split."""
        if self.ar_split is not None:
            self.student.backward_finish(self.ar_split)

    def init_comm(self, rank: int):
        """Create the C-ABI RCCL communicator (MMD_COMM=rccl).  The 128-byte rendezvous token is made on rank 0 and handed out through
        the already-initialised torch.distributed group (any backend: it only carries these 128 bytes)."""
        import torch.distributed as dist
        dll = _lib.LIB.load()
        tok = (ctypes.c_char * 128)()
        if rank == 0:
            rc = dll.mmd_comm_unique_id(ctypes.cast(tok, ctypes.c_void_p))
            if rc != 0:
                raise RuntimeError(f"mmd_comm_unique_id failed with status {rc}")
        box = [bytes(tok)]
        if self.world_size > 1:
            dist.broadcast_object_list(box, src=0, group=self.pg)
        h = ctypes.c_void_p()
        buf = ctypes.create_string_buffer(box[0], 128)
        rc = dll.mmd_comm_init(ctypes.cast(ctypes.pointer(h), ctypes.c_void_p), rank, self.world_size, ctypes.cast(buf, ctypes.c_void_p))
        if rc != 0:
            raise RuntimeError(f"mmd_comm_init failed with status {rc}")
        self.comm = h
        self.comm_stream = torch.cuda.Stream()

    def close_comm(self):
        if self.comm is not None:
            torch.cuda.synchronize()
            _lib.LIB.load().mmd_comm_destroy(self.comm)
            self.comm = None

    def _comm_allreduce(self, phase):
        """C-ABI path: buckets of `phase` on the communicator's stream, ordered after everything enqueued on the compute stream so
        far; phase 1 also makes the compute stream wait for the whole exchange."""
        dll = _lib.LIB.load()
        g = self.student.ps.grad
        buckets = self.grad_buckets()
        cur = torch.cuda.current_stream()
        self.comm_stream.wait_event(cur.record_event())
        sp = self.comm_stream.cuda_stream

        def red(t, n, dtype, op):
            rc = dll.mmd_comm_allreduce_bucket(self.comm, ctypes.c_void_p(t.data_ptr()), n, dtype, op, ctypes.c_void_p(sp))
            if rc != 0:
                raise RuntimeError(f"mmd_comm_allreduce_bucket failed with status {rc}")
        if phase in (0, None):
            for b, e in buckets[0]:
                red(g[b:e], e - b, 0, 0)
            red(self.head_active, 1, 1, 1)
        if phase in (1, None):
            for b, e in buckets[1]:
                red(g[b:e], e - b, 0, 0)
            cur.wait_event(self.comm_stream.record_event())

    def allreduce_grads(self, phase: Optional[int] = None):
        """RCCL all-reduce(sum) of the flat student gradient buffer (teachers are frozen: nothing else is
        exchanged).  The 1/world average is folded into the optimizer's grad_scale.  head_active is reduced
        with max so that every rank gates the same parameter ranges (ranks may disagree on whether their
        batch had pseudo-labels).

        phase 0: issued after the first backward segment, asynchronously - the collective runs on the process group's
        own stream (ordered after everything enqueued so far) next to the second backward segment.  phase 1: the
        remaining ranges after the backward's end; it also makes the current stream wait for phase 0.  phase None: both."""
        if self.world_size <= 1 and not self.force_ar:
            return
        if self.comm is not None:
            return self._comm_allreduce(phase)
        import torch.distributed as dist
        g = self.student.ps.grad
        buckets = self.grad_buckets()
        if phase in (0, None):
            self._ar_work = [dist.all_reduce(g[b:e], op=dist.ReduceOp.SUM, group=self.pg, async_op=True)
                             for b, e in buckets[0]]
            self._ar_work.append(dist.all_reduce(self.head_active, op=dist.ReduceOp.MAX, group=self.pg, async_op=True))
        if phase in (1, None):
            work = (self._ar_work or []) + [dist.all_reduce(g[b:e], op=dist.ReduceOp.SUM, group=self.pg, async_op=True)
                                            for b, e in buckets[1]]
            for w in work:
                w.wait()
            self._ar_work = None

    def optimizer_body(self):
        cfg, ps = self.cfg, self.student.ps
        gs = 1.0 / self.world_size
        if cfg.grad_clip > 0:
            if self.world_size > 1:
                ps.grad.mul_(gs)
                gs = 1.0
            ws = self.ws.alloc((1,), torch.float64)
            call("mmd_clip_grad_norm", ps.grad, ps.grad.numel(), float(cfg.grad_clip), ws)
        args = (ps.flat, ps.grad, self.exp_avg, self.exp_avg_sq, self.adam_main, self.adam_head, self.hyper, self.head_active,
                *self.head_ranges, float(gs), ps.n_params)
        if self.opt_mode == 0:
            call("mmd_adam_step_gated", *args)
        else:
            call("mmd_opt_step_gated", self.opt_mode, *args)
        if self.ema_flat is not None:
            # reads ps.flat only, so its order against refresh_wt() does not matter.  Every rank holds the same weights after the
            # all-reduced step, hence the same average: no collective
            call("mmd_ema_update", ps.flat, self.ema_flat, ps.n_params, ps.rmean, self.ema_rmean, ps.bn_total, ps.rvar, self.ema_rvar,
                 ps.bn_total, self.ema_state, float(cfg.ema_decay), 1 if cfg.ema_warmup else 0)
        self.student.refresh_wt()

    # ------------------------------------------------------------------ eager / graph drivers
    def step(self, batch: Dict[str, torch.Tensor], drop_scale: Optional[torch.Tensor] = None):
        """Eager step (no graph): forward, losses, backward, all-reduce, Adam."""
        B = batch["audio"].shape[0]
        if drop_scale is None:
            if self._drop_injected:
                # an earlier replay(..., drop_scale=mask) / set_drop_scale(mask) left the device flag up: mmd_drop_scale would then leave the
                # fresh buffer below unfilled (garbage drop-connect scales, no error) - release the injection before drawing
                self.set_drop_scale(None)
            drop_scale = torch.empty(self.n_skip, B, device=self.device)
            self.draw_drop_scale(drop_scale)
        out = self.step_body(batch, drop_scale)
        self.allreduce_grads(0)
        self.backward_tail()
        self.allreduce_grads(1)
        self.optimizer_body()
        return out

    @staticmethod
    def _variant(batch) -> str:
        return "aug" if (batch is not None and batch.get("aug_rgb") is not None) else "plain"

    def _training_state(self) -> List[torch.Tensor]:
        """every tensor that a step leaves to the next one (the averaged weights and their update counter too: a warm-up step is not an update)"""
        ps = self.student.ps
        state = [ps.flat, ps.rmean, ps.rvar, ps.nbt, self.exp_avg, self.exp_avg_sq, self.adam_main, self.adam_head, self.head_active]
        if self.ema_flat is not None:
            state += [self.ema_flat, self.ema_rmean, self.ema_rvar, self.ema_state]
        return state

    def _warm_up(self, teacher_labels):
        """two eager steps on the static inputs, on a stream of their own: they size the arenas"""
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                self.step_body(self.static, self.static["drop_scale"], teacher_labels=teacher_labels)
                self.backward_tail()
                self.optimizer_body()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()

    def capture(self, batch: Dict[str, torch.Tensor], teacher_labels: Optional[List[tuple]] = None):
        """Warm up eagerly (sizes the arenas), then capture forward+loss+backward and the optimizer as
        hipGraphs (the backward in two segments when world_size > 1); the gradient all-reduce is launched eagerly between
        them (RCCL is not captured) and overlaps with the second backward segment.
        One set of graphs per step variant: "plain", and "aug" when the batch carries `aug_rgb` (the extra RGB-teacher pass of
        ModelWithNMSKDListLossAugmented); replay() picks by the batch's keys and captures a missing variant on first use.
        teacher_labels: as step_body - the captured step then reads its pseudo-labels from these very tensors (cached labels of the frozen
        teachers: write new ones into them between replays)."""
        B = batch["audio"].shape[0]
        arenas = [self.ws, self.student.arena, self.student.zarena] + [a for n in self.teachers.values() for a in (n.arena, n.zarena)]
        for arena in arenas:
            arena.frozen = False             # a later variant may need more workspace: chunks are only ever appended
        self.static = {k: v.clone() for k, v in batch.items() if v is not None}
        self.static["drop_scale"] = self.make_drop_scale(B)
        torch.cuda.synchronize()
        # snapshot so the warm-up steps do not change the training trajectory
        state = self._training_state()
        snap = [t.clone() for t in state]
        self._warm_up(teacher_labels)
        for arena in arenas:
            arena.frozen = True
        # thread_local: with a process group alive, the RCCL watchdog thread polls its own events; under the default
        # "global" mode such a call from another thread would invalidate the capture
        self.g_main = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.g_main, capture_error_mode="thread_local"):
            self.draw_drop_scale(self.static["drop_scale"])      # (no-op while a mask is injected: set_drop_scale)
            self.step_body(self.static, self.static["drop_scale"], teacher_labels=teacher_labels)
        out = self.out
        self.g_tail = None
        if self.ar_split is not None:
            self.g_tail = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.g_tail, capture_error_mode="thread_local"):
                self.backward_tail()
        self.g_opt = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.g_opt, capture_error_mode="thread_local"):
            self.optimizer_body()
        for dst, src in zip(state, snap):
            dst.copy_(src)
        self.student.refresh()
        torch.cuda.synchronize()
        self._graphs[self._variant(batch)] = CapturedStep(self.static, self.g_main, self.g_tail, self.g_opt, out)

    def replay(self, batch: Optional[Dict[str, torch.Tensor]] = None, drop_scale: Optional[torch.Tensor] = None):
        if batch is not None:
            key = self._variant(batch)
            if key not in self._graphs:
                self.capture(batch)
            cs = self._graphs[key]
            self.static, self.g_main, self.g_tail, self.g_opt, self.out = cs.static, cs.g_main, cs.g_tail, cs.g_opt, cs.out
            for k, v in batch.items():
                if v is not None:
                    self.static[k].copy_(v, non_blocking=True)
        if drop_scale is not None or self._drop_injected:
            self.set_drop_scale(drop_scale)
        self.g_main.replay()
        self.allreduce_grads(0)
        if self.g_tail is not None:
            self.g_tail.replay()
        self.allreduce_grads(1)
        self.g_opt.replay()
        return self.out

    def _predict_device(self, batch: Dict[str, torch.Tensor]):
        """The device half of the evaluation path: eval-mode student detections and the merged multi-teacher pseudo ground truth.
        -> (rows_s [B,cap,6], cnt_s [B], boxes [B,G,5], nbox [B], G, B), all in the step workspace."""
        S = self.cfg.image_size
        B = batch["audio"].shape[0]
        self._begin_workspace(B)
        st = self.student
        st.refresh()
        st.begin_step()
        cls_s, reg_s, _ = st.forward(batch["audio"], train=False)
        A = cls_s.shape[1]
        rows_s, cnt_s = self._pseudo_labels(st, cls_s, reg_s, B, A, S)
        labels = []
        for mod, net in self.teachers.items():
            net.begin_step()
            cls_t, reg_t, _ = net.forward(batch[mod], train=False)
            labels.append(self._pseudo_labels(net, cls_t, reg_t, B, A, S))
        boxes, nbox, G = self._merge([r for r, _ in labels], [c for _, c in labels], B, False)
        return rows_s, cnt_s, boxes, nbox, G, B

    @torch.no_grad()
    def predict(self, batch: Dict[str, torch.Tensor]):
        """Evaluation path (get_predictions_multiteacher): student detections [n,6] per image from an
        eval-mode forward, and the merged multi-teacher pseudo ground truth [m,5] per image, as numpy lists."""
        rows_s, cnt_s, boxes, nbox, G, B = self._predict_device(batch)
        torch.cuda.synchronize()
        cs, nb = cnt_s.cpu().tolist(), nbox.cpu().tolist()
        preds = [rows_s[i, :cs[i]].cpu().numpy() for i in range(B)]
        labels = [boxes[i, :nb[i]].cpu().numpy() for i in range(B)]
        return preds, labels

    # ---- evaluation statistics on the device (csrc/evalstats.hip): begin_eval, eval_batch x N, end_eval -> metrics.table_from_stats
    def begin_eval(self, max_images: int, max_rows: int, max_gt: Optional[int] = None):
        """Allocate and reset the evaluation record (EvalRecord has the layout); max_gt defaults to max_rows."""
        max_images, max_rows = int(max_images), int(max_rows)
        max_gt = max_rows if max_gt is None else int(max_gt)
        if min(max_images, max_rows, max_gt) <= 0:
            raise ValueError("begin_eval: capacities must be positive")
        buf = torch.empty(4 + 3 * max_rows + 3 * max_images + max_gt, dtype=torch.int32, device=self.device)
        buf[:4].zero_()          # cursor and sticky flag; the kernel writes every entry of the record before anyone reads it
        o = 4
        tp = buf[o:o + max_rows]; o += max_rows
        rows = buf[o:o + 2 * max_rows].view(torch.float32); o += 2 * max_rows
        cd = buf[o:o + 3 * max_images].view(torch.float32); o += 3 * max_images
        gt = buf[o:o + max_gt].view(torch.float32)
        self._eval = EvalRecord(buf=buf, cursor=buf[0:3], overflow=buf[3:4], tp=tp, rows=rows, cd=cd, gt=gt,
                                max_rows=max_rows, max_images=max_images, max_gt=max_gt)

    @torch.no_grad()
    def eval_batch(self, batch: Dict[str, torch.Tensor]):
        """predict's device work, then ONE mmd_eval_match call that appends the batch's statistics to the record: no synchronize, no
        device-to-host copy."""
        ev = self._eval
        if ev is None:
            raise RuntimeError("eval_batch without begin_eval")
        rows_s, cnt_s, boxes, nbox, G, B = self._predict_device(batch)
        n = int(_lib.LIB.load().mmd_eval_ws_floats(self.cap, G))
        if n < 0:
            raise RuntimeError(f"mmd_eval_ws_floats({self.cap}, {G}) failed with status {n}")
        ws = self.ws.alloc((B * n,)) if n else None
        call("mmd_eval_match", rows_s, cnt_s, self.cap, boxes, nbox, G, B, ev.rows, ev.tp, ev.max_rows, ev.cd,
             ev.max_images, ev.gt, ev.max_gt, ev.cursor, ws, ev.overflow)

    def end_eval(self) -> dict:
        """The record -> plain numpy: score / label float32 [n] and tp int32 [n] (bit k: true positive at IoU 0.5 + 0.05 k) of the
        predictions in image order, cd float32 [images, 3] (sum dx, sum dy, n_boxes), gt float32 [m] ground-truth classes.  The 4-int
        header is read first (the one synchronize of the evaluation), then only the rows in front of the cursor are copied: the
        traffic follows the data, not the capacity.  Raises when the record (or a pseudo-label array, check_overflow) was too small."""
        return self._record_to_host(*self._close_eval("end_eval"))

    def _close_eval(self, who: str):
        """Ends the evaluation: -> (record, rows, images, classes) behind the cursor, after the overflow checks."""
        ev = self._eval
        if ev is None:
            raise RuntimeError(f"{who} without begin_eval")
        self._eval = None
        if int(ev.overflow.item()):
            raise RuntimeError(ev.capacity_message())
        self.check_overflow()
        nr, ni, ng = (int(v) for v in ev.cursor.cpu().tolist())
        return ev, nr, ni, ng

    @staticmethod
    def _record_to_host(ev, nr, ni, ng) -> dict:
        tp = ev.tp[:nr].cpu().numpy()
        rows = ev.rows[:2 * nr].cpu().numpy().reshape(-1, 2)
        cd = ev.cd[:3 * ni].cpu().numpy().reshape(-1, 3)
        gt = ev.gt[:ng].cpu().numpy()
        return {"score": rows[:, 0].copy(), "label": rows[:, 1].copy(), "tp": tp, "cd": cd, "gt": gt}

    def end_eval_table(self, image_size, with_record: bool = False):
        """end_eval + metrics.table_from_stats without the bulk copy: the same header read and the same raises, then the AP / CD table is
        computed on the record where it lies (csrc/evaltable.hip, metrics.table_on_device) and 2064 doubles come back.  -> the table's
        dict plus "per_class" [n_classes, 7] (class, n_gt, n_pred, precision, recall, AP, F1 at IoU 0.5); predictions of equal score
        rank in record order.  with_record: -> (table, the dict end_eval would have returned).  Raises RuntimeError on a class label
        outside the label range 0 .. 255."""
        from .metrics import table_on_device
        ev, nr, ni, ng = self._close_eval("end_eval_table")
        table = table_on_device(ev.rows, ev.tp, nr, ev.cd, ni, ev.gt, ng, image_size)
        return (table, self._record_to_host(ev, nr, ni, ng)) if with_record else table

    @torch.no_grad()
    def eval_losses(self, batch: Dict[str, torch.Tensor], teacher_labels: Optional[List[tuple]] = None):
        """-> (reg, cls, kd_sum) python floats of one validation batch (eval-mode student; validate() upstream,
        src/optimization/train_methods.py:1135-1150: the sums over the step module's loss lists).  teacher_labels: as step_body."""
        self.student.refresh()
        out = self.step_body(batch, None, teacher_labels=teacher_labels, train=False)
        return out["reg"].item(), out["cls"].item(), out["kd"].sum().item()

    def check_overflow(self):
        ev = self._eval
        if ev is not None and int(ev.overflow.item()):
            raise RuntimeError(ev.capacity_message())
        if int(self.overflow.item()):
            raise RuntimeError("pseudo-label capacity exceeded (cfg cand_cap = %d rows / max_boxes = %d per image; 0 = unlimited)"
                               % (self.cfg.cand_cap, self.cfg.max_boxes))
