"""Explicit forward / backward schedule of one EfficientDet on the HIP kernels (no autograd, no tracing).

The network is static, so the host simply issues the kernel sequence; the whole step is captured in a
hipGraph by step.py.  Activations are NHWC fp32 "rows" [B*H*W, C].  A conv's BatchNorm+swish is not
materialised: the conv writes its raw output z plus per-channel sums, `bn_finalize` turns the sums
into (scale, shift), and every CONSUMER applies act(z*scale+shift) while staging its input
(kernel prologue).  Only narrow tensors (MBConv block outputs, BiFPN node outputs) are materialised.

Reference schedule being restated: YetAnotherEfficientDet.forward (src/YetAnotherEfficientDet.py:662-685),
EfficientNet tap wrapper (:550-572), MBConvBlock.forward (src/YetAnotherEfficientNet.py:450-485),
BiFPN._forward_fast_attention (:320-392), Regressor/Classifier.forward (:463-532); the backward is
what autograd derives for them.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import threading
from dataclasses import dataclass, field
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch

from . import _lib
from .arch import NetSpec, BN_EPS, BN_MOMENTUM, pyramid_sizes
from .pyramid import Pyramid
from .store import ParamStore, Arena

NONE, SWISH, SIGMOID = 0, 1, 2

_PACK = threading.local()      # .on: this thread is inside a pack forward (Net.forward(pack=...))
_SKIP = threading.local()      # .on: this thread is inside Net._wgrad_stream() under MMD_DEV_SKIP_WG: call() launches nothing
# entry points a pack forward may issue WITHOUT the group descriptor: they read no per-net parameters (or, the stems, are issued once per net)
PACK_PLAIN_OK = frozenset({"mmd_stem_conv_fwd", "mmd_maxpool_same_fwd", "mmd_memset_async"})


def call(name: str, *args):
    """_lib.call, except inside a pack forward: there every launch that reads parameters must go through Net._c (group descriptor set,
    honoured by the library or refused) - a plain launch would evaluate every net's images with the first net's weights, silently."""
    if getattr(_SKIP, "on", False):
        return 0
    if getattr(_PACK, "on", False) and name not in PACK_PLAIN_OK:
        raise RuntimeError(f"{name} issued inside a pack forward without the group descriptor (engine.Net._c): it would read net 0's parameters for every image")
    return _lib.call(name, *args)


class WgLayer(ctypes.Structure):
    """MmdWgradLayer of include/mmdistill.h: one 1x1-conv weight gradient of the grouped launch (csrc/pw_wgrad_grouped.hip)."""
    _fields_ = [("dy", ctypes.c_void_p), ("x", ctypes.c_void_p), ("dw", ctypes.c_void_p), ("in_scale", ctypes.c_void_p),
                ("in_shift", ctypes.c_void_p), ("gate", ctypes.c_void_p), ("M", ctypes.c_int), ("K", ctypes.c_int), ("N", ctypes.c_int),
                ("in_act", ctypes.c_int), ("rows_per_image", ctypes.c_int), ("mchunk", ctypes.c_int), ("nsplit", ctypes.c_int),
                ("ntn", ctypes.c_int), ("ntk", ctypes.c_int), ("item0", ctypes.c_int), ("tile0", ctypes.c_int), ("pad_", ctypes.c_int),
                ("ws_off", ctypes.c_longlong)]


# 1x1-conv weight gradients are recorded and run as ONE persistent launch + a deterministic fold per WG_CHUNK recorded layers (round 1 ran
# one launch per layer on the weight-gradient stream, fp32 atomics).  The OTHER leaves (depthwise / squeeze-excite / fusion-weight / bias
# gradients) fork off the main chain where they arise: small and latency-bound, they fill the main chain's gaps - deferring them to the
# segment end as well measured 20.8-22.1 ms/step against 20.5.
# D2 records 99 layers per backward: 60 (round 2) = two launches, the second - every backbone layer below block 19 - alone at the very end
# of the backward (0.93 ms exposed); 45 = three, the last one only blocks 4..0 + stem while the second overlaps the high-resolution blocks'
# main chain (round 3, medians 16.65 -> 16.47 ms/step; 50: 16.70 / 16.82, 80: 16.99 / 17.01; round 2: 30 / 15 layers 20.5 / 20.8 vs 19.7 for 60).
# Round 4 (alternating runs, four rounds): 45: 15.02 - 15.08, 46: 15.17 - 15.25, 47: 14.87 - 14.94, 48 / 49: 14.97 - 15.01 ms/step - the last
# flush is the step's exposed tail (rocprofv3: ~0.45 ms behind the main chain's last kernel at 45), 47 leaves it the two 256^2 project convs
# only; D4 and the bf16 modes do not care
WG_CHUNK = 47
WG_ROWS = 4096        # rows per item: 4096 x (64x64 tile) measured best (1.33 ms per step vs 2.58 at 256)
# grid cap of a flush.  A thinner persistent grid for the flushes that run BESIDE the main chain (whose kernels they starve of CU slots: the two
# M131072 K24 N144 input-gradient GEMMs 380 us apiece there against 77 alone) only made it worse - 4096 / 1024 / 512 / 256 / 128 blocks ->
# 16.34 / 16.33 / 16.45 / 16.96 / 18.47 ms/step: the chip is full there, the window's work is conserved (profiles/r04_notes.md)
WG_BLOCKS = 4096


class Live(NamedTuple):
    """A train-mode BatchNorm whose coefficients forward consumers derive on the fly from the batch sums, in the order they take them (`*live`)."""
    stats: torch.Tensor; gamma: torch.Tensor; beta: torch.Tensor; count: int       # (stats: [2C] double raw sums)


@dataclass
class Feat:
    """rows [B*H*W, C] plus the pending per-channel transform consumers must apply."""
    z: torch.Tensor
    B: int
    H: int
    W: int
    C: int
    scale: Optional[torch.Tensor] = None
    shift: Optional[torch.Tensor] = None
    act: int = NONE
    bn: Optional[Live] = None      # train-mode forward: the BatchNorm is still live (scale / shift are filled at the end of the forward)

    @property
    def M(self) -> int:
        return self.B * self.H * self.W


class GradSlot:
    """Gradient w.r.t. one activation tensor, accumulated over its consumers.  `remaining` counts the contributions still to come (the
    train forward counted the consumers); the kernel that writes the LAST one also produces the backward sums of the BatchNorm whose
    output the tensor is (`sums`, valid when `have_sums`), so that BatchNorm needs no reduce launch of its own."""
    def __init__(self, remaining: int = 0):
        self.t: Optional[torch.Tensor] = None
        self.remaining = remaining
        self.sums: Optional[torch.Tensor] = None
        self.have_sums = False
        self.linear_ok = True          # linear-sum mode (a tensor that is max-pooled somewhere): every contribution so far added its share
        self.stream: Optional[int] = None   # linear mode: the stream every contribution must be issued on (see Net._contrib)


class Aff(NamedTuple):
    """A train-mode BatchNorm's finalized coefficients, in the order every BatchNorm-backward entry point takes them (`*aff`)."""
    scale: Optional[torch.Tensor]; shift: Optional[torch.Tensor]; mean: Optional[torch.Tensor]; invstd: Optional[torch.Tensor]


class BnOut(NamedTuple):
    """Net._bnout[y]: the tensor y = BN(z) [* mul_b[image]] (+ skip) is the output of this train-mode BatchNorm over C channels."""
    z: torch.Tensor; mean: torch.Tensor; invstd: torch.Tensor; C: int
    mul_b: Optional[torch.Tensor]; rpi: int                  # (rpi: rows per image, for mul_b)


class BnSums(NamedTuple):
    """Net._contrib's hand-off to the kernel that writes a gradient contribution: take the backward sums of this BatchNorm over it."""
    z: torch.Tensor; mean: torch.Tensor; invstd: torch.Tensor; sums: torch.Tensor
    mul_b: Optional[torch.Tensor]; rpi: int
    linear: int                 # 1: a max-pooled tensor - the kernel adds the sums of its OWN share (see Net._contrib)

    @property
    def quad(self):             # mmd_bifpn_node_* and mmd_maxpool_same_bwd_acc2; mmd_pyr_add_bnsums takes one pointer array per field
        return self.z, self.mean, self.invstd, self.sums

    @property
    def gemm(self):             # GEMM order: mmd_pwconv_bwd_data_bn2* (the sums' slot workspace follows) and mmd_mbconv_expand_bwd_fused
        return self.z, self.mean, self.invstd, self.mul_b, self.rpi, self.sums


NO_SUMS_QUAD = (None, None, None, None)             # what the kernels take in place of BnSums.quad / .gemm: no sums
NO_SUMS_GEMM = (None, None, None, None, 0, None)


class WgRec(NamedTuple):
    """Net._wg_pending: one recorded 1x1-conv weight gradient dw[N,K] (+)= dy^T pro(x) (the arguments of mmd_pwconv_bwd_weight)."""
    dy: torch.Tensor; x: torch.Tensor; dw: torch.Tensor; M: int; K: int; N: int
    in_scale: Optional[torch.Tensor]; in_shift: Optional[torch.Tensor]; in_act: int; gate: Optional[torch.Tensor]; rpi: int


class SeWgRec(NamedTuple):
    """Net._se_wg: the squeeze-excite FC weight gradients of one block, a row of mmd_se_fc_wgrad_batched's table in field order."""
    dpe: torch.Tensor; dpr: torch.Tensor; hpre: torch.Tensor; pooled: torch.Tensor
    g_reduce_w: torch.Tensor; g_reduce_b: torch.Tensor; g_expand_w: torch.Tensor; g_expand_b: torch.Tensor; C: int; S: int


@dataclass
class LazyDz:
    """A BatchNorm backward that is not materialised: the input- and weight-gradient GEMMs of the conv in front of the
    BatchNorm evaluate dz = BnBwd(g, z) in their operand prologues (mmd_pwconv_bwd_data_bn / _weight_bn)."""
    g: torch.Tensor; z: torch.Tensor; aff: Aff; sums: torch.Tensor
    act: int; mul_b: Optional[torch.Tensor]; rpi: int; bn_name: str; count: int


# ---- the tape: what the train forward hands to the backward, one record type per stage (every field has a reader in the backward)
class StemRec(NamedTuple):
    """Tape.stem: the NCHW image, the stem output (BatchNorm-0 + swish pending on it) and that BatchNorm's finalized statistics."""
    x: torch.Tensor; out: Feat; mean: torch.Tensor; invstd: torch.Tensor


class BlockRec(NamedTuple):
    """Tape.blocks[idx]: one MBConv block.  f0 = the depthwise conv's input: the expand conv's output, or `inp` itself (bn0 None) without one."""
    inp: Feat; out: Feat; f0: Feat; bn0: Optional[Aff]; f1: Feat; bn1: Aff
    pooled: torch.Tensor; hpre: torch.Tensor; gate: torch.Tensor                # squeeze-excite: pooled mean, hidden pre-activation, gate
    z2: torch.Tensor; bn2: Aff; rs: Optional[torch.Tensor]                      # project conv's raw output; rs: drop-connect scale per image


class DownRec(NamedTuple):
    """Tape.down[name]: a down-channel conv of the first BiFPN cell; out = BN(z), materialised or (lazy) pending on z."""
    x: Feat; out: Feat; z: torch.Tensor; bn: Aff


class FirstCellRec(NamedTuple):
    """Tape.first: the p5 -> p6 conv's output and its two max-pooled descendants (the first cell's p6 / p7 inputs)."""
    c6: Feat; p6_in: Feat; p7_in: Feat


class NodeRec(NamedTuple):
    """Tape.nodes[cell][i]: a BiFPN node: its operands (None: absent), parameter names, depthwise output zd, raw 1x1 output z, BatchNorm."""
    in0: Feat; in1: Optional[Feat]; up: Optional[Feat]; pl: Optional[Feat]; theta: str; conv: str
    zd: Feat; z: Optional[torch.Tensor]; bn: Optional[Aff]; out: Feat           # (z, bn: None in an eval forward, whose tape nobody reads)


class HeadLayerRec(NamedTuple):
    """One conv_list layer of a head over the pyramid: input rows x, depthwise output zd, raw 1x1 output z; x_off / off = where the
    BatchNorms of x's producer (None: the BiFPN) / of z start in the contiguous BatchNorm arrays."""
    x: torch.Tensor; x_off: Optional[int]; zd: torch.Tensor; z: torch.Tensor; off: int


class HeadRec(NamedTuple):
    """Tape.heads[name]: the layers, the header's input hx (BatchNorms at hx_off) and depthwise output hzd, each level's offset in the output."""
    layers: List[HeadLayerRec]; hx: torch.Tensor; hx_off: int; hzd: torch.Tensor; yoff: List[int]; lev_stride: int


@dataclass
class Tape:
    """Everything the backward reads from the train forward.  begin_step() starts a fresh one; an eval forward fills a throw-away one."""
    stem: Optional[StemRec] = None
    blocks: Dict[int, BlockRec] = field(default_factory=dict)
    down: Dict[str, DownRec] = field(default_factory=dict)
    first: Optional[FirstCellRec] = None
    nodes: List[List[NodeRec]] = field(default_factory=list)       # one list per BiFPN cell, in forward order
    heads: Dict[str, HeadRec] = field(default_factory=dict)
    feats: Optional[List[Feat]] = None                             # the five BiFPN outputs
    A: int = 0                                                     # anchors per image


# MBConv expand convs with a thin input at high resolution (round 4): BatchNorm-0 backward, input gradient and weight gradient in one pass over
# the 6x expanded gradient (csrc/mbconv_bwd_fused.hip) - dz0 is neither stored nor read back, and the layer leaves the grouped weight-gradient
# launch at the exposed end of the backward.  Taken for layers with at least this many rows
MBW_MIN_ROWS = 32768


def pack_nets(nets: List["Net"]) -> bool:
    """Lay the parameter stores of several frozen nets of one body architecture out at a constant stride inside shared buffers, so that
    they can be evaluated as ONE batch with per-group parameters (Net.forward(pack=...), csrc/common.h MmdGroup).  The nets must have been
    built with a common `stem_slot` (their stems may differ in input channels).  -> False when the stores do not line up."""
    p0 = nets[0].ps
    for n in nets[1:]:
        q = n.ps
        if n.trainable or q.n_params != p0.n_params or q.bn_total != p0.bn_total or q.order != p0.order or q.bn_off != p0.bn_off:
            return False
        if any(q.entries[k].off != p0.entries[k].off or (q.entries[k].native != p0.entries[k].native and q.entries[k].kind != "stem") for k in q.order):
            return False
    dev = p0.flat.device
    G = len(nets)
    flat = torch.zeros(G, p0.n_params, device=dev)
    fsc, fsh = torch.zeros(G, p0.bn_total, device=dev), torch.zeros(G, p0.bn_total, device=dev)
    for gi, n in enumerate(nets):
        flat[gi].copy_(n.ps.flat); fsc[gi].copy_(n.ps.fold_scale); fsh[gi].copy_(n.ps.fold_shift)
        n.ps.flat, n.ps.fold_scale, n.ps.fold_shift = flat[gi], fsc[gi], fsh[gi]      # (ParamStore derives every view from these on the fly)
    return True


class Net:
    def __init__(self, spec: NetSpec, device, trainable: bool, arena: Optional[Arena] = None,
                 zarena: Optional[Arena] = None, precision: str = "fp32", stem_slot: int = 0):
        if precision not in ("fp32", "bf16"):
            # ("bf16_hbm", bf16 STORAGE of the wide MBConv tensors, was deleted in round 6 together with its second library build: measured no
            # faster than "bf16" for three rounds - D4 / 768^2: 53.7 vs 53.6, 50.5 vs 49.2, 48.8 vs 48.4 ms/step - DESIGN.md section 5)
            raise ValueError(f"Unsupported precision {precision}")
        # "bf16" = mixed precision: the 1x1-conv GEMMs (forward, input- and weight-gradient) feed the bf16 MFMA, fp32
        # accumulate; tensors in HBM, depthwise convs, BatchNorm statistics, losses and Adam stay fp32
        self.precision = precision
        self._sfx = "_bf16" if self.precision == "bf16" else ""
        self.spec = spec
        self.device = device
        self.trainable = trainable
        self.ps = ParamStore(spec, device, with_grads=trainable, stem_slot=stem_slot)
        # grouped frozen nets (round 4, csrc/common.h MmdGroup): during a pack forward (n_groups, images_per_group, w_stride, bn_stride) -
        # every supported launch then covers the same layer of all the pack's nets, each workgroup reading its own net's parameters
        self._grp: Optional[tuple] = None
        self.arena = arena or Arena(device)
        self.zarena = zarena or Arena(device, 64 << 20, zero_new=True)       # per-step accumulators, zeroed in one memset
        self.bn_momentum = BN_MOMENTUM
        n = self.ps.bn_total
        if trainable:
            self.t_scale = torch.zeros(n, device=device)
            self.t_shift = torch.zeros(n, device=device)
            self.t_mean = torch.zeros(n, device=device)
            self.t_invstd = torch.zeros(n, device=device)
            self.stats_flat = torch.zeros(2 * n, dtype=torch.float64, device=device)
            lo = torch.zeros(n, dtype=torch.int32)
            lc = torch.zeros(n, dtype=torch.int32)
            for name in self.ps.bn_names:
                o, c = self.ps.bn_off[name], self.ps.bn_c[name]
                lo[o:o + c] = o
                lc[o:o + c] = c
            self.bn_layer_off = lo.to(device)
            self.bn_layer_c = lc.to(device)
            self.bn_count_host = torch.zeros(n, dtype=torch.float32)
            self.bn_count = torch.zeros(n, dtype=torch.float32, device=device)
            self._bn_count_key = None
            descs, tiles = [], 0
            for key in self.ps.wt_off:
                e = self.ps.entries[key]
                R, C = e.native
                descs.append([e.off, self.ps.wt_off[key], R, C, tiles])
                tiles += ((R + 31) // 32) * ((C + 31) // 32)
            self.wt_desc = torch.tensor(descs, dtype=torch.int64, device=device)
            self.wt_tiles = tiles
        self.tape = Tape()
        self._slab_floats: Dict[tuple, int] = {}
        self._wg_read_done = None
        self._anchors: Dict[int, torch.Tensor] = {}
        self._side = None
        self._wg = None           # weight-gradient stream: nothing downstream of a wgrad until the optimizer
        self.mark_block, self.mark_event = -1, None
        self._wg_pending: List[WgRec] = []   # deferred 1x1-conv weight gradients of the current backward segment
        self._wg_count = 0                   # layers recorded so far in this backward
        self._wg_plans: Dict[tuple, dict] = {}  # (segment index, operand signature) -> planned table (built once: arena addresses repeat every step)
        self._wg_segment = 0
        self._linear: set = set()              # train forward: tensors that are a BiFPN node's POOLED operand (their gradient is scattered: linear sums)
        self._uses: Dict[int, int] = {}        # train forward: tensor -> number of gradient contributions its slot will receive
        self._bnout: Dict[int, BnOut] = {}     # train forward: tensor y = BN(z) [* mul_b[image]] (+ skip) -> that BatchNorm
        self._counting = False
        self._theta_desc: Dict[tuple, torch.Tensor] = {}
        self._se_wg: List[SeWgRec] = []        # squeeze-excite FC weight gradients of the current backward segment (one batched launch)
        self._se_wg_tabs: Dict[tuple, torch.Tensor] = {}
        # test aid ("teacher forcing"): probe = dict that receives a copy of every materialised unit output of a forward (stem, MBConv
        # blocks, BiFPN down-channel convs and nodes); force_out = dict name -> rows [M, C] written over that output AFTER the probe, so the
        # next unit consumes the given tensor instead of this net's own (tests/test_gpu_net.py::test_teacher_forced_units_bf16)
        self.probe: Optional[Dict[str, torch.Tensor]] = None
        self.force_out: Optional[Dict[str, torch.Tensor]] = None
        self._lazy = False                     # this forward runs the BiFPN with lazy (consumer-applied) BatchNorms

    def _tf(self, name: str, t: torch.Tensor):
        if self.probe is not None:
            self.probe[name] = t.clone()
        if self.force_out is not None and name in self.force_out:
            t.copy_(self.force_out[name].view_as(t))

    def _use(self, f: "Feat"):
        if self._counting:
            k = f.z.data_ptr()
            self._uses[k] = self._uses.get(k, 0) + 1

    def _c(self, name: str, *args):
        """call() for the frozen-forward entry points that honour the group mode: inside a pack forward the group is set around the launch."""
        if self._grp is None:
            return call(name, *args)
        dll = _lib.LIB.load()
        if dll.mmd_set_group(*self._grp) != 0:
            raise RuntimeError("mmd_set_group refused %r" % (self._grp,))
        ok = False
        try:
            rc = _lib.call(name, *args)
            ok = True
        finally:
            # -22 from the clearing call: no launch read the descriptor, i.e. `name` has no group mode and ran with net 0's parameters
            if dll.mmd_set_group(1, 0, 0, 0) != 0 and ok:
                raise RuntimeError(f"{name} does not honour the group descriptor (csrc/common.h MmdGroup): refused inside a pack forward")
        return rc

    # ------------------------------------------------------------------ parameters
    def load_state(self, state):
        self.ps.load_state(state)
        self.refresh()

    def refresh(self):
        """Recompute derived buffers after parameters changed: eval-BN fold and transposed 1x1 weights."""
        ps = self.ps
        if not ps.flat.is_cuda:
            return            # host-side construction (state-dict plumbing, CPU tests): nothing to derive yet
        call("mmd_bn_fold", ps.flat[ps.gamma_off:ps.gamma_off + ps.bn_total], ps.flat[ps.beta_off:ps.beta_off + ps.bn_total],
             ps.rmean, ps.rvar, BN_EPS, ps.fold_scale, ps.fold_shift, ps.bn_total)
        if self.trainable:
            self.refresh_wt()

    def refresh_wt(self):
        ps = self.ps
        call("mmd_transpose_batched", ps.flat, ps.wt, self.wt_desc, self.wt_desc.shape[0], self.wt_tiles)

    # ------------------------------------------------------------------ small helpers
    def _alloc(self, *shape):
        return self.arena.alloc(shape)

    def _zalloc(self, shape, dtype=torch.float32):
        return self.zarena.alloc(shape, dtype)

    def begin_step(self):
        """Reset the bump arenas and zero the accumulator arena (one memset for all per-step sums)."""
        self.arena.reset()
        self.zarena.reset()
        for c in self.zarena.chunks:
            call("mmd_memset_async", c, 0, c.numel())
        if self.trainable:
            call("mmd_memset_async", self.stats_flat, 0, self.stats_flat.numel() * 8)
        self.tape = Tape()

    def _bn_stats(self, name: str, train: bool):
        """Raw-sum accumulator [2C] (double) of BN `name` for this step (train) or None (eval)."""
        if not train:
            return None
        b = self.ps.bn(name)
        o, c = b["off"], b["C"]
        return self.stats_flat[2 * o:2 * o + 2 * c]

    def _bn_aff(self, name: str, train: bool, stats, count: int):
        """-> (Aff, Live or None).  eval: folded running stats.  train: views that the batched finalize
        at the end of the forward fills (the backward reads them) + the Live record forward consumers use."""
        b = self.ps.bn(name)
        if not train:
            return Aff(b["fscale"], b["fshift"], None, None), None
        o, c = b["off"], b["C"]
        self.bn_count_host[o:o + c] = float(count)
        return (Aff(self.t_scale[o:o + c], self.t_shift[o:o + c], self.t_mean[o:o + c], self.t_invstd[o:o + c]),
                Live(stats, b["gamma"], b["beta"], int(count)))

    @staticmethod
    def _xf(x: Feat):
        """prologue arguments (scale, shift, act, stats, gamma, beta, count) of a forward consumer of x"""
        if x.bn is not None:
            return (None, None, x.act, *x.bn)
        return (x.scale, x.shift, x.act, None, None, None, 0)

    STATS_SLOTS = 64
    # frozen nets: a BiFPN node (fusion, depthwise, 1x1 conv, BN) in one kernel where _node_fusable() says so.  A test aid, not a switch:
    # tests/test_gpu_net.py turns it off on its nets to send a D2 pack forward through the two-launch node path
    FUSE_NODE = True
    # widths above 160 (D4's 224): the whole-node kernel holds two 8x8-pixel tiles in 157 KB of LDS (one block per CU) and reads its 1x1
    # weights from L2 - a win on the latency-bound small maps, a loss on the large ones, where the two-launch path runs a chip-filling GEMM
    # (round 4, D4 / 768^2 at B = 8: every level fused 56.7 ms/step against 54.0 unfused)
    NODE_FUSE_WIDE_MAXROWS = 1152      # (neutral there: fewer launches, same time; 4608: +0.4 ms; every level: +2.7 ms)

    def _node_fusable(self, in0: "Feat") -> bool:
        if not self.ps.flat.is_cuda or _lib.LIB.load().mmd_bifpn_node_fused_supported(in0.C) != 1:
            return False
        return in0.C <= 160 or in0.M <= self.NODE_FUSE_WIDE_MAXROWS

    def _stats_ws(self, stats, M: int, C: int):
        """(workspace, slots) for a BatchNorm-sum producer over M rows: the thin full-resolution layers would send
        thousands of same-address f64 atomics (memory-side, ~17 ns each) to 2C addresses; the kernels spread them over
        `slots` zeroed copies and fold.  Only worth a buffer when M is large (the C side decides whether to use it)."""
        if stats is None or M < 16384:
            return None, 0
        return self._zalloc((self.STATS_SLOTS * 2 * C,), torch.float64), self.STATS_SLOTS

    def _pw(self, x: Feat, wkey: str, N: int, bias=None, stats=None, out_aff=None, out_act=NONE, residual=None,
            gate=None, y=None, ybs=0, yoff=0, plain_in=False):
        M, K = x.M, x.C
        if y is None:
            y = self._alloc(M, N)
        xf = (None, None, NONE, None, None, None, 0) if plain_in else self._xf(x)
        args = (x.z, self.ps.w(wkey), y, M, K, N, *xf, gate, x.H * x.W, bias, out_aff[0] if out_aff else None, out_aff[1] if out_aff else None, out_act,
                residual, stats, ybs, yoff, *self._stats_ws(stats, M, N))
        if self._grp is None and not self._sfx and not plain_in and ybs == 0:
            # (fp32, outside a pack forward, with a producer transform: the launch may take the all-N K-sliced slab kernel, csrc/pw_slab.hip,
            # which needs a workspace for its K slices' partial slabs when the launch has few row slabs)
            call("mmd_pwconv_fwd_form", *args, *self._slab_ws(M, K, N, 0), 0)
        else:
            self._c("mmd_pwconv_fwd" + self._sfx, *args)
        return y

    def _slab_ws(self, M: int, K: int, N: int, bn_operand: int):
        """(workspace, floats) for the K slices of a slab-kernel launch of this shape (mmd_pwconv_slab_ws_floats; (None, 0): the launch runs
        unsliced or on another kernel family).  Plain arena memory: the partial slabs need no zeroing."""
        if not self.ps.flat.is_cuda:
            return None, 0
        key = (M, K, N, bn_operand)
        n = self._slab_floats.get(key)
        if n is None:
            n = self._slab_floats[key] = int(_lib.LIB.load().mmd_pwconv_slab_ws_floats(M, K, N, bn_operand))
        return (self._alloc(n), n) if n > 0 else (None, 0)

    def _dw(self, x: Feat, wkey: str, k: int, s: int, stats=None, out_aff=None, out_act=NONE, pool=None):
        OH, OW = -(-x.H // s), -(-x.W // s)
        y = self._alloc(x.B * OH * OW, x.C)
        args = (x.z, self.ps.w(wkey), y, x.B, x.H, x.W, x.C, k, s, *self._xf(x),
                out_aff[0] if out_aff else None, out_aff[1] if out_aff else None, out_act, stats, pool,
                *self._stats_ws(stats, x.B * OH * OW, x.C))
        self._c("mmd_dwconv_fwd", *args)
        return y, OH, OW

    def anchors(self, image_size: int) -> torch.Tensor:
        """[A,4] (y1,x1,y2,x2) fp32, float64 math then cast (src/YetAnotherEfficientDet.py:116-147)."""
        if image_size not in self._anchors:
            import itertools
            import numpy as np
            scales = np.array([2 ** 0, 2 ** (1.0 / 3.0), 2 ** (2.0 / 3.0)])
            ratios = [(1.0, 1.0), (1.4, 0.7), (0.7, 1.4)]
            allb = []
            for stride in [8, 16, 32, 64, 128]:
                lv = []
                for scale, ratio in itertools.product(scales, ratios):
                    base = self.spec.anchor_scale * stride * scale
                    ax, ay = base * ratio[0] / 2.0, base * ratio[1] / 2.0
                    x = np.arange(stride / 2, image_size, stride)
                    xv, yv = np.meshgrid(x, x)
                    xv, yv = xv.reshape(-1), yv.reshape(-1)
                    b = np.vstack((yv - ay, xv - ax, yv + ay, xv + ax)).swapaxes(0, 1)
                    lv.append(np.expand_dims(b, 1))
                allb.append(np.concatenate(lv, axis=1).reshape(-1, 4))
            self._anchors[image_size] = torch.from_numpy(
                np.ascontiguousarray(np.vstack(allb).astype(np.float32))).contiguous().to(self.device)
        return self._anchors[image_size]

    # ------------------------------------------------------------------ forward
    def forward(self, x, train: bool = False, drop_scale: Optional[torch.Tensor] = None,
                raw_logits: bool = False, pack: Optional[list] = None):
        """x: [B,Cin,S,S] NCHW fp32 on device.  drop_scale: [n_skip_blocks, B] = mask/keep (train only).
        Returns cls [B,A,NC] (probabilities; pre-sigmoid logits with raw_logits=True, a calibration aid), reg [B,A,4],
        features: list of 5 Feat (NHWC rows)."""
        if train and not self.trainable:
            raise RuntimeError("train-mode forward on a frozen (teacher) net")
        spec, ps = self.spec, self.ps
        if pack is not None:
            # pack forward: `pack` = the frozen nets evaluated together (this one first), x = their inputs [Bg, Cin_g, S, S] in the same order.
            # Everything behind the stems runs ONCE over the G x Bg images with per-group parameters (pack_nets laid the stores out alike)
            assert not train and pack[0] is self and len(pack) == len(x) and len(pack) > 1
            Bg, S = x[0].shape[0], x[0].shape[2]
            assert all(xi.shape[0] == Bg and xi.shape[2] == S for xi in x)
            self._grp = (len(pack), Bg, ps.n_params, ps.bn_total)
            _PACK.on = True
            try:
                return self._forward(x, train, drop_scale, raw_logits, pack)
            finally:
                self._grp = None
                _PACK.on = False
        return self._forward(x, train, drop_scale, raw_logits, None)

    def _forward(self, x, train, drop_scale, raw_logits, pack):
        tape = self.tape if train else Tape()
        self._counting = train
        if train:
            self._uses, self._bnout, self._linear = {}, {}, set()
        stem = self._forward_stem(x, train, pack, tape)
        taps = self._forward_blocks(stem, train, drop_scale, tape)
        feats = self._bifpn(taps, train, tape)
        cls, reg = self._forward_heads(feats, train, raw_logits, tape)
        if train:
            self._counting = False
            self._finalize_bn((stem.B, x.shape[2]))
        return cls, reg, feats

    def _forward_stem(self, x, train: bool, pack, tape: Tape) -> Feat:
        """Direct 3x3/s2 stem conv (NCHW image -> NHWC rows); the im2col matrix is only built in the backward, for the weight gradient, on
        the wgrad stream.  x: the image batch; in a pack forward one batch per net."""
        spec, ps, P = self.spec, self.ps, "backbone_net.model"
        B, S = (x[0].shape[0] * len(pack), x[0].shape[2]) if pack is not None else (x.shape[0], x.shape[2])
        OH = (S + 1) // 2
        z = self._alloc(B * OH * OH, spec.stem_out)
        if pack is not None:
            # the stems differ (input channels): one launch per net, each writing its images' rows of the shared stem output
            Bg, rows = x[0].shape[0], x[0].shape[0] * OH * OH
            for gi, (net, xg) in enumerate(zip(pack, x)):
                b0 = net.ps.bn(f"{P}._bn0")
                call("mmd_stem_conv_fwd", xg, net.ps.w(f"{P}._conv_stem.conv.weight"), z[gi * rows:(gi + 1) * rows], Bg, xg.shape[1], S, S,
                     net.ps.stem_kp, spec.stem_out, b0["fscale"], b0["fshift"], SWISH, None, None, 0)
            return Feat(z, B, OH, OH, spec.stem_out)
        Cin, wstem = x.shape[1], ps.w(f"{P}._conv_stem.conv.weight")
        if train:
            st = self._bn_stats(f"{P}._bn0", True)
            a, live = self._bn_aff(f"{P}._bn0", True, st, B * OH * OH)
            call("mmd_stem_conv_fwd", x, wstem, z, B, Cin, S, S, ps.stem_kp, spec.stem_out, None, None, NONE, st,
                 *self._stats_ws(st, B * OH * OH, spec.stem_out))
            out = Feat(z, B, OH, OH, spec.stem_out, a.scale, a.shift, SWISH, live)
            tape.stem = StemRec(x, out, a.mean, a.invstd)
            return out
        # frozen net: the folded BN + swish ride in the producer's epilogue (once per element) instead of the depthwise
        # prologue, which would redo them for every halo pixel (1.6x for 3x3, 2.25x for 5x5 tiles)
        b0 = ps.bn(f"{P}._bn0")
        call("mmd_stem_conv_fwd", x, wstem, z, B, Cin, S, S, ps.stem_kp, spec.stem_out, b0["fscale"], b0["fshift"], SWISH, None, None, 0)
        self._tf("stem", z)
        return Feat(z, B, OH, OH, spec.stem_out)

    def _forward_blocks(self, cur: Feat, train: bool, drop_scale, tape: Tape) -> List[Feat]:
        """The MBConv blocks in order -> the tapped block outputs (the BiFPN's inputs)."""
        taps: List[Feat] = []
        skip_i = 0
        for blk in self.spec.blocks:
            inp = cur
            self._use(inp)                  # the block's own path ...
            if blk.skip:
                self._use(inp)              # ... and the identity skip
            if train:
                rs = drop_scale[skip_i] if blk.skip and blk.drop_rate and drop_scale is not None else None
                rec = tape.blocks[blk.idx] = self._block_fwd_train(blk, inp, rs)
                cur = rec.out
            else:
                cur = self._block_fwd_frozen(blk, inp)
            if blk.skip:
                skip_i += 1
            if blk.idx == self.mark_block and self.ps.flat.is_cuda:
                self.mark_event = torch.cuda.current_stream().record_event()      # "this net is past block k" (step.py staggers the teachers on it)
            self._tf(f"blk{blk.idx}", cur.z)
            if blk.idx in self.spec.taps:
                taps.append(cur)
        return taps

    def _se_bufs(self, blk, q: str, B: int, pooled_dtype):
        """What the two regimes of a block share -> (pooled, hpre, gate, squeeze-excite FC parameters).  Each calls it BEHIND its expand conv,
        where these allocations have always stood: the arenas hand out addresses in call order."""
        ps = self.ps
        pooled = self._zalloc((B, blk.cmid), pooled_dtype)
        hpre = self._alloc(B, blk.se)
        gate = self._alloc(B, blk.cmid)
        return pooled, hpre, gate, (ps.w(f"{q}._se_reduce.conv.weight"), ps.w(f"{q}._se_reduce.conv.bias"),
                                    ps.w(f"{q}._se_expand.conv.weight"), ps.w(f"{q}._se_expand.conv.bias"))

    def _block_fwd_train(self, blk, inp: Feat, rs: Optional[torch.Tensor]) -> BlockRec:
        """One MBConv block in train mode: every conv writes its raw output + BatchNorm sums, its consumer applies the live BatchNorm + swish;
        only the block output is materialised (BatchNorm-2 [* rs per image] + skip in one mmd_affine_act)."""
        ps, q, B = self.ps, f"backbone_net.model._blocks.{blk.idx}", inp.B
        f0, a0 = inp, None
        if blk.expand != 1:
            st0 = self._bn_stats(f"{q}._bn0", True)
            a0, live0 = self._bn_aff(f"{q}._bn0", True, st0, inp.M)
            z0 = self._pw(inp, f"{q}._expand_conv.conv.weight", blk.cmid, stats=st0)
            f0 = Feat(z0, B, inp.H, inp.W, blk.cmid, a0.scale, a0.shift, SWISH, live0)
        pooled, hpre, gate, se_w = self._se_bufs(blk, q, B, torch.float32)
        st1 = self._bn_stats(f"{q}._bn1", True)
        z1, H1, W1 = self._dw(f0, f"{q}._depthwise_conv.conv.weight", blk.kernel, blk.stride, stats=st1)
        M1 = B * H1 * W1
        a1, live1 = self._bn_aff(f"{q}._bn1", True, st1, M1)
        f1 = Feat(z1, B, H1, W1, blk.cmid, a1.scale, a1.shift, SWISH, live1)
        call("mmd_chan_pool", z1, None, None, *live1, SWISH, None, pooled, 1.0 / (H1 * W1), B, H1 * W1, blk.cmid)
        call("mmd_se_fc_fwd", pooled, *se_w, hpre, gate, B, blk.cmid, blk.se)
        st2 = self._bn_stats(f"{q}._bn2", True)
        z2 = self._pw(f1, f"{q}._project_conv.conv.weight", blk.cout, stats=st2, gate=gate)
        a2, live2 = self._bn_aff(f"{q}._bn2", True, st2, M1)
        y = self._alloc(M1, blk.cout)
        call("mmd_affine_act", z2, None, None, *live2, NONE, rs, H1 * W1, inp.z if blk.skip else None, y, M1, blk.cout)
        self._bnout[y.data_ptr()] = BnOut(z2, a2.mean, a2.invstd, blk.cout, rs, H1 * W1)
        return BlockRec(inp=inp, out=Feat(y, B, H1, W1, blk.cout), f0=f0, bn0=a0, f1=f1, bn1=a1, pooled=pooled, hpre=hpre, gate=gate,
                        z2=z2, bn2=a2, rs=rs)

    def _block_fwd_frozen(self, blk, inp: Feat) -> Feat:
        """One MBConv block of a frozen net (alone or in a pack): the folded BatchNorms + swish ride in the producers' epilogues (see the
        stem), BN1 + swish and the squeeze-excite average pool in the depthwise epilogue (no separate pool pass)."""
        ps, q, B = self.ps, f"backbone_net.model._blocks.{blk.idx}", inp.B

        def bn(i):                  # folded (scale, shift) of the block's BatchNorm i
            b = ps.bn(f"{q}._bn{i}")
            return b["fscale"], b["fshift"]

        wexp, wdw = f"{q}._expand_conv.conv.weight", f"{q}._depthwise_conv.conv.weight"
        H1, W1 = -(-inp.H // blk.stride), -(-inp.W // blk.stride)
        # thin input: expand + depthwise in one kernel below, the expanded tensor stays in LDS
        fused_front = (blk.expand != 1 and ps.flat.is_cuda
                       and _lib.LIB.load().mmd_mbconv_expand_dw_supported(inp.C, blk.cmid, blk.kernel, blk.stride) == 1)
        f0 = inp
        if blk.expand != 1 and not fused_front:
            f0 = Feat(self._pw(inp, wexp, blk.cmid, out_aff=bn(0), out_act=SWISH), B, inp.H, inp.W, blk.cmid)
        # (pooled: Q36 fixed-point integer sums - bit-reproducible whatever order the blocks' atomics arrive in, csrc/common.h mmd_pool_add)
        pooled, hpre, gate, se_w = self._se_bufs(blk, q, B, torch.int64)
        if fused_front:
            a1v = self._alloc(B * H1 * W1, blk.cmid)
            self._c("mmd_mbconv_expand_dw_fwd", inp.z, ps.w(wexp), *bn(0), ps.w(wdw), *bn(1), a1v, pooled, B, inp.H, inp.W, inp.C,
                    blk.cmid, blk.kernel, blk.stride)
        else:
            a1v, _, _ = self._dw(f0, wdw, blk.kernel, blk.stride, out_aff=bn(1), out_act=SWISH, pool=pooled)
        self._c("mmd_se_fc_fwd_q", pooled, *se_w, hpre, gate, B, blk.cmid, blk.se)
        y = self._pw(Feat(a1v, B, H1, W1, blk.cmid), f"{q}._project_conv.conv.weight", blk.cout, gate=gate, out_aff=bn(2),
                     residual=inp.z if blk.skip else None)
        return Feat(y, B, H1, W1, blk.cout)

    def _forward_heads(self, feats: List[Feat], train: bool, raw_logits: bool, tape: Tape):
        """Regressor, then classifier, over the pyramid row buffer the last BiFPN cell wrote -> (cls [B,A,NC], reg [B,A,4])."""
        spec, B = self.spec, feats[0].B
        for f in feats:
            self._use(f)                    # one contribution: heads' input gradients (+ the MTA loss' feature gradient) in one launch
        A = sum(f.H * f.W for f in feats) * spec.num_anchors
        reg = self._alloc(B, A, 4)
        cls = self._alloc(B, A, spec.num_classes)
        self._head("regressor", feats, 4, reg, A, NONE, train, tape)
        self._head("classifier", feats, spec.num_classes, cls, A, NONE if raw_logits else SIGMOID, train, tape)
        tape.feats, tape.A = feats, A
        return cls, reg

    def _finalize_bn(self, key: tuple):
        """Every BN layer finalized in one launch: running stats + (scale, shift, mean, invstd) for the backward.  key = (B, S): the
        per-layer row counts the forward noted in bn_count_host are uploaded when it changes."""
        ps = self.ps
        if self._bn_count_key != key:
            self.bn_count.copy_(self.bn_count_host)
            self._bn_count_key = key
        call("mmd_bn_finalize_all", self.stats_flat, self.bn_count, self.bn_layer_off, self.bn_layer_c,
             ps.flat[ps.gamma_off:ps.gamma_off + ps.bn_total], ps.flat[ps.beta_off:ps.beta_off + ps.bn_total],
             ps.rmean, ps.rvar, float(self.bn_momentum), BN_EPS, self.t_scale, self.t_shift, self.t_mean,
             self.t_invstd, ps.bn_total, ps.nbt, ps.nbt.numel())      # (+ num_batches_tracked += 1 for every BN, in the same launch)

    def _sep_bn(self, name: str, zdf: Feat, train: bool, y=None):
        """The 1x1 conv + BatchNorm of a SeparableConvBlock(norm=True, activation=False) on its depthwise output zdf
        -> (materialised output, raw conv output z, Aff); z and Aff are None in eval, where the folded BatchNorm rides in the conv's epilogue."""
        ps, W, M = self.ps, zdf.C, zdf.M
        bias = ps.w(f"{name}.pointwise_conv.conv.bias")
        if not train:
            b = ps.bn(f"{name}.bn")
            y = self._pw(zdf, f"{name}.pointwise_conv.conv.weight", W, bias=bias, out_aff=(b["fscale"], b["fshift"]), y=y)
            return Feat(y, zdf.B, zdf.H, zdf.W, W), None, None
        st = self._bn_stats(f"{name}.bn", True)
        z = self._pw(zdf, f"{name}.pointwise_conv.conv.weight", W, bias=bias, stats=st)
        a, live = self._bn_aff(f"{name}.bn", True, st, M)
        if y is None:
            y = self._alloc(M, W)
        call("mmd_affine_act", z, None, None, *live, NONE, None, 0, None, y, M, W)
        self._bnout[y.data_ptr()] = BnOut(z, a.mean, a.invstd, W, None, 0)
        return Feat(y, zdf.B, zdf.H, zdf.W, W), z, a

    def _down_channel(self, name: str, x: Feat, train: bool, tape: Tape, lazy: bool = False) -> Feat:
        ps, W = self.ps, self.spec.fpn_w
        bias = ps.w(f"{name}.0.conv.bias")
        if not train:
            b = ps.bn(f"{name}.1")
            out = Feat(self._pw(x, f"{name}.0.conv.weight", W, bias=bias, out_aff=(b["fscale"], b["fshift"])), x.B, x.H, x.W, W)
        else:
            st = self._bn_stats(f"{name}.1", True)
            z = self._pw(x, f"{name}.0.conv.weight", W, bias=bias, stats=st)
            a, live = self._bn_aff(f"{name}.1", True, st, x.M)
            if lazy:
                # lazy output: the raw conv output + its BatchNorm as a pending transform the consuming node kernels apply (no affine launch)
                out = Feat(z, x.B, x.H, x.W, W, a.scale, a.shift, NONE, live)
            else:
                y = self._alloc(x.M, W)
                call("mmd_affine_act", z, None, None, *live, NONE, None, 0, None, y, x.M, W)
                out = Feat(y, x.B, x.H, x.W, W)
            self._use(x)
            self._bnout[out.z.data_ptr()] = BnOut(z, a.mean, a.invstd, W, None, 0)
            tape.down[name] = DownRec(x, out, z, a)
        self._tf(name, out.z)       # (does nothing to a lazy output: lazy forwards run without the test hooks, see _bifpn)
        return out

    def _pool(self, x: Feat) -> Feat:
        OH, OW = (x.H + 1) // 2, (x.W + 1) // 2
        y = self._alloc(x.B * OH * OW, x.C)
        call("mmd_maxpool_same_fwd", x.z, y, x.B, x.H, x.W, x.C)
        self._use(x)
        return Feat(y, x.B, OH, OW, x.C)

    def _node(self, cell: str, conv: str, theta: str, in0: Feat, in1: Optional[Feat], up: Optional[Feat],
              pl: Optional[Feat], train: bool, tape: Tape, y=None) -> Feat:
        """One BiFPN node: fast-attention fusion of its operands (in0, same-resolution in1, upsampled `up`, max-pooled `pl`), depthwise 3x3,
        1x1 conv, BatchNorm.  y: the rows to write a materialised output to (the last cell's pyramid row buffer)."""
        name, th, ops = f"{cell}.{conv}", self.ps.w(f"{cell}.{theta}"), (in0, in1, up, pl)
        if not train and self.FUSE_NODE and self._node_fusable(in0):
            out = self._node_fused_frozen(name, th, ops, y)
        else:
            # (the whole-node train kernel also in the bf16 modes: the node's 1x1 conv then runs exact fp32 products in the forward - closer to
            # the fp32 reference than the mode's operand-rounding rule asks for; its two gradient GEMMs follow the mode)
            if train and self._node_fusable(in0):
                zd, z, a, out = self._node_fused_train(name, th, ops, y)
            else:
                zd, z, a, out = self._node_two_launch(name, th, ops, train, y)
            for operand in ops:
                if operand is not None:
                    self._use(operand)
            if pl is not None and train:
                self._linear.add(pl.z.data_ptr())
            tape.nodes[-1].append(NodeRec(in0, in1, up, pl, theta, conv, zd, z, a, out))
        self._tf(name, out.z)
        return out

    def _node_fused_frozen(self, name: str, th, ops, y) -> Feat:
        """frozen net: fusion + depthwise + 1x1 conv + folded BN in one launch, the depthwise output never leaves the CU"""
        ps, in0 = self.ps, ops[0]
        b = ps.bn(f"{name}.bn")
        if y is None:
            y = self._alloc(in0.M, in0.C)
        self._c("mmd_bifpn_node_fwd_fused", *[o.z if o is not None else None for o in ops], th,
                ps.w(f"{name}.depthwise_conv.conv.weight"), ps.w(f"{name}.pointwise_conv.conv.weight"),
                ps.w(f"{name}.pointwise_conv.conv.bias"), b["fscale"], b["fshift"], y, in0.B, in0.H, in0.W, in0.C)
        return Feat(y, in0.B, in0.H, in0.W, in0.C)

    def _node_fused_train(self, name: str, th, ops, y):
        """trainable net: fusion + depthwise + 1x1 conv + BatchNorm sums in one launch (raw z out, depthwise output kept for the backward)
        -> (depthwise output, z, Aff, node output)"""
        ps, in0 = self.ps, ops[0]
        W = in0.C
        st = self._bn_stats(f"{name}.bn", True)
        z, zd = self._alloc(in0.M, W), self._alloc(in0.M, W)
        args = (*[o.z if o is not None else None for o in ops], th,
                ps.w(f"{name}.depthwise_conv.conv.weight"), ps.w(f"{name}.pointwise_conv.conv.weight"),
                ps.w(f"{name}.pointwise_conv.conv.bias"), z, zd, st, in0.B, in0.H, in0.W, W)
        lives = [o.bn if o is not None else None for o in ops]          # operands whose BatchNorm is still pending (lazy producers)
        if any(lv is not None for lv in lives):
            assert self._lazy and all(o.act == NONE for o, lv in zip(ops, lives) if lv is not None)
            stats, gamma, beta, count = zip(*[lv if lv is not None else Live(None, None, None, 0) for lv in lives])
            ptrs = lambda col: (ctypes.c_void_p * 4)(*[None if t is None else t.data_ptr() for t in col])
            call("mmd_bifpn_node_fwd_fused_train_lz", *args, ptrs(stats), ptrs(gamma), ptrs(beta), (ctypes.c_longlong * 4)(*count))
        else:
            call("mmd_bifpn_node_fwd_fused_train", *args)
        a, live = self._bn_aff(f"{name}.bn", True, st, in0.M)
        if self._lazy and y is None:
            # lazy output (every cell but the last, whose outputs the heads and the MTA loss read): no affine launch
            out = Feat(z, in0.B, in0.H, in0.W, W, a.scale, a.shift, NONE, live)
        else:
            if y is None:
                y = self._alloc(in0.M, W)
            call("mmd_affine_act", z, None, None, *live, NONE, None, 0, None, y, in0.M, W)
            out = Feat(y, in0.B, in0.H, in0.W, W)
        self._bnout[out.z.data_ptr()] = BnOut(z, a.mean, a.invstd, W, None, 0)
        return Feat(zd, in0.B, in0.H, in0.W, W), z, a, out

    def _node_two_launch(self, name: str, th, ops, train: bool, y):
        """fusion + depthwise in one launch, then the 1x1 conv (train: + BatchNorm sums, and an affine launch) -> as _node_fused_train.
        The fused activation is not materialised: the node's backward launch recomputes it, also for the depthwise weight gradient"""
        in0 = ops[0]
        zd = self._alloc(in0.M, in0.C)
        self._c("mmd_bifpn_node_dw_fwd", *[o.z if o is not None else None for o in ops], th,
                self.ps.w(f"{name}.depthwise_conv.conv.weight"), None, zd, in0.B, in0.H, in0.W, in0.C)
        zdf = Feat(zd, in0.B, in0.H, in0.W, in0.C)
        out, z, a = self._sep_bn(name, zdf, train, y=y)
        return zdf, z, a, out

    def _bifpn(self, taps: List[Feat], train: bool, tape: Tape) -> List[Feat]:
        feats: List[Feat] = list(taps)
        # "lazy" BiFPN operands of the trainable net (round 4): a node's / down-channel conv's train-mode BatchNorm is applied by the CONSUMING
        # node kernels while they load the operand (forward: from the live batch sums; backward: finalized coefficients) instead of by an
        # mmd_affine_act launch behind every producer: 40 launches less on the student's forward chain.  They need every node on the
        # whole-node train kernel (widths <= 160) and no test hooks that read / overwrite materialised outputs
        self._lazy = (train and self.ps.flat.is_cuda and self.probe is None and self.force_out is None and self.spec.fpn_w <= 160
                      and _lib.LIB.load().mmd_bifpn_node_fused_supported(self.spec.fpn_w) == 1)
        lz = self._lazy
        for c in range(self.spec.fpn_cells):
            cell = f"bifpn.{c}"
            tape.nodes.append([])
            if c == 0:
                p3, p4, p5 = feats
                c6 = self._down_channel(f"{cell}.p5_to_p6", p5, train, tape)         # (max-pooled by its own launch: materialised)
                p6_in = self._pool(c6)
                p7_in = self._pool(p6_in)
                p3_in = self._down_channel(f"{cell}.p3_down_channel", p3, train, tape, lazy=lz)
                p4_in = self._down_channel(f"{cell}.p4_down_channel", p4, train, tape, lazy=lz)
                p5_in = self._down_channel(f"{cell}.p5_down_channel", p5, train, tape, lazy=lz)
                tape.first = FirstCellRec(c6, p6_in, p7_in)
            else:
                p3_in, p4_in, p5_in, p6_in, p7_in = feats
            last = c == self.spec.fpn_cells - 1
            if last:    # final outputs land in ONE pyramid row buffer so the shared-weight heads run all levels per launch
                pyr = Pyramid(p3_in.B, [(f.H, f.W) for f in (p3_in, p4_in, p5_in, p6_in, p7_in)])
                fcat = self._alloc_pyr(pyr, p3_in.C, train)
                ov = pyr.levels(fcat)
                self._pyr, self._fcat = pyr, fcat
            else:
                ov = [None] * 5
            p6_up = self._node(cell, "conv6_up", "p6_w1", p6_in, None, p7_in, None, train, tape)
            p5_up = self._node(cell, "conv5_up", "p5_w1", p5_in, None, p6_up, None, train, tape)
            p4_up = self._node(cell, "conv4_up", "p4_w1", p4_in, None, p5_up, None, train, tape)
            p3_out = self._node(cell, "conv3_up", "p3_w1", p3_in, None, p4_up, None, train, tape, y=ov[0])
            if c == 0:
                p4_in = self._down_channel(f"{cell}.p4_down_channel_2", taps[1], train, tape, lazy=lz)
                p5_in = self._down_channel(f"{cell}.p5_down_channel_2", taps[2], train, tape, lazy=lz)
            p4_out = self._node(cell, "conv4_down", "p4_w2", p4_in, p4_up, None, p3_out, train, tape, y=ov[1])
            p5_out = self._node(cell, "conv5_down", "p5_w2", p5_in, p5_up, None, p4_out, train, tape, y=ov[2])
            p6_out = self._node(cell, "conv6_down", "p6_w2", p6_in, p6_up, None, p5_out, train, tape, y=ov[3])
            p7_out = self._node(cell, "conv7_down", "p7_w2", p7_in, None, None, p6_out, train, tape, y=ov[4])
            feats = [p3_out, p4_out, p5_out, p6_out, p7_out]
        return feats

    def _alloc_pyr(self, pyr: Pyramid, C: int, zero_pad: bool = True) -> torch.Tensor:
        """zero_pad=False: a frozen net's tensor - nothing multiplies its padding rows into a sum (no weight gradients, no batch statistics), whatever
        they hold stays in the padding rows of its consumers' outputs (D4 / 768^2, whose 6^2 level is padded: 40 fill launches less on the pack's chain)."""
        t = self._alloc(pyr.total, C)
        if pyr.padded and zero_pad:             # padding rows are multiplied in the weight-gradient GEMMs: they must be zeros, not stale bits
            for l in range(len(pyr.rows)):          # (only the pad rows: a whole-buffer memset per pyramid tensor cost 1.8 ms/step at 768)
                lo, hi = pyr.row0[l] + pyr.rows[l], pyr.row0[l + 1]
                if hi > lo:
                    call("mmd_memset_async", t[lo:hi], 0, (hi - lo) * C * 4)
        return t

    def _head_nsplit(self) -> int:
        """How many leading pyramid levels the heads' pyramid launches cover: all 5 outside a pack forward.
        Pack forward (grouped frozen nets): the pyramid GEMM's 128-row tiles must not straddle two nets' rows, i.e. every level needs
        images_per_group * H * W % 128 == 0.  D4 / 768^2 at B = 8 misses that on the 6 x 6 level only (288 rows per net): the launches
        then cover the leading levels and each trailing level runs as a plain launch of its own - few rows, so the GEMM lands on the
        32-row skinny kernel, whose tiles divide 288 (csrc/pw_gemm.hip pw_dispatch checks the tile height of the kernel it takes)."""
        if self._grp is None:
            return 5
        good = [(self._grp[1] * h * w) % 128 == 0 for h, w in self._pyr.sizes]
        nsplit = good.index(False) if False in good else 5
        if any(good[nsplit:]) or nsplit == 0:
            raise RuntimeError("pack forward: pyramid levels %r at %d images per net do not split into whole-tile and small trailing levels" % (self._pyr.sizes, self._grp[1]))
        return nsplit

    def _head_dw(self, x, cname: str, y, xf: tuple, nsplit: int, lev_stride: int):
        """Depthwise 3x3 of a head layer over pyramid rows x -> y: the leading nsplit levels in one launch, each trailing level in a plain
        launch.  xf = (scale, shift, act, stats, gamma, beta): x's pending transform, level l's coefficients l * lev_stride channels in."""
        pyr, C, w = self._pyr, x.shape[1], self.ps.w(f"{cname}.depthwise_conv.conv.weight")
        self._c("mmd_dwconv3_pyr", x, w, y, pyr.head_desc(nsplit), C, 0, *xf, lev_stride, None, None, None, NONE, None, None, None, None)
        sc, sh, act = xf[:3]
        for l in range(nsplit, 5):
            (h, wd), lo = pyr.sizes[l], l * lev_stride
            self._c("mmd_dwconv_fwd", pyr.level(x, l), w, pyr.level(y, l), pyr.B, h, wd, C, 3, 1, sc[lo:] if sc is not None else None,
                    sh[lo:] if sh is not None else None, act, None, None, None, 0, None, None, NONE, None, None, None, 0)

    def _head_pw(self, x, cname: str, y, N: int, out_act: int, stats, lev_stride: int, nsplit: int, ybs: int = 0, yoff=None):
        """1x1 conv + bias of a head layer over pyramid rows x, split like _head_dw.  yoff None: y is a pyramid row buffer (stats: the
        per-level BatchNorm sums, lev_stride channels apart); else the header: level l's rows go to y[image, yoff[l]:], images ybs apart."""
        pyr, C = self._pyr, x.shape[1]
        w, bias = self.ps.w(f"{cname}.pointwise_conv.conv.weight"), self.ps.w(f"{cname}.pointwise_conv.conv.bias")
        self._c("mmd_pwconv_fwd_pyr" + self._sfx, x, w, y, pyr.head_desc(nsplit), C, N, bias, out_act, stats, lev_stride, ybs,
                None if yoff is None else (ctypes.c_longlong * 5)(*yoff))
        for l in range(nsplit, 5):
            h, wd = pyr.sizes[l]
            self._c("mmd_pwconv_fwd" + self._sfx, pyr.level(x, l), w, pyr.level(y, l) if yoff is None else y, pyr.rows[l], C, N,
                    None, None, NONE, None, None, None, 0, None, h * wd, bias, None, None, out_act,
                    None, None, ybs, 0 if yoff is None else yoff[l], None, 0)

    def _head(self, hname: str, feats: List[Feat], per_anchor: int, out: torch.Tensor, A: int, out_act: int,
              train: bool, tape: Tape):
        """Regressor / Classifier over all 5 pyramid levels per launch (conv weights shared across levels, BN per level:
        bn_list.<lvl>.<i> sit head_layers*C channels apart in the contiguous BN arrays)."""
        ps, spec, pyr = self.ps, self.spec, self._pyr
        C, nl = feats[0].C, spec.head_layers
        lev_stride = nl * C
        off0 = ps.bn_off[f"{hname}.bn_list.0.0"]
        for lvl in range(5):
            for i in range(nl):
                assert ps.bn_off[f"{hname}.bn_list.{lvl}.{i}"] == off0 + lvl * lev_stride + i * C
        nsplit = self._head_nsplit()
        cur, cur_xf = self._fcat, (None, None, NONE, None, None, None)     # (scale, shift, act, stats, gamma, beta)
        layers = []
        for i in range(nl):
            cname = f"{hname}.conv_list.{i}"
            o = off0 + i * C
            zd = self._alloc_pyr(pyr, C, train)
            self._head_dw(cur, cname, zd, cur_xf, nsplit, lev_stride)
            z = self._alloc_pyr(pyr, C, train)
            st = self.stats_flat[2 * o:] if train else None
            self._head_pw(zd, cname, z, C, NONE, st, lev_stride, nsplit)
            if train:
                for lvl in range(5):
                    ol = o + lvl * lev_stride
                    self.bn_count_host[ol:ol + C] = float(pyr.rows[lvl])
                nxt_xf = (None, None, SWISH, st, ps.flat[ps.gamma_off + o:], ps.flat[ps.beta_off + o:])
            else:
                nxt_xf = (ps.fold_scale[o:], ps.fold_shift[o:], SWISH, None, None, None)
            layers.append(HeadLayerRec(cur, None if i == 0 else off0 + (i - 1) * C, zd, z, o))
            cur, cur_xf = z, nxt_xf
        zd = self._alloc_pyr(pyr, C, train)
        self._head_dw(cur, f"{hname}.header", zd, cur_xf, nsplit, lev_stride)
        aoff, yoff = 0, []
        for (h, w) in pyr.sizes:
            yoff.append(aoff * per_anchor)
            aoff += h * w * spec.num_anchors
        self._head_pw(zd, f"{hname}.header", out, spec.num_anchors * per_anchor, out_act, None, 0, nsplit, A * per_anchor, yoff)
        tape.heads[hname] = HeadRec(layers, cur, off0 + (nl - 1) * C, zd, yoff, lev_stride)

    # ------------------------------------------------------------------ backward (student)
    def _slot(self, f: Feat) -> GradSlot:
        k = f.z.data_ptr()
        if k not in self._slots:
            self._slots[k] = GradSlot(self._uses.get(k, 0))
        return self._slots[k]

    def _contrib(self, f: Feat, can_sum: bool) -> Tuple[GradSlot, Optional[BnSums]]:
        """One gradient contribution to `f` is about to be written.  -> (slot, xs); xs = a BnSums when f is the output of a BatchNorm and
        the writing kernel can take that BatchNorm's backward sums (`can_sum`): over the completed gradient when this is the LAST
        contribution (xs.linear = 0), or over its own share when f is max-pooled somewhere (xs.linear = 1, below).  The caller passes
        xs to the kernel in the layout it takes (BnSums.quad / .gemm); the slot's sums are valid once the last contribution has run."""
        s = self._slot(f)
        s.remaining -= 1
        info: Optional[BnOut] = self._bnout.get(f.z.data_ptr())
        if info is not None and self.ps.flat.is_cuda and f.z.data_ptr() in self._linear:
            # linear mode (the tensor is max-pooled by some node, whose backward scatters into its gradient): every contribution adds the
            # sums of its OWN share (linear = 1); they are complete when the last one has, provided none was unable to
            # Exclusivity: the node backward's LDS-tile scatter reads the interior of this gradient at block start and stores it
            # plainly at block end, so a contribution running BESIDE it on another stream would be lost without a trace (global atomics used
            # to make that safe).  Every contribution to a scattered gradient therefore has to be issued on ONE stream.
            cur = torch.cuda.current_stream().cuda_stream
            if s.stream is None:
                s.stream = cur
            elif s.stream != cur:
                raise RuntimeError("contributions to a scattered (max-pooled) gradient issued on two streams: mmd_bifpn_node_bwd_full's "
                                   "LDS-tile scatter needs exclusive access to it (include/mmdistill.h, EXCLUSIVITY)")
            if not can_sum:
                s.linear_ok = False
                return s, None
            linear, s.have_sums = 1, s.remaining == 0 and s.linear_ok
        elif can_sum and s.remaining == 0 and info is not None and self.ps.flat.is_cuda:
            linear, s.have_sums, s.sums = 0, True, None
        else:
            return s, None
        if s.sums is None:
            s.sums = self._zalloc((2 * info.C,), torch.float64)
        return s, BnSums(info.z, info.mean, info.invstd, s.sums, info.mul_b, info.rpi, linear)

    def _acc(self, f: Feat, src: torch.Tensor):
        """gradient of f (+)= src ; the first writer just adopts the tensor (a contribution without BatchNorm sums)."""
        slot, _ = self._contrib(f, False)
        if slot.t is None:
            slot.t = src
        else:
            call("mmd_scale_acc", src, slot.t, None, 0, 0, 1, src.numel())

    @contextlib.contextmanager
    def _wgrad_stream(self):
        """Weight-gradient kernels are leaves of the backward graph (only the optimizer reads them), so they are
        issued on their own stream - a parallel branch of the captured graph - ordered after everything the
        current stream has enqueued so far; backward() joins the stream at its end.  Arena buffers are never
        reused within a step, so the only ordering needed is producer -> wgrad.
        (Round 4: the small leaves - depthwise / squeeze-excite / bias gradients - on a stream of their own, so that they do not queue behind a
        grouped flush's ~0.9 ms kernel, measured WORSE, all of them or only the last few: 14.72 - 14.89 -> 14.88 - 15.02 ms/step - one more
        branch beside the main chain costs more than the 0.1 ms the last two leaves wait.)"""
        if not self.ps.flat.is_cuda or os.environ.get("MMD_NO_WG"):
            yield
            return
        if self._wg is None:
            self._wg = torch.cuda.Stream()
        self._wg.wait_event(torch.cuda.current_stream().record_event())
        with torch.cuda.stream(self._wg):
            # MMD_DEV_SKIP_WG, timing experiment only (gradients are WRONG): what do the weight-gradient kernels cost the step through
            # contention with the main chain?  Every call() issued inside this context is skipped
            saved, _SKIP.on = getattr(_SKIP, "on", False), bool(_lib.dev_switch("MMD_DEV_SKIP_WG"))
            try:
                yield
            finally:
                _SKIP.on = saved

    def _pw_wgrad(self, dy: torch.Tensor, xz: torch.Tensor, dw: torch.Tensor, M: int, K: int, N: int, in_scale=None, in_shift=None,
                  in_act: int = NONE, gate=None, rpi: int = 1):
        """dW[N,K] (+)= dY^T pro(X): recorded, computed by _wg_flush() every WG_CHUNK layers and at the end of the backward segment."""
        if not self.ps.flat.is_cuda or (self.precision != "fp32" and not self._group_bf16()):
            with self._wgrad_stream():
                call("mmd_pwconv_bwd_weight" + self._sfx, dy, xz, dw, M, K, N, in_scale, in_shift, in_act, gate, rpi)
            return
        self._wg_pending.append(WgRec(dy, xz, dw, M, K, N, in_scale, in_shift, in_act, gate, rpi))
        self._wg_count += 1
        if self._wg_count % WG_CHUNK == 0:
            # (counted over the whole backward, not per segment: the split backward of the data-parallel step then flushes at the same layers as
            # the one-segment form - its second segment's 11 layers would otherwise all sit in the exposed last flush)
            self._wg_flush()

    def _group_bf16(self) -> bool:
        """precision "bf16": grouped as well (round 4, mmd_wgrad_grouped_bf16) where the per-layer launches are skeleton-bound - D2 / 512^2 in
        bf16 15.50 -> 14.64 ms/step; at D4 / 768^2 the layers are tall enough that the per-layer launches on the side stream measure the
        same or better (53.0-53.3 vs 53.5-53.8 ms), so tall nets keep them: the rows of the stem output decide."""
        stem = self.tape.stem
        return stem is None or stem.out.M <= 600000

    def _leaf(self, fn):
        """A leaf of the backward graph other than a 1x1-conv weight gradient (depthwise / squeeze-excite / fusion-weight / bias
        gradients): issued on the weight-gradient stream at once (see WG_CHUNK: holding them back to the flushes measured worse)."""
        with self._wgrad_stream():
            fn()

    def _wg_flush(self):
        """Launch the recorded weight gradients: one persistent grid over all (layer, tile, split) items and one fold, on the
        weight-gradient stream behind everything issued so far."""
        pend, self._wg_pending = self._wg_pending, []
        seg = self._wg_segment
        self._wg_segment += 1
        if not pend:
            return
        ptr = lambda t: 0 if t is None else t.data_ptr()
        sig = tuple((ptr(r.dy), ptr(r.x), ptr(r.dw), r.M, r.K, r.N, ptr(r.in_scale), ptr(r.in_shift), r.in_act, ptr(r.gate), r.rpi) for r in pend)
        # one plan per (segment, operand signature): a second step variant captured later ("aug") may lay its operands out
        # differently, and the device tables of the variants captured before must stay alive - their graphs keep reading them
        plan = self._wg_plans.get((seg, sig))
        if plan is None:
            if self.arena.frozen:
                raise RuntimeError("weight-gradient operands moved after graph capture")
            n = len(pend)
            arr = (WgLayer * n)()
            for a, r in zip(arr, pend):
                a.dy, a.x, a.dw = ptr(r.dy), ptr(r.x), ptr(r.dw)
                a.in_scale, a.in_shift, a.gate = ptr(r.in_scale) or None, ptr(r.in_shift) or None, ptr(r.gate) or None
                a.M, a.K, a.N, a.in_act, a.rows_per_image = r.M, r.K, r.N, r.in_act, max(int(r.rpi), 1)
            ni, nt, wsf = ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong()
            rc = _lib.LIB.load().mmd_wgrad_plan(ctypes.cast(arr, ctypes.c_void_p), n, WG_ROWS, ctypes.cast(ctypes.pointer(ni), ctypes.c_void_p),
                                                ctypes.cast(ctypes.pointer(nt), ctypes.c_void_p), ctypes.cast(ctypes.pointer(wsf), ctypes.c_void_p))
            if rc != 0:
                raise RuntimeError(f"mmd_wgrad_plan failed with status {rc}")
            table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.device)
            plan = {"sig": sig, "table": table, "n": n, "items": ni.value, "tiles": nt.value, "ws": wsf.value,
                    "flops": float(sum(2.0 * r.M * r.K * r.N for r in pend)),
                    "bytes": float(sum(4.0 * (r.M * r.K + r.M * r.N + r.N * r.K) for r in pend)),
                    # every layer's M a multiple of 32 (any net at B >= 2): the launch runs without row clamps / masks (mmd_wgrad_grouped_form)
                    "rows32": int(all(r.M % 32 == 0 for r in pend))}
            self._wg_plans[(seg, sig)] = plan
        ws = self._alloc(plan["ws"])
        with self._wgrad_stream():
            call("mmd_wgrad_grouped_form", plan["table"], plan["n"], plan["items"], plan["tiles"], ws, WG_BLOCKS,
                 plan["flops"], plan["bytes"], 1 if self._sfx else 0, plan["rows32"])

    def _bn_bwd(self, g_in: torch.Tensor, z: torch.Tensor, aff: Aff, bn_name: str, act: int, M: int, C: int, rpi: int = 0,
                mul_bc=None, mul_b=None, add_bc=None, sums=None, lazy: bool = False):
        """BN(+act) backward: returns dz (gradient w.r.t. the conv's raw output); dgamma/dbeta accumulated.
        `sums` given = the per-channel sums were produced elsewhere (fused into another pass): pass 2 only.
        lazy: no pass 2 at all - returns a LazyDz that the 1x1 conv's two gradient GEMMs evaluate in their prologues."""
        b = self.ps.bn(bn_name)
        if sums is None:
            sums = self._zalloc((2 * C,), torch.float64)
            call("mmd_bn_bwd_reduce", g_in, z, *aff, act, mul_bc, mul_b, add_bc, rpi, None, sums, M, C, *self._stats_ws(sums, M, C))
        if lazy and mul_bc is None and add_bc is None:
            return LazyDz(g_in, z, aff, sums, act, mul_b, rpi, bn_name, M)
        dz = self._alloc(M, C)
        call("mmd_bn_bwd_apply", g_in, z, aff.mean, aff.invstd, b["gamma"], sums, M, dz, b["dgamma"], b["dbeta"], M, C,
             aff.scale, aff.shift, act, mul_bc, mul_b, add_bc, rpi)
        return dz

    def _pw_bwd(self, dz, x: Feat, wkey: str, N: int, bias_key: Optional[str], want_dx: bool,
                gate=None, plain_in=False, into: Optional[Feat] = None, pool5: Optional[tuple] = None) -> Optional[torch.Tensor]:
        """Gradients of a 1x1 conv.  into = the Feat whose gradient slot receives dx (normally x itself): dx is then written into / on top
        of that slot by the GEMM's epilogue (no scale_acc launch), together with the backward sums of the BatchNorm that produced the
        Feat when this is the slot's last contribution; returns None in that case."""
        ps, M, K = self.ps, x.M, x.C
        # the weight gradient's operand prologue: (in_scale, in_shift, in_act, gate, rows_per_image)
        xargs = (None, None, NONE, gate, x.H * x.W) if plain_in else (x.scale, x.shift, x.act, gate, x.H * x.W)
        if isinstance(dz, LazyDz):
            return self._pw_bwd_lazy(dz, x, wkey, N, want_dx, gate, xargs, into, pool5)
        if bias_key:
            self._leaf(lambda dz=dz, gb=ps.g(bias_key): call("mmd_colsum", dz, gb, M, N))
        self._pw_wgrad(dz, x.z, ps.g(wkey), M, K, N, *xargs)
        if not want_dx:
            return None
        dx = self._alloc(M, K)
        call("mmd_pwconv_bwd_data" + self._sfx, dz, ps.w_t(wkey), dx, M, K, N, 0)
        if into is not None:
            self._acc(into, dx)
            return None
        return dx

    def _into_slot(self, into: Feat, M: int, K: int) -> Tuple[GradSlot, Optional[torch.Tensor], Optional[BnSums]]:
        """A GEMM epilogue is about to write dx [M, K] into `into`'s slot -> (slot, residual = what it holds so far or None, xs of the total)"""
        slot, xs = self._contrib(into, True)
        assert xs is None or not xs.linear, "the GEMM epilogue sums the accumulated total: not a linear-sum (pooled) tensor"
        residual = slot.t
        if slot.t is None:
            slot.t = self._alloc(M, K)
        return slot, residual, xs

    def _pw_bwd_lazy(self, L: LazyDz, x: Feat, wkey: str, N: int, want_dx: bool, gate, xargs: tuple, into: Optional[Feat], pool5: Optional[tuple]):
        """_pw_bwd behind a lazy BatchNorm backward: the BatchNorm backward runs in the operand prologue of the input-gradient GEMM (a
        bias in front of a BatchNorm has an exactly-zero gradient).  That launch also stores the evaluated dz once and adds dgamma /
        dbeta, so the weight gradient - a leaf on the side stream, ordered behind it - is the plain GEMM on one tensor"""
        ps, b, M, K = self.ps, self.ps.bn(L.bn_name), x.M, x.C
        bnargs = (*L.aff, L.sums, L.count, L.act, L.mul_b, L.rpi)
        self._wg_read_done = None
        if not want_dx:
            with self._wgrad_stream():
                call("mmd_pwconv_bwd_weight_bn" + self._sfx, L.g, L.z, x.z, ps.g(wkey), M, K, N, *xargs, *bnargs, b["dgamma"], b["dbeta"])
                self._wg_read_done = torch.cuda.current_stream().record_event() if ps.flat.is_cuda else None
            return None
        dzm = self._alloc(M, N)
        if (into is not None and M >= MBW_MIN_ROWS and L.act == SWISH and L.mul_b is None and gate is None
                and x.scale is None and x.bn is None and x.act == NONE and ps.flat.is_cuda
                and _lib.LIB.load().mmd_mbconv_expand_bwd_supported(K, N) == 1):
            # thin-input expand conv of a high-resolution block: one pass over (g0, z0) - input gradient, weight gradient, no dz0 in HBM
            slot, residual, xs = self._into_slot(into, M, K)
            call("mmd_mbconv_expand_bwd_fused", L.g, L.z, x.z, ps.w(wkey), slot.t, residual, ps.g(wkey), M, K, N, *L.aff, L.sums, L.count,
                 b["dgamma"], b["dbeta"], *(xs.gemm if xs else NO_SUMS_GEMM))
            return None
        # the input-gradient GEMM: mmd_pwconv_bwd_data_bn*, or _bn2* when its epilogue has work - (residual, *BnSums.gemm, slot workspace, slots)
        # for a gradient slot, then pool5 = the MBConv project conv's pooled pass of the squeeze-excite / BatchNorm-1 backward over (z1, dx)
        slot, residual, xs = self._into_slot(into, M, K) if into is not None else (None, None, None)
        dx = slot.t if into is not None else self._alloc(M, K)
        gemm = (L.g, L.z, ps.w_t(wkey), dx, M, K, N, *bnargs, dzm, b["dgamma"], b["dbeta"])
        if into is not None:
            xsargs = (*xs.gemm, *self._stats_ws(xs.sums, M, K)) if xs else (*NO_SUMS_GEMM, None, 0)
            if self._sfx:
                call("mmd_pwconv_bwd_data_bn2" + self._sfx, *gemm, residual, *xsargs, None, None, None, None, None, None, 0)
            else:
                # (the GEMM reduces over N = the conv's output channels: the slab kernel's "K")
                call("mmd_pwconv_bwd_data_bn2_form", *gemm, residual, *xsargs, None, None, None, None, None, None, 0, *self._slab_ws(M, N, K, 1), 0)
        elif pool5 is not None:
            call("mmd_pwconv_bwd_data_bn2" + self._sfx, *gemm, None, *NO_SUMS_GEMM, None, 0, *pool5)
        else:
            call("mmd_pwconv_bwd_data_bn" + self._sfx, *gemm)
        self._pw_wgrad(dzm, x.z, ps.g(wkey), M, K, N, *xargs)
        return None if into is not None else dx

    def _dw_bwd(self, dzd: torch.Tensor, x: Feat, wkey: str, k: int, s: int, bn_aff: Optional[Aff] = None):
        """-> dx, or (dx, sums) when `bn_aff` = the coefficients of the BatchNorm(+swish) that produced x: the
        input-gradient launch then also accumulates that BN's backward sums (no separate reduce pass; stride 2, round 5: they ride in the
        gather launch too) and, except for thin stride-1 layers, the conv's weight gradient (tile kernel; for the 3x3 layers that gives up
        the faster row-streaming input-gradient kernel and still wins: a weight-gradient leaf costs its full kernel time on the saturated
        chip - 18.44 -> 18.27 ms/step)."""
        ps = self.ps
        wg_inside = bn_aff is not None and (s == 2 or x.C >= 64)      # (block 0, 32 channels at 256^2: 221 us inside vs 47 + 67)
        if not wg_inside:
            self._leaf(lambda: call("mmd_dwconv_bwd_weight", x.z, dzd, ps.g(wkey), x.B, x.H, x.W, x.C, k, s, x.scale, x.shift, x.act))
        dx = self._alloc(x.M, x.C)
        if bn_aff is None:
            call("mmd_dwconv_bwd_data", dzd, ps.w(wkey), dx, x.B, x.H, x.W, x.C, k, s, None, None, None, None, None, None, None, 0, None)
            return dx
        sums = self._zalloc((2 * x.C,), torch.float64)
        call("mmd_dwconv_bwd_data", dzd, ps.w(wkey), dx, x.B, x.H, x.W, x.C, k, s, x.z, *bn_aff, sums,
             *self._stats_ws(sums, x.M, x.C), ps.g(wkey) if wg_inside else None)
        return dx, sums

    def _pyr_dw_bwd(self, dzd, wkey: str, g, desc, C: int, ls: int, x, xo: Optional[int], sums):
        """Input gradient of a shared-weight pyramid depthwise conv; its weight gradient rides in the same launch, and so do the sums of
        the BatchNorm(+swish) backward that consumes g: xo = where x's producer sits in the contiguous BatchNorm arrays, `sums` its sums
        (xo None: x is the heads' input, whose BatchNorms belong to the BiFPN)."""
        ps, t = self.ps, (lambda v: None if xo is None else v[xo:])
        call("mmd_dwconv3_pyr", dzd, ps.w(wkey), g, desc, C, 1, None, None, NONE, None, None, None, ls, x, t(self.t_scale), t(self.t_shift),
             NONE if xo is None else SWISH, ps.g(wkey), t(self.t_mean), t(self.t_invstd), sums)

    def _head_bwd(self, hname: str, per_anchor: int, dout: torch.Tensor, rec: HeadRec, pyr: Pyramid, A: int, C: int):
        """Backward of one head over the whole pyramid; returns the gradient w.r.t. the pyramid feature buffer."""
        spec, ps = self.spec, self.ps
        nout = spec.num_anchors * per_anchor
        desc, Mt, ls = pyr.desc, pyr.total, rec.lev_stride
        dy = self._alloc_pyr(pyr, nout, False)          # (the slice launch writes the padding rows itself; the plain input-gradient GEMMs below write every row)
        call("mmd_slice_rows_pyr", dout, dy, desc, nout, A * per_anchor, (ctypes.c_longlong * len(rec.yoff))(*[int(v) for v in rec.yoff]))
        hw_key = f"{hname}.header.pointwise_conv.conv.weight"
        self._leaf(lambda dy=dy, gb=ps.g(f"{hname}.header.pointwise_conv.conv.bias"): call("mmd_colsum", dy, gb, Mt, nout))
        self._pw_wgrad(dy, rec.hzd, ps.g(hw_key), Mt, C, nout)
        dzd = self._alloc_pyr(pyr, C, False)
        call("mmd_pwconv_bwd_data" + self._sfx, dy, ps.w_t(hw_key), dzd, Mt, C, nout, 0)
        xo = rec.hx_off
        # the depthwise weight gradient rides in the (flipped) input-gradient launch: a leaf launch's kernel time is paid in full; so do
        # the sums of the BatchNorm backward that consumes g (x's producer), instead of a reduce pass over (g, z): every layer's `sums`
        # below were filled by the depthwise launch behind it
        bsums = self._zalloc((2 * 5 * ls,), torch.float64)
        off0 = rec.layers[0].off
        g = self._alloc_pyr(pyr, C)
        self._pyr_dw_bwd(dzd, f"{hname}.header.depthwise_conv.conv.weight", g, desc, C, ls, rec.hx, xo, bsums[2 * (xo - off0):])
        for i in reversed(range(spec.head_layers)):
            L = rec.layers[i]
            cname = f"{hname}.conv_list.{i}"
            o = L.off
            sums = bsums[2 * (o - off0):]
            dz = self._alloc_pyr(pyr, C)
            call("mmd_bn_bwd_apply_pyr", g, L.z, self.t_mean[o:], self.t_invstd[o:], ps.flat[ps.gamma_off + o:], sums, desc, ls, dz,
                 ps.grad[ps.gamma_off + o:], ps.grad[ps.beta_off + o:], C, self.t_scale[o:], self.t_shift[o:], SWISH)
            wkey = f"{cname}.pointwise_conv.conv.weight"
            self._pw_wgrad(dz, L.zd, ps.g(wkey), Mt, C, C)
            dzd = self._alloc_pyr(pyr, C, False)
            call("mmd_pwconv_bwd_data" + self._sfx, dz, ps.w_t(wkey), dzd, Mt, C, C, 0)
            xo = L.x_off
            g = self._alloc_pyr(pyr, C)
            self._pyr_dw_bwd(dzd, f"{cname}.depthwise_conv.conv.weight", g, desc, C, ls, L.x, xo,
                             None if xo is None else bsums[2 * (xo - off0):])
        return g

    def backward(self, dcls_logit: torch.Tensor, dreg: torch.Tensor, dfeats: List[Optional[torch.Tensor]],
                 stop_before: Optional[int] = None, dfeat_pyr: Optional[torch.Tensor] = None):
        """Accumulates parameter gradients into ps.grad.  dcls_logit [B,A,NC] is the gradient w.r.t. the
        classifier header's PRE-sigmoid output, dreg [B,A,4], dfeats[l] (nullable) w.r.t. the BiFPN outputs.
        stop_before=k: stop after backbone block k (heads, BiFPN and blocks >= k done, weight-gradient stream joined), so
        that the caller can start the all-reduce of those gradients; backward_finish() runs blocks < k and the stem.
        dfeat_pyr: the same gradients as dfeats as ONE pyramid row buffer (dfeats[l] are its level slices): the heads' input gradients
        and it are then added in one launch that also takes the BatchNorm-backward sums of the last BiFPN cell's five output nodes."""
        # (gradient slot of every activation tensor; the stem BatchNorm's backward sums, once block 0's input-gradient launch has taken them)
        self._slots, self._stem_sums = {}, None
        self._wg_pending, self._wg_segment, self._se_wg, self._wg_count = [], 0, [], 0
        self._backward_heads(dcls_logit, dreg, dfeats, dfeat_pyr)
        self._backward_bifpn()
        self._backward_blocks([b for b in self.spec.blocks if stop_before is None or b.idx >= stop_before])
        if stop_before is None:
            self.backward_finish(0)
        else:
            self._wg_flush()
            if self._wg is not None:
                torch.cuda.current_stream().wait_stream(self._wg)

    def _backward_heads(self, dcls_logit, dreg, dfeats, dfeat_pyr):
        """Both heads, every layer over the whole pyramid in one launch; their input gradients (+ dfeats) land in the last BiFPN cell's slots."""
        spec, ps, tape, pyr = self.spec, self.ps, self.tape, self._pyr
        feats, C = tape.feats, tape.feats[0].C
        fold_heads = ps.flat.is_cuda and (dfeat_pyr is not None or all(d is None for d in dfeats))
        if not fold_heads:
            for f, d in zip(feats, dfeats):
                if d is not None:
                    self._slot(f).t = d
        # the two heads are independent until their input gradients meet: the regressor runs on a side stream
        # (a parallel branch of the captured graph); bsums / workspaces are allocated here on the host, in order
        main_stream = torch.cuda.current_stream() if ps.flat.is_cuda else None
        if main_stream is not None and self._side is None:
            self._side = torch.cuda.Stream()
        fork = main_stream.record_event() if main_stream is not None else None
        gparts = []
        for hname, per_anchor, dout in (("classifier", spec.num_classes, dcls_logit), ("regressor", 4, dreg)):
            use_side = main_stream is not None and hname == "regressor" and not os.environ.get("MMD_NO_SIDE")
            if use_side:
                self._side.wait_event(fork)
            with torch.cuda.stream(self._side if use_side else main_stream):
                gparts.append(self._head_bwd(hname, per_anchor, dout, tape.heads[hname], pyr, tape.A, C))
        if main_stream is not None:
            main_stream.wait_stream(self._side)
        gsum = gparts[0]
        if fold_heads:
            # classifier + regressor (+ MTA) gradients in one launch, which also takes the BatchNorm-backward sums of the five output nodes
            quads = []
            for lvl, f in enumerate(feats):
                sl, xs = self._contrib(f, True)
                sl.t = pyr.level(gsum, lvl)
                quads.append(NO_SUMS_QUAD if xs is None else [t.data_ptr() for t in xs.quad])
            arrs = [(ctypes.c_void_p * 5)(*col) for col in zip(*quads)]         # (z, mean, invstd, sums), each one pointer per level
            call("mmd_pyr_add_bnsums", gparts[0], gparts[1], dfeat_pyr, gsum, pyr.desc, C, *arrs)
        else:
            call("mmd_scale_acc", gparts[1], gsum, None, 0, 0, 1, gsum.numel())
            for lvl, f in enumerate(feats):
                self._acc(f, pyr.level(gsum, lvl))

    def _backward_bifpn(self):
        """BiFPN cells and nodes in reverse; ONE launch at the end finishes all fusion-weight gradients (the nodes' dot products: wdot_all)."""
        spec, ps, tape = self.spec, self.ps, self.tape
        n_nodes = sum(len(nodes) for nodes in tape.nodes)
        wdot_all = self._zalloc((4 * n_nodes,))
        theta_desc = []
        for c in reversed(range(spec.fpn_cells)):
            cell = f"bifpn.{c}"
            for rec in reversed(tape.nodes[c]):
                if self._slot(rec.out).t is None:
                    continue          # node output unused downstream (cannot happen in this topology)
                n = len(theta_desc)
                self._node_bwd(cell, rec, wdot_all[4 * n:4 * n + 4])
                theta_desc.append((ps.entries[f"{cell}.{rec.theta}"].off, ps.w(f"{cell}.{rec.theta}").numel()))
            if c == 0:
                self._bifpn_inputs_bwd(cell)
        if theta_desc:
            key = tuple(theta_desc)
            if key not in self._theta_desc:
                if self.arena.frozen:       # (under capture the upload would be recorded as a copy from a host temporary)
                    raise RuntimeError("fusion-weight gradient operands moved after graph capture")
                self._theta_desc[key] = torch.tensor(theta_desc, dtype=torch.int64, device=self.device)
            self._leaf(lambda d=self._theta_desc[key], n=len(theta_desc): call("mmd_bifpn_theta_bwd_batched", ps.flat, ps.grad, wdot_all, d, n))

    def _node_bwd(self, cell: str, rec: NodeRec, wdot: torch.Tensor):
        """Backward of one BiFPN node; wdot [4] receives the dot products of its fusion-weight gradient."""
        ps, out = self.ps, rec.out
        s, name, W = self._slot(out), f"{cell}.{rec.conv}", out.C
        wkey, dwkey = f"{name}.pointwise_conv.conv.weight", f"{name}.depthwise_conv.conv.weight"
        L = self._bn_bwd(s.t, rec.z, rec.bn, f"{name}.bn", NONE, out.M, W, lazy=True, sums=s.sums if s.have_sums else None)
        ops = in0, in1, up, pl = rec.in0, rec.in1, rec.up, rec.pl
        mode_ = (1 if in1 is not None else 0) | (2 if up is not None else 0) | (4 if pl is not None else 0)
        # whole-node backward (round 4): the node's BatchNorm backward + its 1x1 conv's input gradient (exact fp32 MFMA) + the depthwise /
        # fusion backward in ONE launch instead of a GEMM launch in front of it - 40 launches off the backward's serial chain.  bf16
        # modes: up to width 160 (closer to the fp32 reference than the mode's operand-rounding rule asks for, like the whole-node
        # forward; D2 bf16 13.48 -> 13.25 ms/step); D4 (224) 49.9 -> 52.2: there the bf16 GEMM + two-launch form stays
        full = W % 16 == 0 and W <= 224 and mode_ in (2, 5, 4) and (self.precision == "fp32" or W <= 160)
        dzd = None if full else self._pw_bwd(L, rec.zd, wkey, W, None, True)
        th = ps.w(f"{cell}.{rec.theta}")
        # One gradient contribution per operand, in the order in0, in1, up, pl; all of them leave the one launch below: the
        # same-resolution operands directly, the upsampled one as 2x2 block sums, the pooled one scattered - added to each
        # window's arg-max with atomics, on top of the earlier contributions (or of zeros: a zero-initialised arena buffer when this
        # is the first one), no dx tensor and no max-pool gather launch over the 4x larger source map.  The launch also takes the
        # BatchNorm-backward sums of every operand gradient it completes (bnsums); `own` bits: an operand that is max-pooled by
        # ANOTHER node keeps its sums linearly, this launch adds the sums of its share
        grad, bnsums, own = [(None, 0)] * 4, [NO_SUMS_QUAD] * 4, 0
        for oi, o in enumerate(ops):
            if o is None:
                continue
            sl, xs = self._contrib(o, True)
            accumulate = 0 if sl.t is None else 1
            if sl.t is None:
                sl.t = self._zalloc((o.M, W)) if oi == 3 else self._alloc(o.M, W)
            grad[oi] = (sl.t, accumulate)
            if xs is not None:
                bnsums[oi] = xs.quad
                own |= (1 << oi) if oi < 3 and xs.linear else 0
        assert in1 is None or grad[0][0].data_ptr() != grad[1][0].data_ptr()
        # lazy operands: their values are read as z * scale + shift (finalized coefficients) inside the launch
        lzb = [o is not None and o.bn is not None for o in ops]
        scs = shs = None
        if any(lzb):
            scs = (ctypes.c_void_p * 4)(*[(o.scale.data_ptr() if l else None) for o, l in zip(ops, lzb)])
            shs = (ctypes.c_void_p * 4)(*[(o.shift.data_ptr() if l else None) for o, l in zip(ops, lzb)])
        xargs = (*[o.z if o is not None else None for o in ops], th, ps.w(dwkey))
        gargs = (in0.B, in0.H, in0.W, W, *grad[0], *grad[1], *grad[2], ps.g(dwkey), *bnsums[0], *bnsums[1], *bnsums[2])
        plargs = (grad[3][0], *bnsums[3], own)
        if full:
            # the evaluated dz is stored once for the conv's weight-gradient GEMM (grouped flush)
            bq, zdf = ps.bn(L.bn_name), rec.zd
            dzm = self._alloc(out.M, W)
            call("mmd_bifpn_node_bwd_full", *xargs, wdot, *gargs, *plargs, scs, shs, L.g, L.z, L.aff.scale, L.aff.mean, L.aff.invstd, L.sums,
                 L.count, ps.w_t(wkey), dzm, bq["dgamma"], bq["dbeta"])
            self._pw_wgrad(dzm, zdf.z, ps.g(wkey), out.M, W, W, None, None, NONE, None, zdf.H * zdf.W)
        elif scs is not None:
            call("mmd_bifpn_node_dw_bwd3_lz", *xargs, dzd, None, wdot, *gargs, *plargs, scs, shs)
        elif pl is not None or own:
            call("mmd_bifpn_node_dw_bwd3", *xargs, dzd, None, wdot, *gargs, *plargs)
        else:
            call("mmd_bifpn_node_dw_bwd2", *xargs, dzd, None, wdot, *gargs)

    def _bifpn_inputs_bwd(self, cell: str):
        """The first cell's inputs: the p6 / p7 max-pool backward, then the six down-channel convs (into the backbone taps' slots)."""
        tape = self.tape
        c6, p6_in, p7_in = tape.first
        s7, s6 = self._slot(p7_in), self._slot(p6_in)
        if s7.t is not None:
            self._contrib(p6_in, False)
            acc = 0 if s6.t is None else 1
            if s6.t is None:
                s6.t = self._alloc(p6_in.M, p6_in.C)
            call("mmd_maxpool_same_bwd_acc", p6_in.z, s7.t, s6.t, None, 0, 0, acc, p6_in.B, p6_in.H, p6_in.W, p6_in.C)
        if s6.t is not None:
            sc6, xs = self._contrib(c6, True)
            sc6.t = self._alloc(c6.M, c6.C)
            call("mmd_maxpool_same_bwd_acc2", c6.z, s6.t, sc6.t, None, 0, 0, 0, c6.B, c6.H, c6.W, c6.C, *(xs.quad if xs else NO_SUMS_QUAD))
        for nm in ("p5_down_channel_2", "p4_down_channel_2", "p5_down_channel", "p4_down_channel", "p3_down_channel", "p5_to_p6"):
            name = f"{cell}.{nm}"
            rec = tape.down[name]
            out, x = rec.out, rec.x
            s = self._slot(out)
            if s.t is None:
                continue
            dz = self._bn_bwd(s.t, rec.z, rec.bn, f"{name}.1", NONE, out.M, out.C, lazy=True, sums=s.sums if s.have_sums else None)
            self._pw_bwd(dz, x, f"{name}.0.conv.weight", out.C, None, True, into=x)

    def backward_finish(self, stop_before: int):
        """Second part of a split backward: backbone blocks < stop_before, then the stem."""
        self._backward_blocks([b for b in self.spec.blocks if b.idx < stop_before])
        self._backward_stem()

    def _backward_blocks(self, blocks):
        """Backbone blocks in reverse, then the squeeze-excite FC weight gradients of all of them in one launch."""
        for blk in reversed(blocks):
            self._block_bwd(blk, self.tape.blocks[blk.idx])
        if self._se_wg:
            recs, self._se_wg = self._se_wg, []
            key = tuple((r.dpe.data_ptr(), r.dpr.data_ptr(), r.hpre.data_ptr(), r.pooled.data_ptr(), r.g_reduce_w.data_ptr()) for r in recs)
            if key not in self._se_wg_tabs:
                if self.arena.frozen:
                    raise RuntimeError("squeeze-excite weight-gradient operands moved after graph capture")
                rows = [[v.data_ptr() if isinstance(v, torch.Tensor) else v for v in r] for r in recs]
                self._se_wg_tabs[key] = torch.tensor(rows, dtype=torch.int64, device=self.device)
            tab, nb = self._se_wg_tabs[key], recs[0].dpe.shape[0]
            self._leaf(lambda tab=tab, n=len(recs), mx=max(r.C * r.S for r in recs), nb=nb: call("mmd_se_fc_wgrad_batched", tab, n, mx, nb))

    def _block_bwd(self, blk, rec: BlockRec):
        """Backward of one MBConv block: project conv, squeeze-excite, depthwise conv, expand conv."""
        ps, q = self.ps, f"backbone_net.model._blocks.{blk.idx}"
        inp, f1 = rec.inp, rec.f1
        s = self._slot(rec.out)
        if s.t is None:
            return                # blocks after the last tap do not exist; defensive
        dy, M1, HW1 = s.t, f1.M, f1.H * f1.W
        dz2 = self._bn_bwd(dy, rec.z2, rec.bn2, f"{q}._bn2", NONE, M1, blk.cout, rpi=HW1, mul_b=rec.rs, lazy=True,
                           sums=s.sums if s.have_sums else None)
        # squeeze-excite backward.  One pass over (z1, g1) pools d(gate) AND the partials of the BN-1 backward sums (the SE kernels finish
        # those sums once dpooled is known, so the expanded tensor is not read by a BN reduce pass); that pass rides in the epilogue of
        # the project conv's input-gradient GEMM, which produces g1
        a1 = rec.bn1
        pool5 = self._zalloc((5, f1.B, blk.cmid))
        g1 = self._pw_bwd(dz2, f1, f"{q}._project_conv.conv.weight", blk.cout, None, True, gate=rec.gate, pool5=(f1.z, *a1, pool5, f1.B))
        # the skip branch may ADOPT dy as the gradient slot of the block input, and the block's own input gradient is later
        # accumulated into that buffer in place; with a lazy BatchNorm backward the project conv's weight-gradient GEMM (side
        # stream) still reads dy, so that later accumulation waits for it (the event is long past by then)
        dy_read = self._wg_read_done if blk.skip else None
        if blk.skip:
            self._acc(inp, dy)
        dpe, dpr, dpooled = self._alloc(f1.B, blk.cmid), self._alloc(f1.B, blk.se), self._alloc(f1.B, blk.cmid)
        sums1 = self._zalloc((2 * blk.cmid,), torch.float64)
        segrads = [ps.g(f"{q}._se_{fc}.conv.{p}") for fc in ("reduce", "expand") for p in ("weight", "bias")]
        # two wide launches for the two FC data gradients (both in one, mmd_se_fc_bwd_fused, is correct, but every block recomputes its
        # image's hidden gradient - S*C MACs, serial per wave: measured 17.0 -> 17.7 ms/step)
        dh = self._zalloc((f1.B, blk.se))
        call("mmd_se_fc_bwd", pool5[0], rec.gate, rec.hpre, rec.pooled, ps.w(f"{q}._se_reduce.conv.weight"),
             ps.w(f"{q}._se_expand.conv.weight"), dpe, dpr, dh, dpooled, 1.0 / HW1, None, None, None, None, f1.B, blk.cmid, blk.se, pool5, sums1)
        # the FC weight gradients of all blocks of the segment in one launch at its end
        self._se_wg.append(SeWgRec(dpe, dpr, rec.hpre, rec.pooled, *segrads, blk.cmid, blk.se))
        f0 = rec.f0
        wkey = f"{q}._depthwise_conv.conv.weight"
        # BatchNorm-1 backward evaluated in the prologue of the depthwise input-gradient launch (stride-1 blocks with an expand conv and
        # >= 64 channels: 17 of D2's 23): dz1 is never written; the other blocks keep the apply pass
        bn1_in_dw = blk.expand != 1 and blk.stride == 1 and blk.cmid >= 64
        if not bn1_in_dw:
            dz1 = self._bn_bwd(g1, f1.z, a1, f"{q}._bn1", SWISH, M1, blk.cmid, rpi=HW1, mul_bc=rec.gate, add_bc=dpooled, sums=sums1)
        if blk.expand != 1:
            a0 = rec.bn0
            if bn1_in_dw:
                b1 = ps.bn(f"{q}._bn1")
                g0 = self._alloc(f0.M, f0.C)
                sums0 = self._zalloc((2 * f0.C,), torch.float64)
                call("mmd_dwconv_bwd_data_bn1", g1, f1.z, ps.w(wkey), g0, f0.B, f0.H, f0.W, f0.C, blk.kernel, *a1, sums1, M1, rec.gate,
                     dpooled, b1["dgamma"], b1["dbeta"], f0.z, *a0, sums0, *self._stats_ws(sums0, f0.M, f0.C), ps.g(wkey))
            else:
                g0, sums0 = self._dw_bwd(dz1, f0, wkey, blk.kernel, blk.stride, bn_aff=a0)
            dz0 = self._bn_bwd(g0, f0.z, a0, f"{q}._bn0", SWISH, f0.M, blk.cmid, sums=sums0, lazy=True)
            if dy_read is not None:
                torch.cuda.current_stream().wait_event(dy_read)
            # the input gradient lands in (on top of) the block input's slot - which may be dy itself, adopted by the skip branch
            # above - and, as that slot's last contribution, carries the previous block's BatchNorm-2 backward sums with it
            self._pw_bwd(dz0, inp, f"{q}._expand_conv.conv.weight", blk.cmid, None, True, into=inp)
        elif blk.idx == 0 and not blk.skip and blk.stride == 1 and self._slot(inp).t is None:
            # block 0 consumes the stem activation directly and is its only consumer: the stem BN's backward sums ride
            # in this input-gradient launch
            stem = self.tape.stem
            g0, self._stem_sums = self._dw_bwd(dz1, f0, wkey, blk.kernel, blk.stride, bn_aff=Aff(inp.scale, inp.shift, stem.mean, stem.invstd))
            self._acc(inp, g0)
        else:
            g0 = self._dw_bwd(dz1, f0, wkey, blk.kernel, blk.stride)
            if dy_read is not None:
                torch.cuda.current_stream().wait_event(dy_read)
            self._acc(inp, g0)

    def _backward_stem(self):
        ps, tape, P, stem_sums = self.ps, self.tape, "backbone_net.model", self._stem_sums
        ximg, stem, mu, istd = tape.stem
        s = self._slot(stem)
        Bi, Cin, Hi, Wi = ximg.shape
        dll = _lib.LIB.load() if ps.flat.is_cuda else None
        # stem weight gradient straight from the NCHW image (mmd_stem_conv_bwd_weight_bn) where the kernel covers the geometry, else im2col + a
        # GEMM item of the last grouped flush
        # (every precision mode: the bf16 rule rounds the operands of the 1x1 convs only - the stem is a 3x3 conv and stays fp32)
        direct = dll is not None and dll.mmd_stem_conv_bwd_weight_supported(Cin, Hi, Wi, ps.stem_kp, stem.C) == 1
        if direct:
            # the last grouped flush (the thin 256^2 layers of blocks 0 - 2) starts NOW, beside the stem's BatchNorm backward and the stem's
            # own weight gradient: the step's exposed tail is the longer of the two, not their sum
            self._wg_flush()
            # no im2col matrix (168 MB at 512^2 x 8 channels): the patches are gathered from the image rows while the dz tile is multiplied -
            # and no dz tensor either: the stem BatchNorm's backward is evaluated while that tile is staged (mmd_stem_conv_bwd_weight_bn)
            if stem_sums is None:
                stem_sums = self._zalloc((2 * stem.C,), torch.float64)
                call("mmd_bn_bwd_reduce", s.t, stem.z, stem.scale, stem.shift, mu, istd, SWISH, None, None, None, 0, None, stem_sums, stem.M, stem.C,
                     *self._stats_ws(stem_sums, stem.M, stem.C))
            b0 = ps.bn(f"{P}._bn0")
            ws = self._alloc(int(dll.mmd_stem_wgrad_ws_floats(stem.C)))
            # on the MAIN stream, whose chain ends here: on the second side stream (the earlier placement) the branch came out serialised BEHIND
            # the grouped flush in the captured graph (rocprofv3 trace: flush 278 us -> fold 46 -> stem 78 -> fold 12, all exposed), the
            # main branch runs beside it
            call("mmd_stem_conv_bwd_weight_bn", ximg, s.t, stem.z, ps.g(f"{P}._conv_stem.conv.weight"), ws, Bi, Cin, Hi, Wi, ps.stem_kp, stem.C,
                 stem.scale, stem.shift, mu, istd, stem_sums, stem.M, SWISH, b0["dgamma"], b0["dbeta"])
        else:
            dz = self._bn_bwd(s.t, stem.z, Aff(stem.scale, stem.shift, mu, istd), f"{P}._bn0", SWISH, stem.M, stem.C, sums=stem_sums)
            with self._wgrad_stream():          # im2col of the input image + weight-gradient GEMM, both off the critical path
                col = self._alloc(stem.M, ps.stem_kp)
                call("mmd_stem_im2col", ximg, col, Bi, Cin, Hi, Wi, ps.stem_kp)
            self._pw_wgrad(dz, col, ps.g(f"{P}._conv_stem.conv.weight"), stem.M, ps.stem_kp, stem.C)
            self._wg_flush()
        if self._wg is not None:
            torch.cuda.current_stream().wait_stream(self._wg)
