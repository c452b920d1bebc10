"""Launch recorder: run one small eager case of the engine and write one line per kernel-library call, arena allocation and stream edge.

    python tools/dev/launch_log.py CASE OUT.log          (one fresh process per case; `--list` names the cases)

Two commits issue the same launches iff their logs are equal byte for byte (profiles/engine_backward_notes.md,
profiles/engine_forward_notes.md, profiles/step_notes.md).  The recorder replaces
mm_distillnet_amd._lib.call BEFORE engine / step are imported, forwards to the real call, and logs per call: the ordinal (by first
appearance) of the current stream, the entry-point name, and per argument
  int / float          its value
  tensor               shape, dtype and the ordinal (by first appearance) of its data_ptr() - two same-shaped tensors swapped show up
  ctypes pointer array per slot None or the pointer's ordinal (the same table as the tensors')
  ctypes int array     its values
  None                 None
Interleaved with these, one line per
  Arena.alloc          `a<arena> alloc <shape> <dtype>`: the arena's ordinal by first appearance - the allocation order itself
  Stream.wait_event / wait_stream / record_event (patched on the Python class before step is imported)
                       `s<stream> wait_event e<event>`, `s<stream> wait_stream s<other>`, `s<stream> record_event e<event>`: the stream
                       table is the launches', events count by first appearance (wait_stream is torch's record_event + wait_event, which
                       follow it as lines of their own).  Every recorded event is kept alive, so no id comes back
Eager runs, no graph capture.  Work-skipping runs (MMD_DEV=1 MMD_DEV_SKIP_WG=1) are logged like any other: the caller sets the environment.
"""
import collections
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch                                    # noqa: E402
from mm_distillnet_amd import _lib              # noqa: E402
from mm_distillnet_amd.store import Arena       # noqa: E402

_real_call = _lib.call
LINES, _STREAMS, _PTRS, _ARENAS, _EVENTS, _KEEP = [], {}, {}, {}, {}, []


def _ordinal(table: dict, key: int) -> int:
    return table.setdefault(key, len(table))


def _describe(a) -> str:
    if a is None:
        return "None"
    if isinstance(a, torch.Tensor):
        return "T%s:%s@%d" % (list(a.shape), str(a.dtype).replace("torch.", ""), _ordinal(_PTRS, a.data_ptr()))
    if isinstance(a, (bool, int, float)):
        return repr(a)
    if isinstance(a, ctypes.Array):
        if a._type_ is ctypes.c_void_p:
            return "P[%s]" % ",".join("None" if v is None else "@%d" % _ordinal(_PTRS, v) for v in a)
        return "I[%s]" % ",".join(str(int(v)) for v in a)
    raise TypeError("launch_log: unexpected argument type %r" % type(a))


def _recording_call(name: str, *args):
    LINES.append("s%d %s %s" % (_ordinal(_STREAMS, torch.cuda.current_stream().cuda_stream), name, " ".join(_describe(a) for a in args)))
    return _real_call(name, *args)


_lib.call = _recording_call


def _stream(s) -> str:
    return "s%d" % _ordinal(_STREAMS, s.cuda_stream)


def _event(e) -> str:
    _KEEP.append(e)
    return "e%d" % _ordinal(_EVENTS, id(e))


def _patch_streams():
    cls = torch.cuda.Stream
    alloc, wait_event, wait_stream, record_event = Arena.alloc, cls.wait_event, cls.wait_stream, cls.record_event

    def rec_alloc(self, shape, dtype=torch.float32):
        if id(self) not in _ARENAS:
            _KEEP.append(self)
        LINES.append("a%d alloc %s %s" % (_ordinal(_ARENAS, id(self)), [int(d) for d in shape], str(dtype).replace("torch.", "")))
        return alloc(self, shape, dtype)

    def rec_wait_event(self, event):
        LINES.append("%s wait_event %s" % (_stream(self), _event(event)))
        return wait_event(self, event)

    def rec_wait_stream(self, stream):
        LINES.append("%s wait_stream %s" % (_stream(self), _stream(stream)))
        return wait_stream(self, stream)

    def rec_record_event(self, event=None):
        event = record_event(self, event)
        LINES.append("%s record_event %s" % (_stream(self), _event(event)))
        return event

    Arena.alloc, cls.wait_event, cls.wait_stream, cls.record_event = rec_alloc, rec_wait_event, rec_wait_stream, rec_record_event


_patch_streams()

from mm_distillnet_amd.arch import make_spec                           # noqa: E402
from mm_distillnet_amd.engine import Net                               # noqa: E402
from mm_distillnet_amd.step import DistillEngine, StepConfig           # noqa: E402
from mm_distillnet_amd.synth import synth_state, synth_inputs          # noqa: E402

DEV = "cuda:0"


def _engine(B: int, S: int = 256, **cfg):
    """Three D2 teachers + D2 student at S^2 with synthetic weights, and a batch of B on the device."""
    specs = {"rgb": make_spec(2, 3), "depth": make_spec(2, 3), "thermal": make_spec(2, 1)}
    tstates = {k: synth_state(s, seed=i + 1, cls_bias=-1.0) for i, (k, s) in enumerate(specs.items())}
    sspec = make_spec(2, 8)
    eng = DistillEngine(sspec, specs, DEV, StepConfig(image_size=S, **cfg))
    eng.load(synth_state(sspec, seed=9), tstates)
    return eng, {k: v.to(DEV) for k, v in synth_inputs(B, S, seed=3).items()}


def _fixed_labels(eng, B: int, n_src: int = 3):
    """labels_from_rows on two or three fixed boxes per image and source"""
    A = eng.student.anchors(eng.cfg.image_size).shape[0]
    per = [[[[20.0 + 8 * t + 4 * i + 30 * k, 30.0 + 6 * k, 90.0 + 8 * t + 4 * i + 30 * k, 110.0 + 6 * k, 0.9 - 0.1 * k - 0.05 * t, 0.0]
             for k in range(2 + (i + t) % 2)] for i in range(B)] for t in range(n_src)]
    return eng.labels_from_rows(per, A)


def train_steps(precision: str, augment: bool, split: bool, steps: int, B: int = 2, aug_rgb: bool = False, injected: bool = False, **cfg):
    """Three D2 teachers + D2 student, 256^2: `steps` eager training steps (split: the two-segment backward of the data-parallel step).
    B = 2: one teacher per stream (8 rows per net on the 2^2 level: no pack); B = 8: the teachers as ONE pack forward, whose 2^2 level (32 rows
    per net, not whole 128-row tiles) the heads run as plain trailing-level launches.
    aug_rgb: the batch carries the KD-list variant's extra RGB input; injected: the pseudo-labels come from `_fixed_labels`; cfg: StepConfig keys."""
    eng, batch = _engine(B, precision=precision, augment=augment, **cfg)
    if split:
        eng.ar_split = eng._default_split()
    if aug_rgb:
        batch["aug_rgb"] = synth_inputs(B, 256, seed=57)["rgb"].to(DEV)
    ds = torch.ones(eng.n_skip, B, device=DEV)
    labels = _fixed_labels(eng, B) if injected else None
    for _ in range(steps):
        if labels is None:
            eng.step(batch, ds)
        else:       # step() takes no labels: its body, tail and optimizer (one rank: no exchange in between)
            eng.step_body(batch, ds, teacher_labels=labels)
            eng.backward_tail()
            eng.optimizer_body()


def eval_paths():
    """The evaluation entry points on one engine: validation losses, the device record with its table, predict."""
    eng, batch = _engine(2)
    eng.eval_losses(batch)
    eng.begin_eval(4, 32768)
    eng.eval_batch(batch)
    eng.end_eval_table(256, with_record=True)
    eng.predict(batch)


def merge_only():
    """merge_labels alone on labels_from_rows output, as NMS and as weighted box fusion."""
    for merge in ("nms", "wbf"):
        eng, _ = _engine(2, label_merge=merge)
        labels = _fixed_labels(eng, 2)
        eng.merge_labels([r for r, _ in labels], [c for _, c in labels])


def net_fwd_bwd(coef: int, S: int, precision: str = "fp32", probe: bool = False):
    """One trainable net: train forward + net.backward(dcls, dreg, dfe) the way tests/test_gpu_net.py calls it."""
    spec = make_spec(coef, 8)
    net = Net(spec, DEV, trainable=True, precision=precision)
    net.load_state(synth_state(spec, seed=13))
    if probe:
        net.probe = {}
    x = synth_inputs(2, S, seed=25)["audio"].to(DEV)
    ds = torch.ones(sum(1 for b in spec.blocks if b.skip), 2, device=DEV)
    net.begin_step()
    cls, reg, feats = net.forward(x, train=True, drop_scale=ds)
    dcls = (0.01 * cls * (1 - cls)).contiguous()
    dreg = (2.0 * reg / reg.numel()).contiguous()
    dfe = [(2.0 * u.z / u.z.numel()).contiguous() for u in feats]
    net.ps.grad.zero_()
    net.backward(dcls, dreg, dfe)


def net_eval(coef: int, S: int, precision: str = "fp32", raw_logits: bool = False, fuse_node: bool = True):
    """One frozen net outside a pack: eval forward at B = 2 (fuse_node False: the two-launch BiFPN node leg, as tests/test_gpu_net.py sets it)."""
    spec = make_spec(coef, 3)
    net = Net(spec, DEV, trainable=False, precision=precision)
    net.load_state(synth_state(spec, seed=13))
    net.FUSE_NODE = fuse_node
    x = synth_inputs(2, S, seed=25)["rgb"].to(DEV)
    net.begin_step()
    net.forward(x, raw_logits=raw_logits)


CASES = {
    "step_fp32": lambda: train_steps("fp32", False, False, 2),
    "step_bf16_aug": lambda: train_steps("bf16", True, False, 2),
    "split": lambda: train_steps("fp32", False, True, 1),
    "d4_fp32": lambda: net_fwd_bwd(4, 256),                      # width 224: non-lazy BiFPN
    "d4_bf16": lambda: net_fwd_bwd(4, 256, "bf16"),              # ... and the two-launch node legs (mmd_bifpn_node_dw_bwd3 / _bwd2)
    "d0": lambda: net_fwd_bwd(0, 128),
    "d1": lambda: net_fwd_bwd(1, 128),                           # width 88
    "d2_probe": lambda: net_fwd_bwd(2, 128, probe=True),         # non-lazy at width 112
    "pack_fp32": lambda: train_steps("fp32", False, False, 1, B=8),     # the pack forward with a trailing level (the cases above do not pack)
    "pack_bf16": lambda: train_steps("bf16", False, False, 1, B=8),
    # the step's other branches, one eager step each at 256^2 (profiles/step_notes.md); pack_fp32 under MMD_PACK_SPLIT=2 / MMD_NO_PACK=1 /
    # MMD_STAGGER=-1 covers the partial pack, one teacher per stream and the schedule without stagger waits: the caller sets the environment
    "list_aug": lambda: train_steps("fp32", False, False, 1, aug_rgb=True, kd_mode="list"),      # fourth pass, label index G, nt + 1
    "at_loss": lambda: train_steps("fp32", False, False, 1, kd_loss="AttentionLoss"),
    "no_kd": lambda: train_steps("fp32", False, False, 1, kd_loss="None"),
    "injected": lambda: train_steps("fp32", False, False, 1, injected=True),
    "injected_b8": lambda: train_steps("fp32", False, False, 1, B=8, injected=True),             # the pack leg's teacher_labels[gi]
    "wbf_giou": lambda: train_steps("fp32", False, False, 1, label_merge="wbf", box_loss="giou", box_weight=2.0),
    "opt_adamw_clip_ema": lambda: train_steps("fp32", False, False, 1, optimizer="AdamW", grad_clip=1.0, ema_decay=0.999),
    "eval_paths": eval_paths,
    "merge_only": merge_only,
    # frozen single-net forwards
    "eval_d2_fp32": lambda: net_eval(2, 128),
    "eval_d2_bf16_raw": lambda: net_eval(2, 128, "bf16", raw_logits=True),
    "eval_d2_two_launch": lambda: net_eval(2, 128, fuse_node=False),
    "eval_d4": lambda: net_eval(4, 256),                         # width 224: the NODE_FUSE_WIDE_MAXROWS branch of _node_fusable
}


def main(argv):
    if argv[1:] == ["--list"]:
        print(" ".join(CASES))
        return 0
    if len(argv) != 3 or argv[1] not in CASES:
        print(__doc__)
        return 2
    torch.cuda.set_device(0)
    CASES[argv[1]]()
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(argv[2])), exist_ok=True)
    with open(argv[2], "w") as f:
        f.write("\n".join(LINES) + "\n")
    names = collections.Counter(line.split()[1] for line in LINES)
    shown = sorted(n for n in names if "node" in n and "bwd" in n or "pwconv_bwd_data" in n or n in (
        "mmd_mbconv_expand_bwd_fused", "mmd_dwconv_bwd_data_bn1", "mmd_pyr_add_bnsums", "mmd_maxpool_same_bwd_acc2"))
    print("%s: %d lines, %d streams; %s" % (argv[1], len(LINES), len(_STREAMS), ", ".join("%s %d" % (n, names[n]) for n in shown)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
