"""Launch recorder: run one small eager case of the engine and write one line per kernel-library call.

    python tools/dev/launch_log.py CASE OUT.log          (one fresh process per case; `--list` names the cases)

Two commits issue the same launches iff their logs are equal byte for byte (profiles/engine_backward_notes.md,
profiles/engine_forward_notes.md).  The recorder replaces
mm_distillnet_amd._lib.call BEFORE engine / step are imported, forwards to the real call, and logs per call: the ordinal (by first
appearance) of the current stream, the entry-point name, and per argument
  int / float          its value
  tensor               shape, dtype and the ordinal (by first appearance) of its data_ptr() - two same-shaped tensors swapped show up
  ctypes pointer array per slot None or the pointer's ordinal (the same table as the tensors')
  ctypes int array     its values
  None                 None
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

_real_call = _lib.call
LINES, _STREAMS, _PTRS = [], {}, {}


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

from mm_distillnet_amd.arch import make_spec                           # noqa: E402
from mm_distillnet_amd.engine import Net                               # noqa: E402
from mm_distillnet_amd.step import DistillEngine, StepConfig           # noqa: E402
from mm_distillnet_amd.synth import synth_state, synth_inputs          # noqa: E402

DEV = "cuda:0"


def train_steps(precision: str, augment: bool, split: bool, steps: int, B: int = 2):
    """Three D2 teachers + D2 student, 256^2: `steps` eager training steps (split: the two-segment backward of the data-parallel step).
    B = 2: one teacher per stream (8 rows per net on the 2^2 level: no pack); B = 8: the teachers as ONE pack forward, whose 2^2 level (32 rows
    per net, not whole 128-row tiles) the heads run as plain trailing-level launches."""
    S = 256
    specs = {"rgb": make_spec(2, 3), "depth": make_spec(2, 3), "thermal": make_spec(2, 1)}
    tstates = {k: synth_state(s, seed=i + 1, cls_bias=-1.0) for i, (k, s) in enumerate(specs.items())}
    sspec = make_spec(2, 8)
    eng = DistillEngine(sspec, specs, DEV, StepConfig(image_size=S, precision=precision, augment=augment))
    eng.load(synth_state(sspec, seed=9), tstates)
    if split:
        eng.ar_split = eng._default_split()
    batch = {k: v.to(DEV) for k, v in synth_inputs(B, S, seed=3).items()}
    ds = torch.ones(eng.n_skip, B, device=DEV)
    for _ in range(steps):
        eng.step(batch, ds)


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
