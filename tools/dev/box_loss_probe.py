"""What the IoU-family box regression criteria cost inside the focal launch sequence (profiles/box_loss_notes.md):

    python3 tools/dev/box_loss_probe.py

Builds bench.py's workload on one box (three D2 teachers + the audio student, 8 x 512^2, the bench's synthetic states), replays one captured
step and takes the student's outputs and the merged pseudo-labels it left; then times the four launches of the focal sequence (zero, assign,
loss, finalize) on those arrays - mmd_focal_loss, and mmd_focal_loss_box in each mode - as back-to-back calls between two events, in
alternating rounds."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import bench as BN  # noqa: E402
from mm_distillnet_amd import _lib  # noqa: E402
from mm_distillnet_amd.arch import make_spec  # noqa: E402
from mm_distillnet_amd.step import BOX_LOSSES, DistillEngine, StepConfig  # noqa: E402
from mm_distillnet_amd.synth import synth_inputs  # noqa: E402

DEV = "cuda:0"
LAUNCHES, ROUNDS = 200, 9


def between_events(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def main():
    torch.cuda.set_device(0)
    S, B, coef = 512, 8, 2
    mods = {"rgb": (3, 1), "depth": (3, 2), "thermal": (1, 3)}
    specs = {k: make_spec(coef, c) for k, (c, _) in mods.items()}
    calib = synth_inputs(4, 256, seed=1234)
    tstates = {k: BN.oracle_calibrated_state(specs[k], seed, calib[k], coef) for k, (_, seed) in mods.items()}
    sspec = make_spec(coef, 8)
    sstate = BN.oracle_calibrated_state(sspec, 4, calib["audio"], coef)
    batch_cpu = synth_inputs(B, S, seed=24)
    for k in tstates:
        BN.tune_teacher_bias(specs[k], tstates[k], batch_cpu[k], DEV)
    batch = {k: v.to(DEV) for k, v in batch_cpu.items()}
    eng = DistillEngine(sspec, specs, DEV, StepConfig(image_size=S, lr=BN.BENCH_LR))
    eng.load(sstate, tstates)
    eng.capture(batch)
    eng.replay(batch)
    torch.cuda.synchronize()
    eng.check_overflow()
    out = eng.out
    cls, reg = out["cls_s"].clone(), out["reg_s"].clone()
    boxes, nbox = out["boxes"].clone(), out["nbox"].clone()
    anchors = eng.student.anchors(S)
    A, nc, G = anchors.shape[0], sspec.num_classes, boxes.shape[1]
    assign = torch.empty(B * A, dtype=torch.int32, device=DEV); npos = torch.empty(B, dtype=torch.int32, device=DEV)
    acc = torch.empty(2 * B, dtype=torch.float64, device=DEV); main_ = torch.empty(2, device=DEV)
    dcls, dreg = torch.empty(B, A, nc, device=DEV), torch.empty(B, A, 4, device=DEV)
    anyb = torch.zeros(1, dtype=torch.int32, device=DEV)
    common = (cls, reg, anchors, boxes, nbox, G, B, A, nc, assign, npos, acc, main_, dcls, dreg, 1.0, 1, anyb)
    runs = {"mmd_focal_loss": lambda: _lib.call("mmd_focal_loss", *common)}
    for name, mode in BOX_LOSSES.items():
        runs["mmd_focal_loss_box %s" % name] = (lambda m: lambda: _lib.call("mmd_focal_loss_box", *common, m, 1.0))(mode)
    t = {k: [] for k in runs}
    losses = {}
    for k, fn in runs.items():
        fn(); torch.cuda.synchronize()
        losses[k] = main_.cpu().tolist()
    for _ in range(ROUNDS):
        for k, fn in runs.items():
            t[k].append(between_events(fn, LAUNCHES))
    print("B %d, A %d, NC %d, boxes per image %s, positive anchors per image %s" % (B, A, nc, nbox.tolist(), npos.tolist()))
    for k, v in t.items():
        print("  %-32s median %7.2f us  min %7.2f  max %7.2f  (regression, classification loss %s; %d rounds of %d back-to-back calls)"
              % (k, statistics.median(v), min(v), max(v), losses[k], ROUNDS, LAUNCHES))


if __name__ == "__main__":
    main()
