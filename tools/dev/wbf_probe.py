"""What the weighted box fusion costs beside the NMS it stands in for (profiles/wbf_merge_notes.md):

    python3 tools/dev/wbf_probe.py

Builds bench.py's workload twice on one box (three D2 teachers + the audio student, 8 x 512^2, the bench's synthetic states), one engine
with label_merge = nms and one with wbf, and prints
  - the merge launch alone, mmd_nms_merge_n against mmd_wbf_merge_n, on the pseudo-label arrays one step of the teachers produced and on a
    stress shape of 999 rows per image: back-to-back launches between two events, alternating rounds;
  - the captured step of both engines, alternating rounds of replays."""
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import bench as BN  # noqa: E402
from mm_distillnet_amd import _lib  # noqa: E402
from mm_distillnet_amd.arch import make_spec  # noqa: E402
from mm_distillnet_amd.postproc import nms_workspace, wbf_merge  # noqa: E402
from mm_distillnet_amd.step import DistillEngine, StepConfig  # noqa: E402
from mm_distillnet_amd.store import Arena  # noqa: E402
from mm_distillnet_amd.synth import synth_inputs  # noqa: E402

DEV = "cuda:0"
LAUNCHES, REPLAYS, ROUNDS = 200, 10, 9


def between_events(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def merge_pair(rows, cnts, B, cap, G):
    """-> (nms launch, wbf launch) over the same arrays, outputs in an arena of their own"""
    ws = Arena(DEV, 64 << 20)
    ovf = torch.zeros(1, dtype=torch.int32, device=DEV)
    ns = len(rows)
    boxes, nbox = ws.alloc((B, G, 5)), ws.alloc((B,), torch.int32)
    mask = ws.alloc((B * 1024 * 16,), torch.int64)
    big = nms_workspace(ws, B, ns * cap)
    vp = ctypes.c_void_p
    srcs, cn = (vp * ns)(*[t.data_ptr() for t in rows]), (vp * ns)(*[t.data_ptr() for t in cnts])
    mark = (ws.ci, ws.off)

    def nms():
        _lib.call("mmd_nms_merge_n", srcs, cn, ns, 0.5, 0, B, boxes, nbox, G, mask, ovf, 0, cap, big)

    def wbf():
        ws.ci, ws.off = mark
        return wbf_merge(ws, rows, cnts, B, cap, 0.5, False, G, 1, ovf)
    return nms, wbf, nbox, ovf


def report(name, rows, cnts, B, cap, G):
    nms, wbf, nbox, ovf = merge_pair(rows, cnts, B, cap, G)
    per = torch.stack(cnts).sum(0).cpu().tolist()
    nms(); torch.cuda.synchronize(); kept = nbox.cpu().tolist()
    _, nb, aux = wbf(); torch.cuda.synchronize(); fused = nb.cpu().tolist()
    members = max(float(aux[i, :fused[i], 1].max()) for i in range(B) if fused[i])
    t = {"nms": [], "wbf": []}
    for _ in range(ROUNDS):
        t["nms"].append(between_events(nms, LAUNCHES)); t["wbf"].append(between_events(wbf, LAUNCHES))
    print("%s: rows per image %s; NMS keeps %s, fusion emits %s (largest cluster %d members); overflow flag %d"
          % (name, per, kept, fused, members, int(ovf.item())))
    for k, v in t.items():
        print("  %-4s launch: median %7.2f us  min %7.2f  max %7.2f  (%d rounds of %d back-to-back launches)"
              % (k, statistics.median(v), min(v), max(v), ROUNDS, LAUNCHES))


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
    engines = {}
    for name in ("nms", "wbf"):
        eng = DistillEngine(sspec, specs, DEV, StepConfig(image_size=S, lr=BN.BENCH_LR, label_merge=name))
        eng.load({k: v.clone() for k, v in sstate.items()}, tstates)
        eng.capture(batch)
        eng.replay(batch)
        torch.cuda.synchronize()
        eng.check_overflow()
        engines[name] = eng
    out = engines["nms"].out
    cap = engines["nms"].cap
    rows, cnts = [r.clone() for r in out["rows_t"]], [c.clone() for c in out["cnt_t"]]
    G = int(max(torch.stack(cnts).sum(0).max().item(), 1))
    report("bench step's pseudo-labels", rows, cnts, B, cap, G)
    # stress: 333 rows per source and image, boxes of 16 .. 64 px scattered over 512^2, four labels
    rng = np.random.default_rng(3)
    cap_s, n = 352, 333
    srows, scnts = [], []
    for _ in range(3):
        a = np.zeros((B, cap_s, 6), np.float32)
        x, y = rng.uniform(0, 448, (B, cap_s)), rng.uniform(0, 448, (B, cap_s))
        a[..., 0], a[..., 1] = x, y
        a[..., 2], a[..., 3] = x + rng.uniform(16, 64, (B, cap_s)), y + rng.uniform(16, 64, (B, cap_s))
        a[..., 4], a[..., 5] = rng.uniform(0.3, 1, (B, cap_s)), rng.integers(0, 4, (B, cap_s))
        srows.append(torch.from_numpy(a).to(DEV)); scnts.append(torch.full((B,), n, dtype=torch.int32, device=DEV))
    report("stress", srows, scnts, B, cap_s, 3 * n)
    # the captured step, alternating
    t = {k: [] for k in engines}
    for _ in range(ROUNDS):
        for k, eng in engines.items():
            t[k].append(between_events(lambda: eng.replay(batch), REPLAYS) / 1e3)
    for k, v in t.items():
        print("step, label_merge = %s: median %7.3f ms  min %7.3f  max %7.3f  (%d rounds of %d replays, alternating)"
              % (k, statistics.median(v), min(v), max(v), ROUNDS, REPLAYS))
    for eng in engines.values():
        eng.check_overflow()
    print("merged labels per image: nms %s, wbf %s" % (engines["nms"].out["nbox"].tolist(), engines["wbf"].out["nbox"].tolist()))


if __name__ == "__main__":
    main()
