"""The cost of the weight averaging in the optimizer graph (profiles/ema_notes.md):

    python3 tools/dev/ema_probe.py                 time the captured optimizer_body of a D2 student with ema_decay = 0 and 0.9998 on one box,
                                                   alternating, and the EMA launch alone in a graph of its own
    python3 tools/dev/ema_probe.py launch [N]      N eager mmd_ema_update launches at D2's sizes, nothing else: the target of
                                                   rocprofv3 --pmc FETCH_SIZE (or WRITE_SIZE) -d DIR -o ema -- python3 tools/dev/ema_probe.py launch

Only the optimizer runs: the gradient buffer is filled with small random numbers, no forward or backward is issued."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from mm_distillnet_amd import _lib  # noqa: E402
from mm_distillnet_amd.arch import make_spec  # noqa: E402
from mm_distillnet_amd.step import DistillEngine, StepConfig  # noqa: E402
from mm_distillnet_amd.synth import synth_state  # noqa: E402

DEV = "cuda"
REPLAYS, ROUNDS = 100, 11


def engine(ema_decay):
    spec = make_spec(2, 8)
    eng = DistillEngine(spec, {"rgb": make_spec(2, 3)}, DEV, StepConfig(image_size=512, ema_decay=ema_decay))
    eng.student.load_state(synth_state(spec, seed=7))
    eng.reset_ema()
    eng.student.ps.grad.copy_(torch.randn(eng.student.ps.n_params, device=DEV) * 1e-3)
    eng.head_active.fill_(1)
    return eng


def captured(body):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        body()                       # code objects loaded before the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        body()
    return g


def time_us(g):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPLAYS):
        g.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / REPLAYS


def ema_call(eng):
    ps = eng.student.ps
    _lib.call("mmd_ema_update", ps.flat, eng.ema_flat, ps.n_params, ps.rmean, eng.ema_rmean, ps.bn_total, ps.rvar, eng.ema_rvar,
              ps.bn_total, eng.ema_state, 0.9998, 1)


def main():
    if sys.argv[1:2] == ["launch"]:
        eng = engine(0.9998)
        for _ in range(int(sys.argv[2]) if len(sys.argv) > 2 else 5):
            ema_call(eng)
        torch.cuda.synchronize()
        ps = eng.student.ps
        print("launched: n_params %d, bn_total %d, algorithmic bytes per launch %d" % (ps.n_params, ps.bn_total,
                                                                                     12 * (ps.n_params + 2 * ps.bn_total)))
        return
    off, on = engine(0.0), engine(0.9998)
    graphs = {"g_opt, ema_decay = 0": captured(off.optimizer_body), "g_opt, ema_decay = 0.9998": captured(on.optimizer_body),
              "mmd_ema_update alone": captured(lambda: ema_call(on))}
    times = {k: [] for k in graphs}
    for g in graphs.values():
        time_us(g)                   # warm-up
    for _ in range(ROUNDS):
        for k, g in graphs.items():
            times[k].append(time_us(g))
    ps = on.student.ps
    print("n_params %d, bn_total %d; %d rounds of %d replays, alternating; us per replay" % (ps.n_params, ps.bn_total, ROUNDS, REPLAYS))
    for k, v in times.items():
        print("%-28s median %8.2f  min %8.2f  max %8.2f" % (k, statistics.median(v), min(v), max(v)))
    assert int(on.ema_state[0].item()) > 0 and torch.isfinite(on.ema_flat).all()


if __name__ == "__main__":
    main()
