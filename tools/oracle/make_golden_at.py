#!/usr/bin/env python3
"""Generate the AttentionLoss fixtures under tests/golden/ by running the REFERENCE's own modules (build container only).

    python tools/oracle/make_golden_at.py            # writes tests/golden/loss_at_*.npz, step_d2_256_{at_*,nokd_pairwise}.npz

Same recipes as tools/oracle/make_golden.py (imported, not edited): the reference's `AttentionLoss()` (src/loss/AttentionLoss.py,
built with its default p = 2 as the reference's factory does) on random maps, and golden_step's whole-step recipe with
`AttentionLoss()` or `criterion_kd = None` in place of `MTALoss`.
"""
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (installs the reference shim, 8 torch threads)

from src.loss.AttentionLoss import AttentionLoss  # noqa: E402

OUT = MG.OUT

# loss fixtures: name -> (generator seed, image count, map sizes, channels, stored inputs?)
#   stock: the loss_mta_stock shapes; wide: levels above 4096 pixels and not powers of two (inputs regenerated from the seed in the
#   tests: stored they would pass the committed-file size limit); zero: stock shapes, teacher 1's image 0 all zeros (F.normalize's clamp)
AT_CASES = {"stock": (17, 2, (16, 8, 4, 2, 1), 12, True),
            "wide": (29, 3, (80, 40, 20, 10, 5), 4, False),
            "zero": (23, 2, (16, 8, 4, 2, 1), 12, True)}


def at_inputs(name):
    """student maps [5] and three teachers' maps [3][5], [B, C, s, s] fp32 (tests/test_kd_criteria.py repeats this)"""
    seed, B, sizes, C, _ = AT_CASES[name]
    g = torch.Generator().manual_seed(seed)
    fs = [torch.randn(B, C, s, s, generator=g) for s in sizes]
    fts = [[torch.randn(B, C, s, s, generator=g) * (0.5 + k) for s in sizes] for k in range(3)]
    if name == "zero":
        for f in fts[1]:
            f[0] = 0.0
    return fs, fts


def golden_at_losses():
    for name, (seed, B, sizes, C, stored) in AT_CASES.items():
        fs, fts = at_inputs(name)
        fs = [f.requires_grad_(True) for f in fs]
        crit = AttentionLoss()
        assert crit.p == 2
        d = {"seed": np.int64(seed), "B": np.int64(B), "C": np.int64(C), "sizes": np.array(sizes, dtype=np.int64)}
        for i, f in enumerate(fs):
            if stored:
                d[f"fs{i}"] = f.detach().numpy().copy()
            else:
                MG.put(d, f"fs{i}", f)
        for k, ft in enumerate(fts):
            for i, f in enumerate(ft):
                if stored:
                    d[f"ft{k}_{i}"] = f.numpy().copy()
                else:
                    MG.put(d, f"ft{k}_{i}", f)
        # per teacher, as ModelWithNMSLoss calls it: loss[t] = criterion(features_s, features_t) -> [5]
        losses = []
        for k, ft in enumerate(fts):
            lk = crit(fs, ft)
            losses.append(lk.detach())
            if k == 0:        # teacher 0 alone: the drop-in module's backward
                lk.sum().backward()
                for i, f in enumerate(fs):
                    d[f"t0_dfs{i}"] = f.grad.numpy().copy(); f.grad = None
        d["loss"] = torch.stack(losses).numpy()
        # the step's KD term: sum over teachers and levels (gradient of the sum)
        sum(crit(fs, ft).sum() for ft in fts).backward()
        for i, f in enumerate(fs):
            d[f"dfs{i}"] = f.grad.numpy().copy(); f.grad = None
        np.savez_compressed(os.path.join(OUT, f"loss_at_{name}.npz"), **d)
        print("at", name, d["loss"])


def golden_at_steps():
    """golden_step's recipe, its KD criterion swapped: the fixtures carry golden_step's keys"""
    tmp = tempfile.mkdtemp()
    saved = MG.OUT, MG.MTALoss, os.environ.get("GOLDEN_STEP_VARIANTS")
    try:
        MG.OUT = tmp
        for tag, factory, variants in (("at", lambda T, p: AttentionLoss(), "pairwise,augmented,rgb1"),
                                       ("nokd", lambda T, p: None, "pairwise")):
            MG.MTALoss = factory
            os.environ["GOLDEN_STEP_VARIANTS"] = variants
            MG.golden_step()
            for v in variants.split(","):
                shutil.move(os.path.join(tmp, f"step_d2_256_{v}.npz"), os.path.join(OUT, f"step_d2_256_{tag}_{v}.npz"))
    finally:
        MG.OUT, MG.MTALoss = saved[0], saved[1]
        if saved[2] is None:
            os.environ.pop("GOLDEN_STEP_VARIANTS", None)
        else:
            os.environ["GOLDEN_STEP_VARIANTS"] = saved[2]
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    which = sys.argv[1:] or ["losses", "step"]
    if "losses" in which:
        golden_at_losses()
    if "step" in which:
        golden_at_steps()
