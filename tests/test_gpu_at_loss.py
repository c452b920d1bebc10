"""GPU: kd_loss = AttentionLoss / None on the HIP path - mmd_at_loss_multi against the reference's AttentionLoss() (tests/golden/loss_at_*),
its run-to-run determinism, the drop-in module, the whole step against golden_step's recipe with the swapped criterion, graph replay,
the refusals and train.py end to end."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mm_distillnet_amd import _lib
from mm_distillnet_amd.step import DistillEngine, StepConfig
from mm_distillnet_amd.synth import synth_inputs
from helpers import make_state, check_summary
from test_kd_criteria import at_case
from test_gpu_step import MODS, teacher_states, drop_scale_from, grad_checks, step_batch

call = _lib.call
DEV = "cuda"


def rows(f):  # [B,C,H,W] -> [B*H*W, C] on the device
    return f.permute(0, 2, 3, 1).contiguous().to(DEV)


def run_at(fs, fts, gscale=1.0):
    """all (level, teacher) pairs through mmd_at_loss_multi -> (loss [nt, nlev], da per level, student rows per level)"""
    B, nt, nlev = fs[0].shape[0], len(fts), len(fs)
    a_s, a_t, das, hw, frs = [], [[] for _ in fts], [], [], []
    for lvl, f in enumerate(fs):
        C, HW = f.shape[1], f.shape[2] * f.shape[3]
        fr = rows(f)
        a = torch.empty(B * HW, device=DEV)
        call("mmd_mta_attention", fr, a, B * HW, C, 2.0)
        a_s.append(a); hw.append(HW); frs.append(fr); das.append(torch.full((B * HW,), float("nan"), device=DEV))
        for k, ft in enumerate(fts):
            at = torch.empty(B * HW, device=DEV)
            call("mmd_mta_attention", rows(ft[lvl]), at, B * HW, C, 2.0)
            a_t[k].append(at)
    loss = torch.full((nt, nlev), float("nan"), device=DEV)
    vp = ctypes.c_void_p
    call("mmd_at_loss_multi", (vp * nlev)(*[t.data_ptr() for t in a_s]),
         (vp * (nt * nlev))(*[a_t[k][l].data_ptr() for k in range(nt) for l in range(nlev)]), (vp * nlev)(*[t.data_ptr() for t in das]),
         (ctypes.c_int * nlev)(*hw), nlev, nt, B, loss, gscale, torch.empty(nt * nlev * B, device=DEV))
    return loss, das, frs


def at_grads(fs, das, frs):
    out = []
    for f, da, fr in zip(fs, das, frs):
        B, C, H, W = f.shape
        df = torch.empty(B * H * W, C, device=DEV)
        call("mmd_mta_attention_bwd", fr, da, df, B * H * W, C, 2.0, 0)
        out.append(df.view(B, H, W, C).permute(0, 3, 1, 2).cpu())
    return out


def floor_of(ref):
    """absolute floor: 1 % of the smallest non-zero reference loss, so that it cannot pass a wrong small level"""
    nz = np.abs(ref[ref != 0])
    return 0.01 * float(nz.min())


def check_losses_and_grads(loss, dfs, gold, key_loss, key_grad):
    ref = gold[key_loss]
    np.testing.assert_allclose(loss, ref, rtol=1e-4, atol=floor_of(gold["loss"]))
    for i, df in enumerate(dfs):
        r = gold[f"{key_grad}{i}"]
        err = float(np.abs(df.numpy() - r).max())
        assert err <= 2e-3 * float(np.abs(r).max()), (i, err, float(np.abs(r).max()))


@pytest.mark.parametrize("name", ["stock", "wide", "zero"])
def test_at_kernel_golden(golden_dir, name):
    """one launch for 3 teachers x 5 levels: losses rtol 1e-4 (floor 1 % of the smallest non-zero golden loss), gradients (sum over the
    teachers) within 2e-3 of the largest reference value; a 1x1 level gives exactly 0 loss and 0 gradient"""
    gold = np.load(os.path.join(golden_dir, f"loss_at_{name}.npz"))
    fs, fts = at_case(gold)
    loss, das, frs = run_at(fs, fts)
    dfs = at_grads(fs, das, frs)
    loss = loss.cpu().numpy()
    print(name, "loss", loss, "golden", gold["loss"])
    check_losses_and_grads(loss, dfs, gold, "loss", "dfs")
    for lvl, f in enumerate(fs):
        if f.shape[2] * f.shape[3] == 1:
            zero = gold["loss"][:, lvl] == 0
            assert (loss[zero, lvl] == 0).all()
            if zero.all():
                assert (dfs[lvl] == 0).all()
    if name == "stock":
        assert (gold["loss"][:, 4] == 0).all()      # the 1x1 case is present


def test_at_kernel_bitwise_reproducible(golden_dir):
    gold = np.load(os.path.join(golden_dir, "loss_at_wide.npz"))
    fs, fts = at_case(gold)
    l1, d1, _ = run_at(fs, fts, 0.005)
    l2, d2, _ = run_at(fs, fts, 0.005)
    torch.cuda.synchronize()
    assert torch.equal(l1.view(torch.int32), l2.view(torch.int32))
    for a, b in zip(d1, d2):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_at_kernel_rejects_bad_arguments():
    dll = _lib.LIB.load()
    vp = ctypes.c_void_p
    one = (vp * 1)(1)
    hw = (ctypes.c_int * 1)(4)
    assert dll.mmd_at_loss_multi(None, one, None, hw, 1, 1, 2, 1, 1.0, 1, None) == -22
    assert dll.mmd_at_loss_multi(one, one, None, hw, 6, 1, 2, 1, 1.0, 1, None) == -22      # nlev > 5
    assert dll.mmd_at_loss_multi(one, one, None, hw, 1, 5, 2, 1, 1.0, 1, None) == -22      # nteachers > 4
    assert dll.mmd_at_loss_multi(one, one, None, hw, 1, 1, 0, 1, 1.0, 1, None) == -22      # B = 0
    assert dll.mmd_at_loss_multi(one, one, None, hw, 1, 1, 2, 1, 1.0, None, None) == -22   # no workspace


@pytest.mark.parametrize("name", ["stock", "wide", "zero"])
def test_attention_loss_module(golden_dir, name):
    """the drop-in module (one teacher per call, as ModelWithNMSLoss calls it) forward + backward against teacher 0 of the fixture"""
    from mm_distillnet_amd.model import AttentionLoss
    gold = np.load(os.path.join(golden_dir, f"loss_at_{name}.npz"))
    fs, fts = at_case(gold)
    fs = [f.to(DEV).requires_grad_(True) for f in fs]
    crit = AttentionLoss()
    loss = crit(fs, [t.to(DEV) for t in fts[0]])
    assert tuple(loss.shape) == (5,)
    loss.sum().backward()
    ref = gold["loss"][0]
    np.testing.assert_allclose(loss.detach().cpu().numpy(), ref, rtol=1e-4, atol=floor_of(gold["loss"]))
    for i, f in enumerate(fs):
        r = gold[f"t0_dfs{i}"]
        err = float(np.abs(f.grad.cpu().numpy() - r).max())
        assert err <= 2e-3 * float(np.abs(r).max()), (i, err)
    with pytest.raises(Exception, match="list of teachers"):
        crit(fs, [[t.to(DEV) for t in ft] for ft in fts])
    with pytest.raises(Exception, match="same shape"):
        crit(fs, [t.to(DEV) for t in fts[0][1:]] + [fts[0][0].to(DEV)])


def build(variant, kd_loss, S=256, p=2.0):
    mods = {"rgb": MODS["rgb"]} if variant == "rgb1" else MODS
    teachers = teacher_states(2, mods)
    spec_s, st_s = make_state(2, 8, 24, "audio")
    cfg = StepConfig(image_size=S, augment=variant == "augmented", kd_loss=kd_loss, p=p)
    eng = DistillEngine(spec_s, {k: v[0] for k, v in teachers.items()}, DEV, cfg)
    eng.load(st_s, {k: v[1] for k, v in teachers.items()})
    return eng, spec_s


@pytest.mark.parametrize("fixture", ["at_pairwise", "at_augmented", "at_rgb1", "nokd_pairwise"])
def test_step_golden_reference_labels_kd_criteria(golden_dir, fixture):
    """test_gpu_step.py::test_step_golden_reference_labels with kd_loss = AttentionLoss / None: the teachers' pseudo-labels from the
    reference run; loss scalars 2e-4, kd rtol 1e-4 (floor: 1 % of the smallest non-zero golden term), gradients 2e-3, Adam 1e-5 / 1e-4"""
    gold = np.load(os.path.join(golden_dir, f"step_d2_256_{fixture}.npz"))
    tag, variant = fixture.split("_")
    S, B = 256, 2
    eng, spec = build(variant, "AttentionLoss" if tag == "at" else "None", S)
    nt = len(eng.teachers)
    batch = step_batch(variant, B, S)
    ds = drop_scale_from(gold, spec)
    A = eng.student.anchors(S).shape[0]
    labels = eng.labels_from_rows([[gold[f"teacher{ti}_img{i}"] for i in range(B)] for ti in range(nt)], A)
    out = eng.step_body(batch, ds, teacher_labels=labels)
    torch.cuda.synchronize()
    eng.check_overflow()
    kd = out["kd"].cpu().numpy()
    print(fixture, "kd", kd, "golden", gold["kd"].reshape(-1))
    np.testing.assert_allclose(out["reg"].cpu().numpy(), gold["reg"], rtol=2e-4)
    np.testing.assert_allclose(out["cls"].cpu().numpy(), gold["cls"], rtol=2e-4)
    if tag == "nokd":
        assert (gold["kd"] == 0).all() and kd.shape == (nt, 5) and (kd == 0).all()
    else:
        np.testing.assert_allclose(kd, gold["kd"].reshape(kd.shape), rtol=1e-4, atol=floor_of(gold["kd"]))
    loss = 1.0 * (out["reg"].item() + out["cls"].item()) + 0.005 * out["kd"].sum().item()
    assert abs(loss - float(gold["loss"])) < 2e-4 * abs(float(gold["loss"]))
    grad_checks(gold, eng.student.ps.export_grads(), 2e-3, 2e-3, 2e-3)
    eng.optimizer_body()
    torch.cuda.synchronize()
    params = eng.student.ps.export_state()
    for k in gold.files:
        if k.startswith("adam.") and k.endswith(".head"):
            name = k[5:-5]
            check_summary(gold, "adam." + name, params[name], 1e-5, 1e-4)


def test_attention_loss_ignores_cfg_p():
    """the criterion's p is 2 whatever cfg p says: p = 3 gives the p = 2 step (eager-vs-eager noise of test_graph_replay_matches_eager)"""
    S, B = 128, 2
    batch = {k: v.to(DEV) for k, v in synth_inputs(B, S, seed=5).items()}
    eng_a, _ = build("pairwise", "AttentionLoss", S, p=2.0)
    eng_b, _ = build("pairwise", "AttentionLoss", S, p=3.0)
    ds = eng_a.make_drop_scale(B, torch.Generator(device=DEV).manual_seed(1))
    oa = eng_a.step_body(batch, ds)
    ob = eng_b.step_body(batch, ds)
    torch.cuda.synchronize()
    assert (oa["kd"] != 0).any()
    np.testing.assert_allclose(oa["kd"].cpu().numpy(), ob["kd"].cpu().numpy(), rtol=1e-4, atol=1e-6)
    ga, gb = eng_a.student.ps.grad, eng_b.student.ps.grad
    assert (ga - gb).abs().max().item() <= 2e-3 * ga.abs().max().item()


@pytest.mark.parametrize("kd_loss", ["AttentionLoss", "None"])
def test_graph_replay_matches_eager_kd_criteria(kd_loss):
    """test_gpu_step.py::test_graph_replay_matches_eager for the other criteria"""
    S, B = 128, 2
    batch = {k: v.to(DEV) for k, v in synth_inputs(B, S, seed=5).items()}
    eng_a, _ = build("pairwise", kd_loss, S)
    eng_b, _ = build("pairwise", kd_loss, S)
    ds = eng_a.make_drop_scale(B, torch.Generator(device=DEV).manual_seed(1))
    eng_b.capture(batch)
    oa = eng_a.step_body(batch, ds)
    eng_b.set_drop_scale(ds)
    eng_b.g_main.replay()
    torch.cuda.synchronize()
    ob = eng_b.out
    assert oa["nbox"].tolist() == ob["nbox"].tolist()
    for k in ("reg", "cls", "kd"):
        np.testing.assert_allclose(oa[k].cpu().numpy(), ob[k].cpu().numpy(), rtol=1e-4, atol=1e-6)
    assert ((ob["kd"] == 0).all() if kd_loss == "None" else (ob["kd"] != 0).any())
    ga, gb = eng_a.student.ps.grad, eng_b.student.ps.grad
    assert torch.isfinite(gb).all()
    assert (ga - gb).abs().max().item() <= 2e-3 * ga.abs().max().item()
    eng_a.optimizer_body(); eng_b.g_opt.replay()
    torch.cuda.synchronize()
    assert eng_a.adam_main[0].item() == eng_b.adam_main[0].item() == 1.0
    for _ in range(2):
        eng_b.replay(batch, ds)
    torch.cuda.synchronize()
    assert eng_b.out["nbox"].tolist() == oa["nbox"].tolist()
    assert torch.isfinite(eng_b.student.ps.flat).all() and eng_b.adam_main[0].item() == 3.0
    # validate() path: eval-mode losses through the same step body
    reg, cls, kd = eng_b.eval_losses(batch)
    assert np.isfinite(reg) and np.isfinite(cls) and ((kd == 0.0) if kd_loss == "None" else (kd > 0.0))


def test_engine_refuses_attention_loss_with_kdlist():
    spec_s, _ = make_state(2, 8, 24, "audio")
    t = teacher_states(2, {"rgb": MODS["rgb"]})
    with pytest.raises(Exception, match="kdlist"):
        DistillEngine(spec_s, {k: v[0] for k, v in t.items()}, DEV, StepConfig(image_size=128, kd_mode="list", kd_loss="AttentionLoss"))


def test_train_main_kd_loss(tmp_path, monkeypatch):
    """train.py --overwrite '{"kd_loss": ...}' end to end: AttentionLoss trains with a non-zero KD term other than MTA's, None with none"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.chdir(tmp_path)
    sys.path.insert(0, root)
    import train
    cfgf = os.path.join(root, "configs", "mm-distillnet.cfg")
    kd = {}
    for name, extra in (("at", ', "kd_loss": "AttentionLoss"'), ("none", ', "kd_loss": "None"'), ("mta", "")):
        ov = ('{"image_size": 128, "batch_size": 2, "synthetic_length": 8, "num_epoches": 1, "exp_name": "exp_%s", "resume": "False", '
              '"num_workers": 0, "no_validation": "True"%s}' % (name, extra))
        loss = train.main(["--config_file", cfgf, "--overwrite", ov, "--max_steps", "3"])
        assert np.isfinite(loss)
        logs = json.load(open(tmp_path / f"exp_{name}" / "all_logs.0.json"))
        kd[name] = [v for _, _, v in logs[f"exp_{name}/Train/KD"]]
    print("Train/KD", kd)
    assert kd["none"] and all(v == 0.0 for v in kd["none"])
    assert kd["at"] and all(v > 0.0 for v in kd["at"])
    assert len(kd["at"]) == len(kd["mta"]) and all(a != m for a, m in zip(kd["at"], kd["mta"]))
