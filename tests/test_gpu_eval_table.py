"""GPU: csrc/evaltable.hip against the float64 restatements of tests/evaltable_ref.py (which tests/test_eval_table_cpu.py ties to the
host path): the stable radix sort mmd_sort_desc_f32 permutation for permutation, the AP / CD table mmd_eval_table through
metrics.table_from_record_device, and DistillEngine.end_eval_table on the engine of tests/test_gpu_eval_engine.py.

Tolerances: both sides do the same float64 operations per class and differ in the order of one sum of at most n terms of size <= 1
(n * 2^-53 ~ 5e-13 at the largest record here), so the AP entries hold 1e-7 absolute on the percent scale and the per-class rows 1e-9;
counts are exact; CDx / CDy hold 1e-5 relative against the host's float32 pairwise mean (off by about log2(n) * 2^-24)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import evaltable_ref as R
from mm_distillnet_amd import _lib
from mm_distillnet_amd import metrics as M

DEV = "cuda"
S = 256


def tile():
    return int(_lib.LIB.load().mmd_sort_tile())


def sizes():
    T = tile()
    return [1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 17]


def keys_of(kind, n, rng):
    if kind == "random":
        return (rng.standard_normal(n) * np.float32(10.0) ** rng.integers(-3, 4, n)).astype(np.float32)
    if kind == "special":
        vals = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, np.inf, -np.inf, 1.0, -1.0, 3.4e38, -3.4e38], np.float32)
        return rng.choice(vals, n)
    if kind == "four":
        return rng.choice(np.array([0.25, -3.0, 0.0, 7.5], np.float32), n)
    k = rng.standard_normal(n).astype(np.float32)
    nans = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xffffffff], np.uint32).view(np.float32)
    hit = rng.random(n) < 0.3
    k[hit] = rng.choice(nans, int(hit.sum()))
    return k


@pytest.mark.parametrize("n_cls", [0, 3, 20])
@pytest.mark.parametrize("kind", ["random", "special", "four", "nan"])
def test_sort_equals_the_stable_order(kind, n_cls):
    rng = np.random.default_rng(11 + n_cls)
    for n in sizes():
        key = keys_of(kind, n, rng)
        cls = rng.choice(np.array([0, 7, 255] if n_cls == 3 else np.arange(n_cls) * 13, np.float32), n) if n_cls else None
        perm = M.sort_desc_device(torch.from_numpy(key).to(DEV), None if cls is None else torch.from_numpy(cls).to(DEV)).cpu().numpy()
        np.testing.assert_array_equal(perm, R.sort_order(key, cls), err_msg="%s n = %d classes = %d" % (kind, n, n_cls))


@pytest.mark.parametrize("bad", [256.0, 1.5, -1.0, float("nan")])
def test_sort_flags_a_class_outside_the_range(bad):
    n = tile() + 5
    key = torch.rand(n, device=DEV)
    cls = torch.zeros(n, device=DEV)
    cls[n - 2] = bad
    ws = torch.empty(int(_lib.LIB.load().mmd_sort_desc_ws_bytes(n)), dtype=torch.uint8, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    perm = torch.empty(n, dtype=torch.int32, device=DEV)
    _lib.call("mmd_sort_desc_f32", key, cls, n, perm, ws, status)
    assert int(status.item()) & 1
    assert sorted(perm.cpu().tolist()) == list(range(n))          # unspecified order, still a permutation
    with pytest.raises(RuntimeError, match="0 .. 255"):
        M.sort_desc_device(key, cls)
    status.zero_()
    _lib.call("mmd_sort_desc_f32", key, None, n, perm, ws, status)      # without classes nothing is flagged
    assert int(status.item()) == 0


def check_table(got, stats, tie_free):
    want = R.table_ref(stats, S)
    assert set(got) == {"AP@Ave", "AP@0.5", "AP@0.75", "CDx", "CDy", "per_class"}
    host = M.table_from_stats(stats, S)
    for k in ("AP@Ave", "AP@0.5", "AP@0.75"):
        print(k, got[k], want[k], host[k])
        assert abs(got[k] - want[k]) <= 1e-7, (k, got[k], want[k])
        if tie_free:
            assert abs(got[k] - host[k]) <= 1e-7, (k, got[k], host[k])
    for k in ("CDx", "CDy"):
        print(k, got[k], host[k])
        assert abs(got[k] - host[k]) <= 1e-5 * abs(host[k]), (k, got[k], host[k])
    per, ref = got["per_class"], want["per_class"]
    assert per.shape == ref.shape and per.dtype == np.float64
    np.testing.assert_array_equal(per[:, :3], ref[:, :3])           # class, n_gt, n_pred
    np.testing.assert_allclose(per[:, 3:], ref[:, 3:], rtol=0, atol=1e-9)
    return want


@pytest.mark.parametrize("name", ["empty", "one_class_all_tp", "one_class_all_fp", "missing_and_extra_class", "random_masks",
                                  "two_classes_across_tiles", "images_without_boxes", "heavy_ties"])
def test_table_equals_the_reference(name):
    stats, tie_free = R.records(tile())[name]
    got = M.table_from_record_device(stats, S, DEV)
    check_table(got, stats, tie_free)
    if name == "empty":
        assert got["AP@Ave"] == 0.0 and got["CDx"] == 10000.0 and got["CDy"] == 10000.0
        np.testing.assert_array_equal(got["per_class"], [[2, 1, 0, 0, 0, 0, 0], [6, 2, 0, 0, 0, 0, 0]])


def test_table_mean_aps_and_every_element_of_out():
    """the nine mean APs of out[0..8], and a dirty `out` / workspace: every element is written"""
    stats, _ = R.records(tile())["random_masks"]
    rows = torch.from_numpy(np.stack([stats["score"], stats["label"]], 1)).to(DEV)
    tp, cd, gt = (torch.from_numpy(stats[k]).to(DEV) for k in ("tp", "cd", "gt"))
    nb = int(_lib.LIB.load().mmd_eval_table_ws_bytes(rows.shape[0], gt.shape[0]))
    outs = []
    for fill in (0x00, 0xff):
        ws = torch.full((nb,), fill, dtype=torch.uint8, device=DEV)
        out = torch.full((M.TABLE_OUT,), float("nan") if fill else 123.0, dtype=torch.float64, device=DEV)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        _lib.call("mmd_eval_table", rows, tp, rows.shape[0], cd, cd.shape[0], gt, gt.shape[0], float(S), out, ws, status)
        assert int(status.item()) == 0
        outs.append(out.cpu().numpy())
    np.testing.assert_array_equal(outs[0], outs[1])
    want = R.table_ref(stats, S)
    np.testing.assert_allclose(outs[0][:9], want["mean_ap"], rtol=0, atol=1e-9)
    assert outs[0][14] == 4 and outs[0][15] == 0
    absent = np.setdiff1d(np.arange(256), [0, 3, 6, 255])
    assert not outs[0][16:].reshape(256, 8)[absent].any()


@pytest.mark.parametrize("bad", [256.0, 2.5])
def test_table_flags_a_label_outside_the_range(bad):
    stats, _ = R.records(tile())["one_class_all_tp"]
    for field in ("gt", "label"):
        s = {k: v.copy() for k, v in stats.items()}
        s[field][3] = bad
        with pytest.raises(RuntimeError, match="label range 0 .. 255"):
            M.table_from_record_device(s, S, DEV)


def test_engine_end_eval_table(golden_dir):
    """one evaluation judged both ways (the engine and batches of tests/test_gpu_eval_engine.py), and end_eval's raises"""
    from mm_distillnet_amd.arch import make_spec
    from mm_distillnet_amd.step import DistillEngine, StepConfig
    from mm_distillnet_amd.synth import synth_inputs
    from test_oracle_golden import val_states
    g = np.load(os.path.join(golden_dir, "validate_d2_256.npz"))
    size, N, B = int(g["image_size"]), int(g["n"]), int(g["batch"])
    tstates, spec, st_s = val_states()
    eng = DistillEngine(spec, {"rgb": make_spec(2, 3), "depth": make_spec(2, 3), "thermal": make_spec(2, 1)}, DEV, StepConfig(image_size=size))
    eng.load(st_s, tstates)
    data = synth_inputs(N, size, seed=61)
    batches = [{k: v[b * B:(b + 1) * B].to(DEV) for k, v in data.items()} for b in range(N // B)]
    eng.begin_eval(N, 1 << 14)
    for batch in batches:
        eng.eval_batch(batch)
    table, stats = eng.end_eval_table(size, with_record=True)
    assert stats["score"].size > 1 and stats["gt"].size > 0 and table["AP@0.5"] > 0, "the comparison needs detections and pseudo ground truth"
    want = R.table_ref(stats, size)
    for k in ("AP@Ave", "AP@0.5", "AP@0.75"):
        assert abs(table[k] - want[k]) <= 1e-7, (k, table[k], want[k])
    host = M.table_from_stats(stats, size)
    for k in ("CDx", "CDy"):
        assert abs(table[k] - host[k]) <= 1e-5 * abs(host[k]), (k, table[k], host[k])
    np.testing.assert_array_equal(table["per_class"][:, :3], want["per_class"][:, :3])
    np.testing.assert_allclose(table["per_class"][:, 3:], want["per_class"][:, 3:], rtol=0, atol=1e-9)
    # without with_record only the table comes back; a record one row too small raises, and an evaluation cannot end twice
    eng.begin_eval(N, stats["score"].size - 1, stats["gt"].size)
    for batch in batches:
        eng.eval_batch(batch)
    with pytest.raises(RuntimeError, match="evaluation record capacity exceeded"):
        eng.end_eval_table(size)
    with pytest.raises(RuntimeError, match="end_eval_table without begin_eval"):
        eng.end_eval_table(size)
