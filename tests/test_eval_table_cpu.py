"""CPU: the C ABI of csrc/evaltable.hip (mmd_sort_tile, mmd_sort_desc_ws_bytes, mmd_sort_desc_f32, mmd_eval_table_ws_bytes, mmd_eval_table)
without a GPU - signatures, refused arguments, workspace sizes - and the float64 reference the GPU tests hold the kernels to
(tests/evaltable_ref.py) against the project's host path, metrics.table_from_stats / ap_per_class, wherever that path is well defined:
on records without score ties."""
import ctypes

import numpy as np
import pytest

import evaltable_ref as R
from mm_distillnet_amd import metrics as M

P, LL, F = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_float
SIGS = {"mmd_sort_tile": [],
        "mmd_sort_desc_ws_bytes": [LL],
        "mmd_sort_desc_f32": [P, P, LL, P, P, P, P],
        "mmd_eval_table_ws_bytes": [LL, LL],
        "mmd_eval_table": [P, P, LL, P, LL, P, LL, F, P, P, P, P]}


@pytest.fixture(scope="module")
def dll():
    import __graft_entry__ as ge
    ge.build()
    from mm_distillnet_amd import _lib
    return _lib.LIB.load()


def test_header_declares_the_entry_points(dll):
    from mm_distillnet_amd import _lib
    sigs = _lib.LIB.symbols()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, types in SIGS.items():
        assert sigs.get(name) == types, name
        assert hasattr(raw, name), name


def test_sizes(dll):
    T = dll.mmd_sort_tile()
    assert T > 0 and T % 64 == 0
    ns = [0, 1, 63, 64, T - 1, T, T + 1, 3 * T + 17, 65536, 1 << 20, 1 << 24]
    ws = [dll.mmd_sort_desc_ws_bytes(n) for n in ns]
    assert all(w > 0 for w in ws) and ws == sorted(ws)
    # two key and two index buffers of n items each, and a counter per digit value and block
    assert all(w >= 16 * n + 1024 * ((n + T - 1) // T) for w, n in zip(ws, ns))
    tw = [dll.mmd_eval_table_ws_bytes(n, 100) for n in ns]
    assert all(t > w for t, w in zip(tw, ws)) and tw == sorted(tw)
    assert dll.mmd_eval_table_ws_bytes(1000, 0) <= dll.mmd_eval_table_ws_bytes(1000, 1 << 20)
    for bad in (-1, 1 << 31, 1 << 40):
        assert dll.mmd_sort_desc_ws_bytes(bad) == -22
        assert dll.mmd_eval_table_ws_bytes(bad, 1) == -22 and dll.mmd_eval_table_ws_bytes(1, bad) == -22


def test_sort_refuses_bad_arguments_without_gpu(dll):
    p = 4096            # never dereferenced: validation precedes any launch
    f = dll.mmd_sort_desc_f32
    assert f(p, None, 0, p, p, p, None) == 0 and f(None, None, 0, None, p, p, None) == 0      # n = 0: nothing to do
    assert f(p, p, 0, p, p, p, None) == 0
    for args in ((None, None, 8, p, p, p), (p, None, 8, None, p, p), (p, None, 8, p, None, p), (p, None, 8, p, p, None),
                 (p, None, 0, p, None, p), (p, None, 0, p, p, None),
                 (p, None, -1, p, p, p), (p, None, 1 << 31, p, p, p), (p, None, 1 << 40, p, p, p),
                 (p + 2, None, 8, p, p, p), (p, p + 1, 8, p, p, p), (p, None, 8, p + 2, p, p), (p, None, 8, p, p + 8, p), (p, None, 8, p, p, p + 1)):
        assert f(*args, None) == -22, args


def test_table_refuses_bad_arguments_without_gpu(dll):
    p = 4096
    f = dll.mmd_eval_table
    good = dict(rows=p, tp=p, n_rows=10, cd=p, n_img=3, gt=p, n_gt=5, S=256.0, out=p, ws=p, status=p)
    for bad in (dict(rows=None), dict(tp=None), dict(cd=None), dict(gt=None), dict(out=None), dict(ws=None), dict(status=None),
                dict(n_rows=-1), dict(n_img=-1), dict(n_gt=-1), dict(n_rows=1 << 31), dict(n_gt=1 << 31), dict(n_img=1 << 31),
                dict(rows=p + 2), dict(tp=p + 1), dict(cd=p + 3), dict(gt=p + 2), dict(out=p + 4), dict(ws=p + 8), dict(status=p + 2),
                dict(n_rows=0, out=None), dict(n_rows=0, n_img=0, n_gt=0, ws=None)):
        a = dict(good, **bad)
        assert f(a["rows"], a["tp"], a["n_rows"], a["cd"], a["n_img"], a["gt"], a["n_gt"], a["S"], a["out"], a["ws"], a["status"], None) == -22, bad


def test_sort_order_reference():
    """the restated order on a case small enough to read"""
    key = np.array([0.5, np.nan, -0.0, 0.5, np.inf, 0.0, -np.inf, 1e-45, -np.nan], np.float32)
    assert R.sort_order(key).tolist() == [4, 0, 3, 7, 2, 5, 6, 1, 8]
    cls = np.array([1, 0, 1, 0, 1, 0, 0, 1, 0], np.float32)
    assert R.sort_order(key, cls).tolist() == [3, 5, 6, 1, 8, 4, 0, 7, 2]


@pytest.mark.parametrize("name", ["empty", "one_class_all_tp", "one_class_all_fp", "missing_and_extra_class", "random_masks",
                                  "two_classes_across_tiles", "images_without_boxes"])
def test_reference_equals_host_path_without_ties(name):
    stats, tie_free = R.records(2048)[name]
    assert tie_free
    want, got = M.table_from_stats(stats, 256), R.table_ref(stats, 256)
    for k in ("AP@Ave", "AP@0.5", "AP@0.75"):
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), (k, got[k], want[k])
    for k in ("CDx", "CDy"):          # the host averages the float32 quotients in float32
        assert abs(got[k] - want[k]) <= 1e-5 * abs(want[k]), (k, got[k], want[k])
    if stats["score"].size:
        p, r, ap, f1, classes, _ = M.ap_per_class((stats["tp"] & 1).astype(np.float64), stats["score"], stats["label"], stats["gt"])
        per = got["per_class"]
        np.testing.assert_array_equal(per[:, 0], classes)
        np.testing.assert_array_equal(per[:, 1], np.unique(stats["gt"], return_counts=True)[1])
        np.testing.assert_array_equal(per[:, 2], [(stats["label"] == c).sum() for c in classes])
        for col, ref in ((3, p), (4, r), (5, ap), (6, f1)):
            np.testing.assert_allclose(per[:, col], ref, rtol=1e-12, atol=0)


def test_reference_ranks_equal_scores_in_record_order():
    """two predictions of one score, the true positive second: record order puts the false positive first"""
    stats = {"score": np.array([0.5, 0.5], np.float32), "label": np.zeros(2, np.float32), "tp": np.array([0, 511], np.int32),
             "cd": np.array([[1, 1, 1]], np.float32), "gt": np.zeros(1, np.float32)}
    assert R.table_ref(stats, 256)["AP@0.5"] == 50.0
    stats["tp"] = stats["tp"][::-1].copy()
    assert R.table_ref(stats, 256)["AP@0.5"] == 100.0
