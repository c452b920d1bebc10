"""CPU: the host restatements of the weighted box fusion (tests/wbf_ref.py) against cases worked out by hand and against each other, and the
host side of cfg `label_merge` / `label_merge_votes`: StepConfig's checks, train.py's keys, the header's declaration."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

import wbf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "mm-distillnet.cfg")
F = np.float32


def rows(*r):
    return np.array(r, dtype=F).reshape(-1, 6)


NONE = rows()


def test_two_boxes_round_weights():
    """weights 0.75 and 0.25 (W = 1): IoU = 32 / 96 > 0.3; x1 = 0 * .75 + 4 * .25 = 1, x2 = 8 * .75 + 12 * .25 = 9"""
    a, b = rows([0, 0, 8, 8, 0.75, 1]), rows([4, 0, 12, 8, 0.25, 1])
    r = R.wbf_f32([[a], [b]], 1, 0.3)
    assert r.boxes[0].dtype == F and r.aux[0].dtype == F
    assert r.boxes[0].tolist() == [[1, 0, 9, 8, 1]] and r.aux[0].tolist() == [[0.5, 2, 2]] and r.members == [[[0, 1]]]
    assert not r.overflow
    # the same pair at a threshold above 1 / 3: two clusters, each a lone box, in score order
    r = R.wbf_f32([[b], [a]], 1, 0.35)
    assert r.boxes[0].tolist() == [[0, 0, 8, 8, 1], [4, 0, 12, 8, 1]] and r.aux[0].tolist() == [[0.75, 1, 1], [0.25, 1, 1]]
    assert r.members == [[[1], [0]]]


def test_three_boxes_round_weights():
    """weights 0.5, 0.25, 0.25 (W = 1).  A + B: IoU 48 / 80 = 0.6 -> fused (2/3, 0, 8 2/3, 8); C against it: 7 1/3 * 6 = 44 over
    64 + 64 - 44 = 84 -> 0.52 > 0.5.  Sums: x1 = .5, y1 = .5, x2 = 4 + 2.5 + 2 = 8.5, y2 = 4 + 2 + 2.5 = 8.5"""
    a, b, c = rows([0, 0, 8, 8, 0.5, 0]), rows([2, 0, 10, 8, 0.25, 0]), rows([0, 2, 8, 10, 0.25, 0])
    r = R.wbf_f32([[a], [b], [c]], 1, 0.5)
    assert r.boxes[0].tolist() == [[0.5, 0.5, 8.5, 8.5, 0]] and r.members == [[[0, 1, 2]]]
    assert r.aux[0].tolist() == [[float(F(1) / F(3)), 3, 3]]
    # C alone against A: 48 / 80 as well - but with B of another source list the order of equal scores is the gather order
    r2 = R.wbf_f32([[a], [c], [b]], 1, 0.5)
    assert r2.members == [[[0, 1, 2]]] and r2.boxes[0].tolist() == [[0.5, 0.5, 8.5, 8.5, 0]]


def test_labels_do_not_mix():
    a, b = rows([0, 0, 8, 8, 0.75, 1]), rows([0, 0, 8, 8, 0.25, 2])
    r = R.wbf_f32([[a], [b]], 1, 0.3)
    assert r.boxes[0].tolist() == [[0, 0, 8, 8, 1], [0, 0, 8, 8, 2]] and r.aux[0][:, 1].tolist() == [1, 1]


def test_tie_goes_to_the_lowest_cluster():
    """(2, 0, 8, 4) overlaps (0, 0, 4, 4) and (6, 0, 10, 4) by 8 of 16 + 24 - 8 = 32 each: IoU 0.25 twice, cluster 0 takes it"""
    left, right, mid = [0, 0, 4, 4, 0.5, 0], [6, 0, 10, 4, 0.25, 0], [2, 0, 8, 4, 0.125, 0]
    r = R.wbf_f32([[rows(left, right, mid)]], 1, 0.2)
    assert r.members == [[[0, 2], [1]]]
    r = R.wbf_f32([[rows(right, left, mid)]], 1, 0.2)          # the clusters are born in score order, whatever the row order
    assert r.members == [[[1, 2], [0]]]
    # inclusive decides at IoU == thr exactly
    assert R.wbf_f32([[rows(left, right, mid)]], 1, 0.25).members == [[[0], [1], [2]]]
    assert R.wbf_f32([[rows(left, right, mid)]], 1, 0.25, inclusive=True).members == [[[0, 2], [1]]]


def test_min_votes_counts_distinct_sources():
    a, b, lone = [0, 0, 8, 8, 0.75, 1], [4, 0, 12, 8, 0.25, 1], [100, 100, 120, 120, 0.9, 1]
    # the pair from two sources, the lone box from source 0
    srcs = [[rows(a, lone)], [rows(b)]]
    assert [len(R.wbf_f32(srcs, 1, 0.3, min_votes=v).boxes[0]) for v in (1, 2)] == [2, 1]
    assert R.wbf_f32(srcs, 1, 0.3, min_votes=2).boxes[0].tolist() == [[1, 0, 9, 8, 1]]
    # the same pair from ONE source: two members, one vote
    r = R.wbf_f32([[rows(a, b)], [NONE]], 1, 0.3, min_votes=2)
    assert len(r.boxes[0]) == 0 and r.boxes[0].shape == (0, 5)
    assert R.wbf_f32([[rows(a, b)], [NONE]], 1, 0.3).aux[0].tolist() == [[0.5, 2, 1]]


def test_merge01_and_capacities():
    p, q = [0, 0, 8, 8, 0.75, 1], [4, 0, 12, 8, 0.25, 1]
    # image 1 takes image 0's rows in front of its own when it has rows itself; image 0 and every later image keep theirs
    r = R.wbf_f32([[rows(p), rows(q), rows(p)]], 3, 0.3, merge01=True)
    assert [b.tolist() for b in r.boxes] == [[[0, 0, 8, 8, 1]], [[1, 0, 9, 8, 1]], [[0, 0, 8, 8, 1]]]
    assert r.members[1] == [[0, 1]]
    assert [len(b) for b in R.wbf_f32([[rows(p), NONE]], 2, 0.3, merge01=True).boxes] == [1, 0]      # image 1 empty: stays empty
    assert [len(b) for b in R.wbf_f32([[NONE, rows(q)]], 2, 0.3, merge01=True).boxes] == [0, 1]
    assert [len(b) for b in R.wbf_f32([[rows(p)]], 1, 0.3, merge01=True).boxes] == [1]                # B = 1: ignored
    # source indices travel with image 0's rows: two sources, one vote each, merged into image 1
    r = R.wbf_f32([[rows(p), NONE], [NONE, rows(q)]], 2, 0.3, merge01=True, min_votes=2)
    assert [len(b) for b in r.boxes] == [0, 1] and r.aux[1].tolist() == [[0.5, 2, 2]]
    # max_boxes cuts in birth order and raises the flag; 1025 rows are cut to the first 1024 in gather order
    three = rows([0, 0, 1, 1, 0.5, 0], [2, 0, 3, 1, 0.75, 0], [4, 0, 5, 1, 0.25, 0])
    r = R.wbf_f32([[three]], 1, 0.5, max_boxes=2)
    assert r.overflow and r.boxes[0][:, 0].tolist() == [2, 0]
    many = np.zeros((1025, 6), F)
    many[:, 0] = np.arange(1025) * 2; many[:, 2] = many[:, 0] + 1; many[:, 3] = 1; many[:, 4] = 0.5
    many[:, 5] = np.arange(1025) % 64          # (64 labels: a row is compared with a 64th of the clusters, which keeps this quick)
    r = R.wbf_f32([[many]], 1, 0.5)
    assert r.overflow and len(r.boxes[0]) == 1024 and r.boxes[0][-1, 0] == 2046


@pytest.mark.parametrize("seed,nsrc,thr,inclusive,merge01", [(1, 3, 0.5, False, False), (2, 4, 0.55, True, True), (3, 2, 0.4, False, True),
                                                             (4, 1, 0.5, False, False)])
def test_f32_against_f64_on_clear_scenes(seed, nsrc, thr, inclusive, merge01):
    S, B = 512.0, 3
    srcs, ref = R.clear_scene(seed, B, nsrc, thr, inclusive, merge01, S)
    assert ref.margin > 1e-3
    got = R.wbf_f32(srcs, B, thr, inclusive, merge01)
    assert got.members == ref.members and sum(len(m) for m in got.members) > 0
    assert max(len(k) for m in got.members for k in m) >= min(2, nsrc)          # something was fused
    for b in range(B):
        assert np.array_equal(got.boxes[b][:, 4], ref.boxes[b][:, 4]) and np.array_equal(got.aux[b][:, 1:], ref.aux[b][:, 1:])
        for k, m in enumerate(got.members[b]):
            assert np.abs(got.boxes[b][k, :4] - ref.boxes[b][k, :4]).max() <= R.coordinate_bound(len(m), S), (b, k, len(m))
            assert abs(got.aux[b][k, 0] - ref.aux[b][k, 0]) <= (len(m) + 1) * 2.0 ** -24
    # the same scene again: the generator is a function of the seed
    again, _ = R.clear_scene(seed, B, nsrc, thr, inclusive, merge01, S)
    assert all(np.array_equal(x, y) for s, t in zip(srcs, again) for x, y in zip(s, t))


# ---------------------------------------------------------------- cfg keys and StepConfig
def test_step_config_label_merge():
    from mm_distillnet_amd.step import StepConfig
    sc = StepConfig()
    assert sc.label_merge == "nms" and sc.label_merge_votes == 1
    sc = StepConfig(label_merge="wbf", label_merge_votes=3)
    assert sc.label_merge == "wbf" and sc.label_merge_votes == 3
    for bad in ("soft", "WBF", "", None, 1):
        with pytest.raises(ValueError, match="label_merge"):
            StepConfig(label_merge=bad)
    for bad in (0, 5, -1, 1.0, "2", None, True):
        with pytest.raises(ValueError, match="label_merge_votes"):
            StepConfig(label_merge="wbf", label_merge_votes=bad)
    for thr in (0.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="conf_threshold"):
            StepConfig(label_merge="wbf", conf_threshold=thr)
        assert StepConfig(conf_threshold=thr).label_merge == "nms"          # the NMS takes any threshold, as before


def test_engine_refuses_more_votes_than_teachers():
    from mm_distillnet_amd.arch import make_spec
    from mm_distillnet_amd.step import DistillEngine, StepConfig
    with pytest.raises(ValueError, match="label_merge_votes 2 exceeds the 1 teachers"):
        DistillEngine(make_spec(0, 8), {"rgb": make_spec(0, 3)}, "cpu", StepConfig(image_size=128, label_merge="wbf", label_merge_votes=2))


def test_train_cfg_keys():
    sys.path.insert(0, ROOT)
    import train
    cfg, _ = train.parse_config(["--config_file", CFG])
    sc = train.step_config(cfg)
    assert (sc.label_merge, sc.label_merge_votes) == ("nms", 1)
    assert train.TR.label_merge_settings(cfg) == {"label_merge": "nms", "label_merge_votes": 1}
    cfg, _ = train.parse_config(["--config_file", CFG, "--overwrite", json.dumps({"label_merge": "wbf", "label_merge_votes": 2})])
    sc = train.step_config(cfg)
    assert (sc.label_merge, sc.label_merge_votes) == ("wbf", 2)
    assert sc.merge_iou == 0.5 and sc.inclusive_nms is False
    for ov in ({"label_merge": "softnms"}, {"label_merge": "wbf", "label_merge_votes": 0}, {"label_merge": "wbf", "conf_threshold": 0}):
        cfg, _ = train.parse_config(["--config_file", CFG, "--overwrite", json.dumps(ov)])
        with pytest.raises(ValueError, match="label_merge|conf_threshold"):
            train.step_config(cfg)


def test_header_declares_wbf_merge_as_python_calls_it():
    from mm_distillnet_amd import _lib
    sig = _lib.parse_header()["mmd_wbf_merge_n"]
    P, I = ctypes.c_void_p, ctypes.c_int
    assert sig == [P, P, I, ctypes.c_float, I, I, P, P, I, P, I, P, I, I, P]
    import ast
    import inspect
    from mm_distillnet_amd import postproc
    tree = ast.parse(inspect.getsource(postproc.wbf_merge))
    calls = [n for n in ast.walk(tree) if isinstance(n, ast.Call) and n.args and isinstance(n.args[0], ast.Constant)
             and n.args[0].value == "mmd_wbf_merge_n"]
    assert len(calls) == 1 and len(calls[0].args) - 1 == len(sig) - 1          # everything but the stream, which _lib.call appends


def test_wbf_entry_point_rejects_bad_arguments_without_gpu():
    from mm_distillnet_amd import _lib
    dll = _lib.LIB.load()
    one = (ctypes.c_void_p * 4)(8, 8, 8, 8)          # never dereferenced: validation comes before any launch

    def rc(srcs=one, cnts=one, nsrc=3, B=2, boxes=8, nbox=8, maxg=4, min_votes=1, ovf=8, cap=8):
        return dll.mmd_wbf_merge_n(srcs, cnts, nsrc, 0.5, 0, B, boxes, nbox, maxg, None, min_votes, ovf, 0, cap, None)
    for kw in (dict(srcs=None), dict(cnts=None), dict(boxes=None), dict(nbox=None), dict(ovf=None), dict(nsrc=0), dict(nsrc=5), dict(B=0),
               dict(maxg=0), dict(cap=0), dict(min_votes=0), dict(min_votes=4), dict(srcs=(ctypes.c_void_p * 4)(8, None, 8, 8))):
        assert rc(**kw) == -22, kw
