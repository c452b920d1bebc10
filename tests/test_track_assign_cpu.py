"""The tracker's optimal association rule, CPU side: TrackConfig.assign and its graph key, the scipy restatement
(tests/track_assign_ref.py) against brute-force enumeration of every matching, the scenes on which it must differ from the greedy rule
(tests/track_ref.py), detect.py's --track_assign option and the C ABI of mmd_track_update_assign / mmd_track_update_bank_assign without
a GPU."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest

import mot_ref
import track_assign_ref
import track_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def _cfg(**kw):
    from mm_distillnet_amd.tracker import TrackConfig
    return TrackConfig(**kw)


def _record(windows):
    rows = [r for w in windows for r in w]
    win = [i for i, w in enumerate(windows) for _ in w]
    return np.asarray(rows, np.float32).reshape(-1, 6), np.asarray(win, np.int32), len(windows)


_box, crossing = track_assign_ref.box, track_assign_ref.crossing
DIFFERS, DIFFERS_KW, WEIGHT = track_assign_ref.DIFFERS, track_assign_ref.DIFFERS_KW, track_assign_ref.WEIGHT


# ---------------------------------------------------------------------------------------------- TrackConfig
def test_track_config_takes_the_rule_and_refuses_any_other():
    assert _cfg().assign == "greedy" and _cfg(assign="greedy").assign == "greedy" and _cfg(assign="optimal").assign == "optimal"
    for bad in ("Optimal", "hungarian", "", None, 1, 0, True, b"optimal"):
        with pytest.raises(ValueError, match="TrackConfig: assign"):
            _cfg(assign=bad)


def test_the_greedy_key_is_unchanged_and_the_optimal_key_differs():
    assert _cfg().key() == (0.3, 0.5, 2, 0.0, 64) == _cfg(assign="greedy").key()
    assert _cfg(iou_min=1.0, beta=0.0).key() == (1.0, 0.0, 2, 0.0, 64)
    assert _cfg(assign="optimal").key() == (0.3, 0.5, 2, 0.0, 64, "optimal")
    assert _cfg(assign="optimal").key() != _cfg().key() and hash(_cfg(assign="optimal").key()) is not None
    assert _cfg(assign="optimal", max_tracks=8).key() != _cfg(assign="optimal").key()


# ---------------------------------------------------------------------------------------------- the restatement
def _matchings(T, n):
    """every matching of T slots and n detections as a tuple of (t, d) pairs, the empty one included"""
    out = []
    for k in range(min(T, n) + 1):
        for ts in itertools.combinations(range(T), k):
            for ds in itertools.permutations(range(n), k):
                out.append(tuple(zip(ts, ds)))
    return out


def _brute(W, allowed):
    """-> (best set of allowed pairs, its weight, the weight of the best DIFFERENT set of allowed pairs)"""
    weight = {}
    for m in _matchings(*W.shape):
        pairs = frozenset(p for p in m if allowed[p])
        weight[pairs] = float(sum(W[p] for p in pairs))
    order = sorted(weight.items(), key=lambda kv: -kv[1])
    return order[0][0], order[0][1], (order[1][1] if len(order) > 1 else -np.inf)


def _problem(rng, T, n):
    """T tracks born in window 0 (so slot t = id t, velocity 0: the prediction is the box) and n detections in window 1; some labels
    differ, now and then a coordinate is NaN"""
    def boxes(k):
        out = []
        for _ in range(k):
            x, y, s = rng.uniform(0, 30), rng.uniform(0, 12), rng.uniform(14, 26)
            out.append([x, y, x + s, y + s, 0.9, float(rng.choice([6, 6, 6, 14]))])
        return out
    first, second = boxes(T), boxes(n)
    if rng.random() < 0.25:
        first[int(rng.integers(T))][int(rng.integers(4))] = NAN
    if rng.random() < 0.25:
        second[int(rng.integers(n))][int(rng.integers(4))] = NAN
    return [tuple(b) for b in first], [tuple(b) for b in second]


def test_restatement_against_brute_force_on_small_problems():
    rng = np.random.default_rng(5)
    shapes = [(T, n) for T in range(1, 5) for n in range(1, 5)]
    seen = dict(more_slots=0, more_dets=0, label=0, nan=0, multi=0, decided=0, greedy_differs=0)
    for k in range(320):
        T, n = shapes[k % len(shapes)]
        first, second = _problem(rng, T, n)
        cfg = _cfg(assign="optimal", iou_min=0.2, max_tracks=8)
        tb, det = np.asarray(first, np.float32), np.asarray(second, np.float32)
        W, allowed = track_assign_ref.weights(tb[:, :4], tb[:, 5], det, cfg.iou_min)
        assert W.dtype == np.float64 and np.isfinite(W).all() and (W[~allowed] == 0).all() and (W[allowed] >= np.float32(0.2)).all()
        best, weight, runner_up = _brute(W, allowed)
        pairs, got_weight = track_assign_ref.solve(W, allowed)
        assert abs(got_weight - weight) <= 1e-12
        margin = track_assign_ref.margin(W, allowed, pairs)
        if not best:
            assert margin == np.inf and pairs == []
            continue
        assert abs(margin - (weight - runner_up)) <= 1e-12, (k, margin, weight, runner_up)
        if margin <= 1e-9:
            continue
        assert frozenset(pairs) == best
        # the same through `track`: the matched detection carries its slot's id, the others are born behind the T ids of window 0
        ids, slots, glob, m = track_assign_ref.track(*_record([first, second]), cfg)
        assert abs(m - margin) <= 1e-12
        want, nxt = [-1] * n, T
        for t, d in best:
            want[d] = t
        for d in range(n):
            if want[d] < 0:
                want[d], nxt = nxt, nxt + 1
        assert ids.tolist() == list(range(T)) + want and glob.tolist() == [nxt, 0]
        matched = sorted(t for t, _ in best)
        assert [t for t in range(T) if slots[t, 10] == 2] == matched and [t for t in range(T) if slots[t, 11] == 1] == \
            [t for t in range(T) if t not in matched]
        seen["decided"] += 1
        seen["more_slots"] += T > n
        seen["more_dets"] += n > T
        seen["label"] += bool((tb[:, 5][:, None] != det[:, 5][None, :]).any())
        seen["nan"] += bool(np.isnan(tb).any() or np.isnan(det).any())
        seen["multi"] += len(best) >= 2
        seen["greedy_differs"] += track_ref.track(*_record([first, second]), _cfg(iou_min=0.2, max_tracks=8))[0].tolist() != ids.tolist()
    print(seen)
    assert seen["decided"] >= 200 and min(seen.values()) >= 5, seen


def test_optimal_differs_from_greedy_where_the_largest_iou_blocks_the_second_track():
    cfg_o, cfg_g = _cfg(assign="optimal", **DIFFERS_KW), _cfg(**DIFFERS_KW)
    rec = _record(list(DIFFERS))
    iou = track_ref.iou_matrix(rec[0][:2, :4], rec[0][2:, :4])
    assert iou[0, 0] == iou.max() and iou[0, 1] >= 0.2 and iou[1, 0] >= 0.2 and iou[1, 1] == 0            # the case has not degenerated
    assert float(iou[0, 1]) + float(iou[1, 0]) > float(iou[0, 0])
    opt, greedy = track_assign_ref.track(*rec, cfg_o), track_ref.track(*rec, cfg_g)
    assert opt[0].tolist() == [0, 1, 1, 0] and opt[2].tolist() == [2, 0] and opt[3] > 0.1
    assert greedy[0].tolist() == [0, 1, 0, 2] and greedy[2].tolist() == [3, 0]
    assert opt[0].tolist() != greedy[0].tolist() and not np.array_equal(opt[1], greedy[1])
    assert opt[1][:2, 10].tolist() == [2, 2] and greedy[1][:2, 10].tolist() == [2, 1] and greedy[1][1, 11] == 1


def test_maximum_weight_is_not_maximum_cardinality():
    """On this case the greedy rule agrees with the optimum - it always takes the largest IoU first, and a second pair it could add the
    optimum would add too - so what the optimum must differ from here is the matching with the most pairs."""
    cfg = _cfg(assign="optimal")
    rec = _record(list(WEIGHT))
    W, allowed = track_assign_ref.weights(rec[0][:2, :4], rec[0][:2, 5], rec[0][2:], cfg.iou_min)
    assert allowed.tolist() == [[True, True], [True, False]] and W[0, 0] > 0.9 and 0.3 < W[0, 1] < 0.4 and 0.3 < W[1, 0] < 0.4
    assert W[0, 0] > W[0, 1] + W[1, 0]                                                      # one pair beats two
    most = max(_matchings(2, 2), key=lambda m: (sum(bool(allowed[p]) for p in m), sum(W[p] for p in m if allowed[p])))
    assert sorted(p for p in most if allowed[p]) == [(0, 1), (1, 0)]                        # the maximum-cardinality matching
    opt = track_assign_ref.track(*rec, cfg)
    assert opt[0].tolist() == [0, 1, 0, 2] and opt[2].tolist() == [3, 0] and opt[3] > 0.1   # the single pair; the other box is born
    assert opt[1][0, 10] == 2 and opt[1][1, 10] == 1 and opt[1][1, 11] == 1 and opt[1][2, 1] == 2      # the other track ages
    greedy = track_ref.track(*rec, _cfg())
    for a, b in zip(opt[:3], greedy):
        np.testing.assert_array_equal(a, b)


def test_fewer_identity_switches_on_a_crossing_scene():
    windows, gt = crossing()
    rows, window, n = _record(windows)
    assert n == 10
    greedy = track_ref.track(rows, window, n, _cfg())[0]
    opt = track_assign_ref.track(rows, window, n, _cfg(assign="optimal"))
    assert opt[3] > 1e-6
    figures = [mot_ref.evaluate((rows, window, gt), (rows, window, ids), n)["overall"] for ids in (greedy, opt[0])]
    print("greedy: idsw %d, ids %s; optimal: idsw %d, ids %s" % (figures[0]["idsw"], greedy.tolist(), figures[1]["idsw"], opt[0].tolist()))
    assert figures[1]["idsw"] < figures[0]["idsw"]
    assert figures[1]["idsw"] == 0 and opt[0].tolist() == gt.tolist() and greedy.max() == 2      # greedy gave birth to a third id


def test_the_restatement_goes_on_from_a_state():
    windows, _ = crossing()
    rows, win, n = _record(windows)
    cfg = _cfg(assign="optimal")
    whole = track_assign_ref.track(rows, win, n, cfg)
    cut = int(np.searchsorted(win, 4))
    first = track_assign_ref.track(rows[:cut], win[:cut], 4, cfg)
    second = track_assign_ref.track(rows[cut:], win[cut:] - 4, 6, cfg, first[1], first[2])
    np.testing.assert_array_equal(np.concatenate([first[0], second[0]]), whole[0])
    got = second[1].copy()
    got[:, 12] += 4 * (got[:, 0] != 0)
    np.testing.assert_array_equal(got, whole[1])
    np.testing.assert_array_equal(second[2], whole[2])
    assert min(first[3], second[3]) == whole[3]


# ---------------------------------------------------------------------------------------------- detect.py
def test_track_assign_option_is_checked_before_any_gpu_call(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import detect
    import torch

    def refuse(*a, **k):
        raise AssertionError("the GPU was reached")

    monkeypatch.setattr(torch.cuda, "set_device", refuse)
    monkeypatch.setattr(torch, "load", refuse)
    np.save(tmp_path / "one.npy", np.zeros((8, 9000), np.float32))
    cfgf = os.path.join(ROOT, "configs", "mm-distillnet.cfg")
    argv = ["--config_file", cfgf, "--checkpoint", str(tmp_path / "none.pth"), "--input", str(tmp_path / "one.npy"),
            "--output", str(tmp_path / "o.csv")]
    assert detect.parse_args(argv).track_assign == "greedy"
    assert detect.parse_args(argv + ["--window_s", "0.1", "--track", "--track_assign", "optimal"]).track_assign == "optimal"
    with pytest.raises(ValueError, match="--window_s"):                                       # as the other --track options
        detect.main(argv + ["--track", "--track_assign", "optimal"])
    with pytest.raises(ValueError, match="TrackConfig: assign"):
        detect.main(argv + ["--window_s", "0.1", "--track", "--track_assign", "hungarian"])
    assert not os.path.exists(tmp_path / "o.csv")
    # a good value passes the flag checks: the first thing refused is then the load of the checkpoint
    with pytest.raises(AssertionError, match="the GPU was reached"):
        detect.main(argv + ["--window_s", "0.1", "--track", "--track_assign", "optimal"])
    assert "--track_assign greedy|optimal" in detect.__doc__ and "maximum IoU sum" in detect.__doc__


# ---------------------------------------------------------------------------------------------- C ABI without a GPU
def test_header_declares_and_library_exports_the_entry_points():
    import __graft_entry__ as ge
    ge.build()
    from mm_distillnet_amd import _lib
    sigs = _lib.LIB.symbols()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name, old in (("mmd_track_update_assign", "mmd_track_update"), ("mmd_track_update_bank_assign", "mmd_track_update_bank")):
        assert name in sigs and hasattr(dll, name)
        assert sigs[name] == sigs[old][:-1] + [ctypes.c_int, ctypes.c_void_p]               # the old arguments, assign, the stream
    assert len(sigs["mmd_track_update"]) == 16 and len(sigs["mmd_track_update_bank"]) == 19
    text = open(_lib.HEADER).read()
    head = text[:text.index("int mmd_track_update_assign(")]
    comment = head[head.rindex("\n\n"):].replace("\n// ", " ")
    for phrase in ("0 = greedy", "1 = optimal", "anything else -22", "MAXIMUM WEIGHT", "not maximum cardinality", "false for NaN",
                   "linear_sum_assignment", "unspecified", "nothing is matched"):
        assert phrase in comment, phrase


def test_bad_arguments_are_rejected_without_gpu():
    import __graft_entry__ as ge
    ge.build()
    from mm_distillnet_amd import _lib
    dll = _lib.LIB.load()
    p = ctypes.c_void_p(4096)            # never dereferenced: validation precedes any launch

    def single(ptrs=None, assign=1, B=3, max_tracks=64):
        q = [p] * 7 if ptrs is None else ptrs
        return dll.mmd_track_update_assign(q[0], q[1], B, 4, q[2], q[3], 6, q[4], q[5], q[6], max_tracks, 0.3, 0.5, 2, 0.0, assign, None)

    def bank(ptrs=None, assign=1, n_sessions=2, max_tracks=64):
        q = [p] * 9 if ptrs is None else ptrs
        return dll.mmd_track_update_bank_assign(q[0], q[1], 3, 4, q[2], q[3], q[4], n_sessions, q[5], 6, q[6], q[7], q[8], max_tracks,
                                                0.3, 0.5, 2, 0.0, assign, None)

    for assign in (2, -1, 3, 1 << 20):
        assert single(assign=assign) == -22 and bank(assign=assign) == -22, assign
    for assign in (0, 1):
        for k in range(7):
            assert single([None if j == k else p for j in range(7)], assign) == -22, (assign, k)
        for k in range(9):
            assert bank([None if j == k else p for j in range(9)], assign) == -22, (assign, k)
        assert single(assign=assign, B=0) == -22 and single(assign=assign, B=1025) == -22 and single(assign=assign, max_tracks=257) == -22
        assert bank(assign=assign, n_sessions=0) == -22 and bank(assign=assign, max_tracks=0) == -22
