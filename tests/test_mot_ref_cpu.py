"""CPU: the tracking-evaluation rule (tests/mot_ref.py) on cases worked out by hand, the host side of mm_distillnet_amd.mot (`prepare`:
every refusal, the stable sort, the dense ids, the offset tables; `derive`), and the C ABI of csrc/moteval.hip without a GPU."""
import ctypes
import math

import numpy as np
import pytest

import mot_cases
import mot_ref

COUNT_KEYS = ("n_gt", "n_hyp", "tp", "fp", "fn", "idsw", "frag", "mt", "pt", "ml", "idtp", "idfp", "idfn")


@pytest.mark.parametrize("name", sorted(mot_cases.hand_cases()))
def test_reference_gives_the_hand_computed_counts(name):
    gt, hyp, n_windows, iou_min, want = mot_cases.hand_cases()[name]
    got = mot_ref.evaluate(gt, hyp, n_windows, iou_min, check_unique=True)
    assert {k: got["overall"][k] for k in COUNT_KEYS} == want
    assert got["unique"], got["margin"]
    o = got["overall"]
    assert o["mota"] == 1.0 - (o["fn"] + o["fp"] + o["idsw"]) / o["n_gt"]
    assert o["idf1"] == 2 * o["idtp"] / (2 * o["idtp"] + o["idfp"] + o["idfn"])


def test_reference_iou_sum_and_ratios():
    gt, hyp, n_windows, iou_min, _ = mot_cases.hand_cases()["greedy_not_optimum"]
    got = mot_ref.evaluate(gt, hyp, n_windows, iou_min)["overall"]
    f = np.float32
    want = float(f(60) / f(140)) + float(f(70) / f(130)) + float(f(90) / f(110))
    assert abs(got["motp"] * 3 - want) < 1e-12
    assert got["precision"] == 1.0 and got["recall"] == 1.0 and got["mota"] == 1.0
    # nothing at all: every ratio is NaN
    e = (np.zeros((0, 6), np.float32), np.zeros(0, np.int64), np.zeros(0, np.int64))
    got = mot_ref.evaluate(e, e, 2)["overall"]
    assert all(math.isnan(got[k]) for k in ("mota", "motp", "precision", "recall", "idp", "idr", "idf1")) and got["tp"] == 0


def test_uniqueness_check_notices_a_tie():
    # two hypotheses at the same place: either may take the ground-truth box
    gt = mot_cases.rec([(0, 0, mot_cases.box(0))])
    hyp = mot_cases.rec([(0, 1, mot_cases.box(1)), (0, 2, mot_cases.box(1))])
    got = mot_ref.evaluate(gt, hyp, 1, 0.5, check_unique=True)
    assert got["unique"] is False and got["margin"] == 0.0 and got["overall"]["tp"] == 1


# ---------------------------------------------------------------------------------------------- the host side of mot.py
def _no_device(monkeypatch):
    from mm_distillnet_amd import _lib, mot

    def fail(*a, **k):
        raise AssertionError("the device was reached")
    monkeypatch.setattr(mot, "run_device", fail)
    monkeypatch.setattr(_lib.LIB, "load", fail)
    return mot


def test_every_refusal_comes_before_the_device(monkeypatch):
    mot = _no_device(monkeypatch)
    box, rec = mot_cases.box, mot_cases.rec
    ok = rec([(0, 0, box(0)), (1, 0, box(1))])
    with pytest.raises(ValueError, match="gt row 1 has track -1"):
        mot.mot_metrics(rec([(0, 0, box(0)), (1, -1, box(1))]), ok, 2, "cuda:0")
    with pytest.raises(ValueError, match="gt track 3 occurs more than once in window 1 of session 0"):
        mot.mot_metrics(rec([(0, 3, box(0)), (1, 3, box(1)), (1, 3, box(5))]), ok, 2, "cuda:0")
    with pytest.raises(ValueError, match="hyp track 7 occurs more than once in window 0 of session 2"):
        h = rec([(0, 7, box(0)), (0, 7, box(1)), (0, 7, box(2))])
        mot.mot_metrics(ok, h + (np.array([2, 1, 2]),), 2, "cuda:0")
    # rows without a track may share a window
    many = rec([(0, -1, box(k)) for k in range(256)] + [(1, -1, box(0))])
    with pytest.raises(AssertionError, match="the device was reached"):
        mot.mot_metrics(ok, many, 2, "cuda:0")
    with pytest.raises(ValueError, match="hyp holds 257 rows in window 0 of session 0: at most 256"):
        mot.mot_metrics(ok, rec([(0, -1, box(k)) for k in range(257)]), 2, "cuda:0")
    with pytest.raises(ValueError, match="gt holds 257 rows in window 1"):
        mot.mot_metrics(rec([(1, k, box(k)) for k in range(257)]), ok, 2, "cuda:0")
    crowd = rec([(w, w * 256 + k, box(k)) for w in range(5) for k in range(205)])           # 1025 tracks
    with pytest.raises(ValueError, match="1025 tracks of one side in one session: the identity measures hold at most 1024"):
        mot.mot_metrics(ok, crowd, 5, "cuda:0")
    with pytest.raises(AssertionError, match="the device was reached"):
        mot.mot_metrics(ok, crowd, 5, "cuda:0", identity=False)
    with pytest.raises(ValueError, match="window indices must lie inside"):
        mot.mot_metrics(ok, ok, 1, "cuda:0")
    with pytest.raises(ValueError, match="2 rows, 2 window indices, 1 track ids"):
        mot.mot_metrics(ok, (ok[0], ok[1], ok[2][:1]), 2, "cuda:0")
    with pytest.raises(ValueError, match="iou_min"):
        mot.mot_metrics(ok, ok, 2, "cuda:0", iou_min=0.0)
    with pytest.raises(ValueError, match="n_windows"):
        mot.mot_metrics(ok, ok, 0, "cuda:0")
    with pytest.raises(ValueError, match="rows, window, track"):
        mot.mot_metrics(ok[:2], ok, 2, "cuda:0")


def test_prepare_sorts_stably_and_makes_dense_ids(monkeypatch):
    mot = _no_device(monkeypatch)
    box = mot_cases.box
    rows = np.array([box(k) for k in range(6)], np.float32)
    window = np.array([1, 0, 1, 0, 2, 0])
    track = np.array([40, 7, 9, 40, 7, 9])
    session = np.array([1, 0, 1, 1, 0, 0])
    hyp = (rows[:2], np.array([2, 0]), np.array([-1, 5]), np.array([1, 1]))
    p = mot.prepare((rows, window, track, session), hyp, 3)
    g = p["gt"]
    assert p["n_sessions"] == 2 and p["n_windows"] == 3
    # session 0: windows 0 (rows 1, 5 in record order), 2 (row 4); session 1: window 0 (row 3), 1 (rows 0, 2)
    assert g["rows"][:, 0].tolist() == [1, 5, 4, 3, 0, 2]
    assert g["off"].tolist() == [0, 2, 2, 3, 4, 6, 6] and g["off"].dtype == np.int32
    # dense ids per session in rising id order: session 0 {7: 0, 9: 1}, session 1 {9: 0, 40: 1}
    assert g["dense"].tolist() == [0, 1, 0, 1, 1, 0] and g["trk_off"].tolist() == [0, 2, 4]
    assert g["u_sess"].tolist() == [0, 0, 1, 1] and g["u_id"].tolist() == [7, 9, 9, 40]
    h = p["hyp"]
    assert h["off"].tolist() == [0, 0, 0, 0, 1, 1, 2] and h["dense"].tolist() == [0, -1] and h["trk_off"].tolist() == [0, 0, 1]


def test_derive_and_assemble_match_the_reference(monkeypatch):
    """`assemble` on counts taken from the reference gives the reference's dictionaries: the host arithmetic of mot.py is the rule's"""
    mot = _no_device(monkeypatch)
    recs = [mot_cases.traffic(s)[:2] for s in (1, 2)]
    gt = mot_cases.interleave([r[0] for r in recs], 5)
    hyp = mot_cases.interleave([r[1] for r in recs], 6)
    ref = mot_ref.evaluate(gt, hyp, 12)
    p = mot.prepare(gt, hyp, 12)
    names = ("n_gt", "n_hyp", "tp", "fp", "fn", "idsw", "frag")
    counts = np.array([[s[k] for k in names] + [12] for s in ref["sessions"]], np.int64)
    res = {"counts": counts, "iou_sum": ref["iou_sums"], "present": ref["gt_tracks"][:, 2].astype(np.int32),
           "matched": ref["gt_tracks"][:, 3].astype(np.int32), "idtp": np.array([s["idtp"] for s in ref["sessions"]], np.int64)}
    got = mot.assemble(p, res)
    assert np.array_equal(got["gt_tracks"], ref["gt_tracks"])
    assert tuple(got["overall"]) == mot.KEYS
    for a, b in zip([got["overall"]] + got["sessions"], [ref["overall"]] + ref["sessions"]):
        for k in mot.KEYS:
            assert a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]), k
    res["idtp"] = None
    assert tuple(mot.assemble(p, res)["overall"]) == mot.CLEAR_KEYS


# ---------------------------------------------------------------------------------------------- C ABI without a GPU
def test_header_declares_and_library_exports_the_entry_points():
    import __graft_entry__ as ge
    ge.build()
    from mm_distillnet_amd import _lib
    sigs = _lib.LIB.symbols()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    P, I, LL, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float
    want = {"mmd_mot_clear_ws_bytes": [LL],
            "mmd_mot_clear": [P, P, P, LL, P, P, P, LL, I, I, P, LL, F, P, P, P, P, P, P],
            "mmd_mot_id_counts": [P, P, P, LL, P, P, P, LL, I, I, P, P, I, P, LL, F, P, P],
            "mmd_mot_id_assign": [P, P, LL, P, P, I, I, P, P]}
    for name, types in want.items():
        assert sigs[name] == types and hasattr(dll, name), name
    text = open(_lib.HEADER).read()

    def comment_of(name):
        lines = text[:text.index("int %s(" % name)].rstrip("\n").split("\n")
        out = []
        while lines and lines[-1].startswith("//"):
            out.append(lines.pop()[2:].strip())
        return " ".join(reversed(out))

    assert "need no zeroing" in comment_of("mmd_mot_clear") and "two runs give the same bits" in comment_of("mmd_mot_clear")
    assert "CALLER ZEROES C" in comment_of("mmd_mot_id_counts") and "1 .. 1024" in comment_of("mmd_mot_id_counts")
    assert "needs no zeroing" in comment_of("mmd_mot_id_assign")


def test_bad_arguments_are_rejected_without_gpu():
    import __graft_entry__ as ge
    ge.build()
    from mm_distillnet_amd import _lib
    dll = _lib.LIB.load()
    p = ctypes.c_void_p(4096)            # never dereferenced: validation precedes any launch
    assert dll.mmd_mot_clear_ws_bytes(0) > 0 and dll.mmd_mot_clear_ws_bytes(1000) >= 8000
    assert dll.mmd_mot_clear_ws_bytes(-1) == -22 and dll.mmd_mot_clear_ws_bytes(1 << 27) == -22

    def clear(ptrs=None, n_g=5, n_h=5, S=1, W=3, T=2):
        q = [p] * 12 if ptrs is None else ptrs
        return dll.mmd_mot_clear(q[0], q[1], q[2], n_g, q[3], q[4], q[5], n_h, S, W, q[6], T, 0.5, q[7], q[8], q[9], q[10], q[11], None)

    for k in range(12):
        assert clear([None if j == k else p for j in range(12)]) == -22, k
    for bad in (dict(n_g=-1), dict(n_h=-1), dict(S=0), dict(S=65536), dict(W=0), dict(T=-1), dict(n_g=1 << 31), dict(S=65535, W=1 << 16)):
        assert clear(**bad) == -22, bad

    def counts(ptrs=None, S=1, W=3, most=4, c_total=16):
        q = [p] * 10 if ptrs is None else ptrs
        return dll.mmd_mot_id_counts(q[0], q[1], q[2], 5, q[3], q[4], q[5], 5, S, W, q[6], q[7], most, q[8], c_total, 0.5, q[9], None)

    for k in range(10):
        assert counts([None if j == k else p for j in range(10)]) == -22, k
    for bad in (dict(S=0), dict(S=65536), dict(W=0), dict(most=0), dict(most=1025), dict(c_total=0)):
        assert counts(**bad) == -22, bad

    def assign(ptrs=None, S=1, most=4, c_total=16):
        q = [p] * 5 if ptrs is None else ptrs
        return dll.mmd_mot_id_assign(q[0], q[1], c_total, q[2], q[3], S, most, q[4], None)

    for k in range(5):
        assert assign([None if j == k else p for j in range(5)]) == -22, k
    for bad in (dict(S=0), dict(S=65536), dict(most=0), dict(most=1025), dict(c_total=0)):
        assert assign(**bad) == -22, bad
