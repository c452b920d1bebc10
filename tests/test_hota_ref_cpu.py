"""CPU: the HOTA restatement (tests/hota_ref.py) on closed forms worked out by hand from the published definition, the host side of
mm_distillnet_amd.mot's `hota_metrics` (refusals before the library loads, `hota_prepare`, `hota_assemble`), the C ABI of the three
`mmd_hota_*` entry points without a GPU, and the uniqueness proof of every input tests/test_gpu_hota.py runs."""
import ctypes
import math

import numpy as np
import pytest

import hota_cases
import hota_ref
import mot_cases

box, rec = mot_cases.box, mot_cases.rec
KEYS = ("hota", "deta", "assa", "detre", "detpr", "assre", "asspr", "loca")


def _near(a, b, ulps=8):
    return abs(a - b) <= ulps * 2.0 ** -52 * max(abs(b), 1e-300)


# ---------------------------------------------------------------------------------------------- closed forms
def test_thresholds_and_q():
    assert hota_ref.ALPHA32.dtype == np.float32 and len(hota_ref.ALPHA32) == 19
    assert float(hota_ref.ALPHA32[9]) == 0.5 and float(hota_ref.ALPHA32[0]) == float(np.float32(0.05))
    assert hota_ref.q(np.float32(1.0)) == 2 ** 32 and hota_ref.q(np.float32(0.5)) == 2 ** 31 and hota_ref.q(0.0) == 0
    assert hota_ref.q(2.0 ** -33) == 1 and hota_ref.q(2.0 ** -34) == 0                    # floor(x * 2^32 + 0.5)
    assert hota_ref.bins(1.0) == 19 and hota_ref.bins(0.0) == 0 and hota_ref.bins(np.float32(0.05)) == 1


def test_perfect_tracking_gives_one_everywhere():
    gt = rec([(w, t, box(40 * t + w)) for w in range(6) for t in range(3)])
    got = hota_ref.evaluate(gt, gt, 6, check_unique=True)
    assert got["unique"]
    assert got["overall"] == {k: 1.0 for k in KEYS} and got["sessions"] == [got["overall"]]
    assert got["alphas"]["overall"]["tp"].tolist() == [18] * 19


@pytest.mark.parametrize("n", [1, 4, 7])
def test_one_track_followed_by_two_ids(n):
    """every TP has TPA = n, FNA = n, FPA = 0: A = n / 2n per TP -> AssA = AssRe = 1/2, AssPr = 1, DetA = 1, HOTA = sqrt(1/2)"""
    got = hota_ref.evaluate(*hota_cases.split_track(n))
    per = got["alphas"]["overall"]
    assert per["tp"].tolist() == [2 * n] * 19
    for k in range(19):
        assert per["deta"][k] == 1.0 and per["detre"][k] == 1.0 and per["detpr"][k] == 1.0 and per["loca"][k] == 1.0
        assert per["assa"][k] == 0.5 and per["assre"][k] == 0.5 and per["asspr"][k] == 1.0
        assert per["hota"][k] == math.sqrt(0.5)
    assert _near(got["overall"]["hota"], math.sqrt(0.5)) and got["overall"]["assa"] == 0.5 and got["overall"]["deta"] == 1.0
    assert got["P"][0].tolist() == [[n * 2 ** 32, n * 2 ** 32]]


def test_iou_two_thirds_passes_thirteen_thresholds():
    got = hota_ref.evaluate(rec([(0, 0, box(0))]), rec([(0, 0, box(2))]), 1)
    assert got["tp"][0].tolist() == [1] * 13 + [0] * 6
    s = np.float32(80) / np.float32(120)
    assert got["loc"][0] == [int(hota_ref.q(s))] * 13 + [0] * 6
    per = got["alphas"]["overall"]
    assert per["loca"][:13].tolist() == [float(s)] * 13 and per["loca"][13:].tolist() == [1.0] * 6
    assert per["deta"][:13].tolist() == [1.0] * 13 and per["deta"][13:].tolist() == [0.0] * 6
    assert _near(got["overall"]["deta"], 13 / 19) and _near(got["overall"]["hota"], 13 / 19)


def test_iou_one_half_passes_alpha_9():
    gt, hyp, n_windows = mot_cases.hand_cases()["iou_equals_iou_min"][:3]
    got = hota_ref.evaluate(gt, hyp, n_windows)
    assert got["tp"][0].tolist() == [1] * 10 + [0] * 9 and got["hist"][0][0, 0].tolist() == [0] * 9 + [1] + [0] * 9


def test_unequal_labels_pair_nothing():
    gt, hyp, n_windows = mot_cases.hand_cases()["labels_differ"][:3]
    got = hota_ref.evaluate(gt, hyp, n_windows)["overall"]
    assert got["deta"] == 0.0 and got["assa"] == 0.0 and got["hota"] == 0.0 and got["loca"] == 1.0


def test_a_row_without_a_track_is_a_false_positive_at_every_threshold():
    # the row without a track lies exactly on the vehicle and still cannot take it
    got = hota_ref.evaluate(rec([(0, 0, box(0))]), rec([(0, -1, box(0)), (0, 4, box(1))]), 1)
    per = got["alphas"]["overall"]
    assert got["n_hyp"] == [2] and got["P"][0].shape == (1, 1)
    assert per["tp"].tolist() == [1] * 16 + [0] * 3                                       # 9 / 11 = .818
    assert per["detpr"][:16].tolist() == [0.5] * 16 and per["detre"][:16].tolist() == [1.0] * 16
    assert all(_near(v, 1 / 2) for v in per["deta"][:16])                                 # TP / (TP + FN + FP) = 1 / (1 + 0 + 1)
    # nothing at all: the detection ratios are NaN, LocA is 1
    e = (np.zeros((0, 6), np.float32), np.zeros(0, np.int64), np.zeros(0, np.int64))
    got = hota_ref.evaluate(e, e, 2)["overall"]
    assert math.isnan(got["deta"]) and math.isnan(got["hota"]) and got["assa"] == 0.0 and got["loca"] == 1.0


def test_alignment_changes_the_pairing():
    gt, hyp, n_windows = hota_cases.alignment_wins()
    got = hota_ref.evaluate(gt, hyp, n_windows, check_unique=True)
    assert got["unique"]
    # cell 0 = (g, id 11), cell 1 = (g, id 22): id 11 keeps the vehicle in window 4 at IoU 7/13 (10 thresholds); 9/11 would pass 16
    assert got["hist"][0][0, 0].tolist() == [0] * 9 + [1] + [0] * 8 + [4] and int(got["hist"][0][0, 1].sum()) == 0
    assert got["tp"][0].tolist() == [5] * 10 + [4] * 9
    # the alignment by hand: window 4 gives id 11 the share q(7/13) / (q(7/13) + q(9/11))
    a, b = int(hota_ref.q(np.float32(70) / np.float32(130))), int(hota_ref.q(np.float32(90) / np.float32(110)))
    assert got["P"][0].tolist() == [[4 * 2 ** 32 + int(hota_ref.q(a / (a + b))), int(hota_ref.q(b / (a + b)))]]
    # without the alignment the window would pair the vehicle with id 22
    alone = hota_ref.evaluate(tuple(x[4:] for x in gt), tuple(x[4:] for x in hyp), 5)
    assert int(alone["hist"][0][0, 1].sum()) == 1 and int(alone["hist"][0][0, 0].sum()) == 0


def test_overall_is_the_tp_weighted_combination():
    a, b = hota_cases.case("traffic"), hota_cases.split_track(4)
    gt = tuple(np.concatenate([x, y]) for x, y in zip(mot_cases.with_session(a[0], 0), mot_cases.with_session(b[0], 1)))
    hyp = tuple(np.concatenate([x, y]) for x, y in zip(mot_cases.with_session(a[1], 0), mot_cases.with_session(b[1], 1)))
    both = hota_ref.evaluate(gt, hyp, 12)
    one = [hota_ref.evaluate(*a), hota_ref.evaluate(*b[:2], 12)]
    for s in range(2):
        assert both["sessions"][s] == one[s]["overall"]
    per, parts = both["alphas"]["overall"], [r["alphas"]["overall"] for r in one]
    tp = [p["tp"].astype(np.float64) for p in parts]
    assert per["tp"].tolist() == (parts[0]["tp"] + parts[1]["tp"]).tolist() and per["tp"][0] > parts[1]["tp"][0] > 0
    for k in ("assa", "assre", "asspr", "loca"):
        want = (parts[0][k] * tp[0] + parts[1][k] * tp[1]) / (tp[0] + tp[1])
        assert np.allclose(per[k], want, rtol=1e-14, atol=0), k
    n_gt, n_hyp = sum(r["n_gt"][0] for r in one), sum(r["n_hyp"][0] for r in one)
    assert np.allclose(per["deta"], per["tp"] / (n_gt + n_hyp - per["tp"]), rtol=1e-15, atol=0)
    assert np.allclose(per["hota"], np.sqrt(per["deta"] * per["assa"]), rtol=1e-15, atol=0)
    assert _near(both["overall"]["hota"], float(np.mean(per["hota"])))


def test_uniqueness_check_notices_a_tie():
    hyp = rec([(0, 1, box(1)), (0, 2, box(1))])                       # two hypotheses at the same place, each seen once
    got = hota_ref.evaluate(rec([(0, 0, box(0))]), hyp, 1, check_unique=True)
    assert got["unique"] is False and got["margin"] == 0.0


@pytest.mark.parametrize("name", hota_cases.NAMES)
def test_every_gpu_case_has_one_optimum(name):
    """no case of test_gpu_hota.py is left out: each window's matching is the only one within hota_ref.MARGIN of the scores' scale"""
    ref = hota_cases.reference(name)
    assert ref["unique"] and ref["margin"] > hota_ref.MARGIN, (name, ref["margin"])
    print(name, "smallest relative loss of a re-solve:", ref["margin"])


def test_the_cases_cover_the_shapes():
    cells = {name: hota_cases.reference(name)["cells"] for name in hota_cases.NAMES}
    assert cells["iou_equals_iou_min"] == [1] and cells["cells_3x1"] == [3] and cells["lanes_5x300"] == [1500] and cells["lanes_300x5"] == [1500]
    assert cells["no_hyp_tracks"][1:] == [0, 0] and cells["bank"][2] == 0 and min(cells["bank"][:2] + cells["bank"][3:]) > 0
    per = [np.bincount(hota_cases.case("traffic")[k][1], minlength=12) for k in (0, 1)]
    assert 0 in per[0] and 0 in per[1] and (per[0] == 0).tolist() != (per[1] == 0).tolist()      # windows empty on one side, on both
    assert np.bincount(hota_cases.case("fragmentation")[1][1], minlength=4).tolist() == [1, 0, 1, 1]      # .. and with one row
    for name, (ng, nh) in (("crowd_256x3", (256, 3)), ("crowd_3x256", (3, 256)), ("crowd_256x256", (256, 256)), ("crowd_5x9", (5, 9)), ("crowd_9x5", (9, 5))):
        gt, hyp, _ = hota_cases.case(name)
        assert np.bincount(gt[1]).max() == ng and np.bincount(hyp[1]).max() == nh
    assert min(hota_cases.reference(n)["tp"][0][0] for n in hota_cases.CROWDS) > 0


# ---------------------------------------------------------------------------------------------- the host side of mot.py
def _no_device(monkeypatch):
    from mm_distillnet_amd import _lib, mot

    def fail(*a, **k):
        raise AssertionError("the device was reached")
    monkeypatch.setattr(mot, "hota_run_device", fail)
    monkeypatch.setattr(_lib.LIB, "load", fail)
    return mot


def test_keys():
    from mm_distillnet_amd import mot
    assert mot.HOTA_KEYS == KEYS == hota_ref.KEYS
    assert mot.CLEAR_KEYS == ("n_gt", "n_hyp", "tp", "fp", "fn", "idsw", "frag", "mt", "pt", "ml", "mota", "motp", "precision", "recall")
    assert mot.ID_KEYS == ("idtp", "idfp", "idfn", "idp", "idr", "idf1") and mot.KEYS == mot.CLEAR_KEYS + mot.ID_KEYS
    assert np.array_equal(mot.hota_alphas(), hota_ref.ALPHA32.astype(np.float64))


def test_every_refusal_comes_before_the_device(monkeypatch):
    mot = _no_device(monkeypatch)
    ok = rec([(0, 0, box(0)), (1, 0, box(1))])
    with pytest.raises(AssertionError, match="the device was reached"):
        mot.hota_metrics(ok, ok, 2, "cuda:0")
    with pytest.raises(ValueError, match=r"n_windows = 1048577: at most 2\^20"):
        mot.hota_metrics(ok, ok, 2 ** 20 + 1, "cuda:0")
    # 14 sessions of 1024 x 1024 tracks: 14 680 064 cells, 19 words each, are more than 2^28
    rows = np.tile(np.array([box(20.0 * k) for k in range(256)], np.float32), (4 * 14, 1))
    window, session = np.tile(np.repeat(np.arange(4), 256), 14), np.repeat(np.arange(14), 1024)
    big = (rows, window, np.tile(np.arange(1024), 14), session)
    with pytest.raises(ValueError, match=r"14680064 track pairs over all sessions need 278921216 histogram cells: at most 2\^28"):
        mot.hota_metrics(big, big, 4, "cuda:0")
    # what mot_metrics refuses, hota_metrics refuses: the caps of prepare hold
    with pytest.raises(ValueError, match="hyp holds 257 rows in window 0 of session 0: at most 256"):
        mot.hota_metrics(ok, rec([(0, -1, box(k)) for k in range(257)]), 2, "cuda:0")
    with pytest.raises(ValueError, match="1025 tracks of one side in one session"):
        mot.hota_metrics(ok, rec([(w, w * 256 + k, box(k)) for w in range(5) for k in range(205)]), 5, "cuda:0")
    with pytest.raises(ValueError, match="gt row 1 has track -1"):
        mot.hota_metrics(rec([(0, 0, box(0)), (1, -1, box(1))]), ok, 2, "cuda:0")
    with pytest.raises(ValueError, match="n_windows"):
        mot.hota_metrics(ok, ok, 0, "cuda:0")


def test_prepare_and_assemble_match_the_reference(monkeypatch):
    """`hota_assemble` on sums taken from the reference gives the reference's dictionaries, and `hota_prepare`'s track and session counts
    are the reference's: the host arithmetic of mot.py is the rule's"""
    mot = _no_device(monkeypatch)
    for name in ("bank", "no_hyp_tracks", "traffic"):
        gt, hyp, n_windows = hota_cases.case(name)
        ref = hota_cases.reference(name)
        p = mot.hota_prepare(gt, hyp, n_windows)
        S = p["n_sessions"]
        assert p["n_gt"].tolist() == ref["n_gt"] and p["n_hyp"].tolist() == ref["n_hyp"] and p["c_off"].tolist() == np.concatenate([[0], np.cumsum(ref["cells"])]).tolist()
        assert p["gc"].dtype == np.int32 and p["tc"].dtype == np.int32 and int(p["gc"].sum()) == sum(ref["n_gt"])
        assert int(p["tc"].sum()) == int((np.asarray(hyp[2]) >= 0).sum()) and len(p["tc"]) == max(1, int(p["hyp"]["trk_off"][-1]))
        res = {"tp": np.stack(ref["tp"]), "loc": np.array(ref["loc"], np.uint64).reshape(S, 19), "num": np.stack(ref["num"])}
        got = mot.hota_assemble(p, res)
        assert tuple(got["overall"]) == mot.HOTA_KEYS and sorted(got) == ["alphas", "overall", "sessions"]
        for a, b in zip([got["overall"]] + got["sessions"], [ref["overall"]] + ref["sessions"]):
            for k in mot.HOTA_KEYS:
                assert a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]), (name, k)
                assert type(a[k]) is float
        for a, b in zip([got["alphas"]["overall"]] + got["alphas"]["sessions"], [ref["alphas"]["overall"]] + ref["alphas"]["sessions"]):
            assert np.array_equal(a["tp"], b["tp"]) and a["tp"].dtype == np.int64
            for k in mot.HOTA_KEYS:
                assert np.array_equal(a[k], b[k], equal_nan=True) and a[k].dtype == np.float64 and a[k].shape == (19,)
        assert np.array_equal(got["alphas"]["alpha"], mot.hota_alphas())


# ---------------------------------------------------------------------------------------------- C ABI without a GPU
P, I, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
SIGS = {"mmd_hota_align": [P, P, P, LL, P, P, P, LL, I, I, P, P, I, P, LL, P, P],
        "mmd_hota_match": [P, P, P, LL, P, P, P, LL, I, I, P, P, I, P, LL, P, P, LL, P, LL, P, P, P, P],
        "mmd_hota_assoc": [P, P, LL, P, P, P, LL, P, LL, I, I, P, P]}


def test_header_declares_and_library_exports_the_entry_points():
    import __graft_entry__ as ge
    ge.build()
    from mm_distillnet_amd import _lib
    sigs = _lib.LIB.symbols()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name, types in SIGS.items():
        assert sigs[name] == types and hasattr(dll, name), name
    text = open(_lib.HEADER).read()

    def comment_of(name):
        lines = text[:text.index("int %s(" % name)].rstrip("\n").split("\n")
        out = []
        while lines and lines[-1].startswith("//"):
            out.append(lines.pop()[2:].strip())
        return " ".join(reversed(out))

    assert "CALLER ZEROES P" in comment_of("mmd_hota_align")
    assert "CALLER ZEROES hist, tp and loc" in comment_of("mmd_hota_match")
    assert "needs no zeroing" in comment_of("mmd_hota_assoc") and "two runs give the same bits" in comment_of("mmd_hota_assoc")


def test_bad_arguments_are_rejected_without_gpu():
    import __graft_entry__ as ge
    ge.build()
    from mm_distillnet_amd import _lib
    dll = _lib.LIB.load()
    p = ctypes.c_void_p(4096)            # never dereferenced: validation precedes any launch
    sizes = (dict(n_g=-1), dict(n_h=-1), dict(S=0), dict(S=65536), dict(W=0), dict(W=(1 << 20) + 1), dict(n_g=1 << 31), dict(most=0), dict(most=1025),
             dict(c_total=0), dict(c_total=(1 << 28) // 19 + 1))

    def align(ptrs=None, n_g=5, n_h=5, S=1, W=3, most=4, c_total=16):
        q = [p] * 10 if ptrs is None else ptrs
        return dll.mmd_hota_align(q[0], q[1], q[2], n_g, q[3], q[4], q[5], n_h, S, W, q[6], q[7], most, q[8], c_total, q[9], None)

    def match(ptrs=None, n_g=5, n_h=5, S=1, W=3, most=4, c_total=16, T_g=4, T_h=4):
        q = [p] * 15 if ptrs is None else ptrs
        return dll.mmd_hota_match(q[0], q[1], q[2], n_g, q[3], q[4], q[5], n_h, S, W, q[6], q[7], most, q[8], c_total, q[9], q[10], T_g, q[11], T_h,
                                  q[12], q[13], q[14], None)

    def assoc(ptrs=None, S=1, most=4, c_total=16, T_g=4, T_h=4):
        q = [p] * 7 if ptrs is None else ptrs
        return dll.mmd_hota_assoc(q[0], q[1], c_total, q[2], q[3], q[4], T_g, q[5], T_h, S, most, q[6], None)

    for fn, n in ((align, 10), (match, 15), (assoc, 7)):
        for k in range(n):
            assert fn([None if j == k else p for j in range(n)]) == -22, (fn.__name__, k)
    for bad in sizes:
        assert align(**bad) == -22 and match(**bad) == -22, bad
    for bad in (dict(S=0), dict(S=65536), dict(most=0), dict(most=1025), dict(c_total=0), dict(c_total=(1 << 28) // 19 + 1)):
        assert assoc(**bad) == -22, bad
    for bad in (dict(T_g=-1), dict(T_h=-1), dict(T_g=1 << 27), dict(T_h=1 << 27)):
        assert match(**bad) == -22 and assoc(**bad) == -22, bad
