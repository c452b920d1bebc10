"""Tracking evaluation on the GPU: mm_distillnet_amd.mot (csrc/moteval.hip: mmd_mot_clear, mmd_mot_id_counts, mmd_mot_id_assign) against
the numpy / scipy restatement tests/mot_ref.py.  Integer counts and the per-track arrays are compared exactly; iou_sum within a relative
n_pairs * 2^-52 (a float64 sum of positive terms in another order differs by at most that), MOTP within two more roundings.  Every
random CLEAR input must pass the reference's uniqueness check (each assign step's optimum is the only one within 1e-6), which is
ASSERTED: the seeds below were picked so that it holds."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import mot_cases
import mot_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


def _mot():
    from mm_distillnet_amd import mot
    return mot


@functools.lru_cache(maxsize=None)
def _case(name):
    """name -> (gt, hyp, n_windows, iou_min, reference with the uniqueness check); computed once, never changed"""
    hand = mot_cases.hand_cases()
    if name in hand:
        gt, hyp, n_windows, iou_min, _ = hand[name]
    elif name == "traffic":                      # windows without ground truth, without hypotheses, with neither
        gt, hyp, n_windows, iou_min = mot_cases.traffic(1)
    elif name.startswith("crowd_"):              # crowd_<ng>x<nh>
        ng, nh = (int(v) for v in name[6:].split("x"))
        gt, hyp, n_windows, iou_min = mot_cases.crowd(7 + ng + 3 * nh, ng, nh)
    elif name == "bank":                         # sessions 0, 1, 3 interleaved; session 2 has no row at all
        recs = [mot_cases.traffic(s) for s in (21, 22, 23)]
        def merged(k, seed):
            got = mot_cases.interleave([r[k] for r in recs], seed)
            return got[:3] + (np.where(got[3] == 2, 3, got[3]),)
        gt, hyp, n_windows, iou_min = merged(0, 1), merged(1, 2), 12, 0.5
    elif name in ("lanes_5x300", "lanes_300x5"):
        gt, hyp, n_windows, iou_min = _lanes(31)
        if name == "lanes_300x5":
            gt, hyp = hyp, gt
    else:
        raise KeyError(name)
    return gt, hyp, n_windows, iou_min, mot_ref.evaluate(gt, hyp, n_windows, iou_min, check_unique=True)


def _lanes(seed, n_lanes=5, pool=60, W=80):
    """5 ground-truth tracks on 5 lanes, 300 hypothesis tracks: lane k's hypothesis changes its id (out of `pool` ids of its own) from
    window to window and now and then sits on the next lane's vehicle, so C [5, 300] has small counts off the diagonal blocks too"""
    r = np.random.RandomState(seed)
    g, h = [], []
    for w in range(W):
        for k in range(n_lanes):
            x, y = 3.0 * w, 25.0 * k
            g.append((w, k, [x, y, x + 30.0, y + 20.0, 1.0, 6.0]))
            tid = 1000 * k + (w if w < pool else int(r.randint(pool)))
            yy = y + (25.0 if r.rand() < 0.3 and k + 1 < n_lanes else 0.0) + r.normal(0, 1.0)
            xx = x + r.normal(0, 1.0)
            h.append((w, tid, [xx, yy, xx + 30.0, yy + 20.0, 0.8, 6.0]))
    return mot_cases.rec(g), mot_cases.rec(h), W, 0.5


def _same_dicts(got, ref, pairs):
    mot = _mot()
    for k in got:
        a, b = got[k], ref[k]
        if k == "motp":
            assert (a != a and b != b) or abs(a - b) <= (pairs + 2) * EPS * abs(b), (k, a, b)
        else:
            assert a == b or (a != a and b != b), (k, a, b)
            assert type(a) is (int if k in ("n_gt", "n_hyp", "tp", "fp", "fn", "idsw", "frag", "mt", "pt", "ml", "idtp", "idfp", "idfn") else float), k
    assert tuple(got) == (mot.KEYS if "idtp" in ref else mot.CLEAR_KEYS)


def _check(name, identity=True):
    mot = _mot()
    gt, hyp, n_windows, iou_min, ref = _case(name)
    assert ref["unique"], (name, ref["margin"])
    prep = mot.prepare(gt, hyp, n_windows, iou_min, identity)
    raw = mot.run_device(prep, DEV)
    for s, want in enumerate(ref["iou_sums"]):
        assert abs(raw["iou_sum"][s] - want) <= ref["pairs"][s] * EPS * want, (name, s)
    got = mot.assemble(prep, raw)
    assert np.array_equal(got["gt_tracks"], ref["gt_tracks"]) and got["gt_tracks"].dtype == np.int64
    assert len(got["sessions"]) == len(ref["sessions"])
    ref_d = [ref["overall"]] + ref["sessions"]
    if not identity:
        ref_d = [{k: v for k, v in d.items() if k in mot.CLEAR_KEYS} for d in ref_d]
    for a, b in zip([got["overall"]] + got["sessions"], ref_d):
        _same_dicts(a, b, ref["overall"]["tp"])
    return got, ref


@pytest.mark.parametrize("name", sorted(mot_cases.hand_cases()))
def test_hand_cases_through_the_kernels(name):
    got, _ = _check(name)
    want = mot_cases.hand_cases()[name][4]
    assert {k: got["overall"][k] for k in want} == want


def test_windows_without_rows_on_either_side():
    got, ref = _check("traffic")
    assert ref["overall"]["idsw"] > 0 and ref["overall"]["fn"] > 0 and ref["overall"]["fp"] > 0 and ref["overall"]["frag"] > 0
    _check("traffic", identity=False)


@pytest.mark.parametrize("name", ["crowd_5x9", "crowd_9x5", "crowd_70x70", "crowd_256x256"])
def test_crowded_windows(name):
    """both transpositions, more than one wave in the arg-min, augmenting paths longer than one, the cap of 256 rows"""
    got, ref = _check(name)
    assert ref["overall"]["tp"] > 0 and ref["overall"]["idsw"] > 0


def test_interleaved_sessions_equal_the_sessions_alone():
    mot = _mot()
    got, ref = _check("bank")
    gt, hyp, n_windows, iou_min, _ = _case("bank")
    assert len(got["sessions"]) == 4 and got["sessions"][2]["n_gt"] == 0 and got["sessions"][2]["n_hyp"] == 0
    assert got["sessions"][2]["mota"] != got["sessions"][2]["mota"] and got["sessions"][2]["idtp"] == 0
    for s in (0, 1, 3):
        alone = mot.mot_metrics(tuple(a[gt[3] == s] for a in gt[:3]), tuple(a[hyp[3] == s] for a in hyp[:3]), n_windows, DEV, iou_min)
        assert alone["overall"] == got["sessions"][s]
        assert np.array_equal(alone["gt_tracks"][:, 1:], got["gt_tracks"][got["gt_tracks"][:, 0] == s][:, 1:])
    total = sum(got["sessions"][s]["idtp"] for s in range(4))
    assert got["overall"]["idtp"] == total and got["overall"]["tp"] == sum(d["tp"] for d in got["sessions"])


@pytest.mark.parametrize("name", ["lanes_5x300", "lanes_300x5"])
def test_identity_with_columns_strided_past_256(name):
    got, ref = _check(name)
    gt, hyp = _case(name)[:2]
    assert sorted((len(np.unique(gt[2])), len(np.unique(hyp[2])))) == [5, 300]
    assert 0 < ref["overall"]["idtp"] < ref["overall"]["tp"]


def test_identity_with_a_session_without_tracks_on_one_side():
    """session 0 is the identity-switch case; session 1 has ground-truth tracks and hypothesis rows, none of which has a track; session
    2 has hypothesis tracks and no ground truth"""
    mot = _mot()
    hand = mot_cases.hand_cases()
    g0, h0 = hand["id_switch"][:2]
    g1 = hand["fragmentation"][0]
    h1 = (g1[0], g1[1], np.full(len(g1[0]), -1))
    h2 = hand["fragmentation"][1]
    gt = tuple(np.concatenate([a, b]) for a, b in zip(mot_cases.with_session(g0, 0), mot_cases.with_session(g1, 1)))
    hyp = tuple(np.concatenate([a, b, c]) for a, b, c in zip(mot_cases.with_session(h0, 0), mot_cases.with_session(h1, 1), mot_cases.with_session(h2, 2)))
    ref = mot_ref.evaluate(gt, hyp, 4, 0.5, check_unique=True)
    assert ref["unique"]
    got = mot.mot_metrics(gt, hyp, 4, DEV)
    for a, b in zip([got["overall"]] + got["sessions"], [ref["overall"]] + ref["sessions"]):
        _same_dicts(a, b, ref["overall"]["tp"])
    assert [s["idtp"] for s in got["sessions"]] == [2, 0, 0] and [s["idfp"] for s in got["sessions"]] == [1, 4, 3]
    assert got["sessions"][1]["fp"] == 4 and got["sessions"][1]["fn"] == 4 and got["sessions"][2]["fp"] == 3
    assert np.array_equal(got["gt_tracks"], ref["gt_tracks"])


def _assign(mats):
    """mmd_mot_id_assign on integer matrices given directly -> idtp per matrix"""
    from mm_distillnet_amd import _lib
    G, H = [m.shape[0] for m in mats], [m.shape[1] for m in mats]
    flat = np.concatenate([np.asarray(m, np.int32).reshape(-1) for m in mats] + [np.zeros(1, np.int32)])
    c_off = np.concatenate([[0], np.cumsum([g * h for g, h in zip(G, H)])]).astype(np.int64)

    def dev(a, dt):
        return torch.from_numpy(np.asarray(a, dt)).to(DEV)
    idtp = torch.full((len(mats),), -7, dtype=torch.int64, device=DEV)              # needs no zeroing
    _lib.call("mmd_mot_id_assign", dev(flat, np.int32), dev(c_off[:-1], np.int64), len(flat), dev(np.concatenate([[0], np.cumsum(G)]), np.int32),
              dev(np.concatenate([[0], np.cumsum(H)]), np.int32), len(mats), max(1, max(G), max(H)), idtp)
    torch.cuda.synchronize()
    return idtp.cpu().numpy().tolist()


def test_identity_assignment_on_given_matrices():
    r = np.random.RandomState(5)
    mats = [np.array([[5, 4, 0], [4, 0, 0], [0, 3, 3]]),          # greedy takes 5, then 3: 8; the optimum is 4 + 4 + 3 = 11
            r.randint(0, 20, (5, 300)), r.randint(0, 20, (300, 5)), r.randint(0, 4, (70, 70)), r.randint(0, 50, (40, 260)),
            np.zeros((0, 4), np.int64), np.zeros((3, 0), np.int64), np.zeros((2, 2), np.int64),
            r.randint(0, 3, (300, 1024)) * (r.rand(300, 1024) < 0.02), np.array([[7]])]
    want = [mot_ref.id_matrix_idtp(m) for m in mats]
    assert want[0] == 11 and want[5] == 0 and want[6] == 0
    assert _assign(mats) == want


def _launch(prep, fill):
    """the three kernels on buffers filled with the byte `fill` wherever the header says no zeroing is needed -> every output, as bytes"""
    from mm_distillnet_amd import _lib
    G, H, S, W = prep["gt"], prep["hyp"], prep["n_sessions"], prep["n_windows"]
    T = int(G["trk_off"][-1])

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if len(a) else None

    def filled(n, dtype):
        return torch.full((n * torch.empty(0, dtype=dtype).element_size(),), fill, dtype=torch.uint8, device=DEV).view(dtype)
    counts, iou_sum, idtp = filled(S * 8, torch.int64), filled(S, torch.float64), filled(S, torch.int64)
    present, matched = filled(T, torch.int32), filled(T, torch.int32)
    ws = filled(int(_lib.LIB.load().mmd_mot_clear_ws_bytes(T)), torch.uint8)
    sizes = np.diff(G["trk_off"]).astype(np.int64) * np.diff(H["trk_off"]).astype(np.int64)
    c_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    C = torch.zeros(max(int(c_off[-1]), 1), dtype=torch.int32, device=DEV)
    a = [dev(G["rows"]), dev(G["dense"]), dev(G["off"]), len(G["rows"]), dev(H["rows"]), dev(H["dense"]), dev(H["off"]), len(H["rows"]), S, W]
    g_toff, h_toff, c_off_d = dev(G["trk_off"]), dev(H["trk_off"]), dev(c_off[:-1])
    most = max(1, int(np.diff(G["trk_off"]).max()), int(np.diff(H["trk_off"]).max()))
    _lib.call("mmd_mot_clear", *a, g_toff, T, prep["iou_min"], counts, iou_sum, present, matched, ws)
    _lib.call("mmd_mot_id_counts", *a, g_toff, h_toff, most, c_off_d, C.numel(), prep["iou_min"], C)
    _lib.call("mmd_mot_id_assign", C, c_off_d, C.numel(), g_toff, h_toff, S, most, idtp)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dict(counts=counts.view(S, 8), iou_sum=iou_sum, idtp=idtp, present=present, matched=matched, C=C).items()}


@pytest.mark.parametrize("name", ["bank", "crowd_70x70"])
def test_dirty_buffers_and_two_runs_give_the_same_bits(name):
    mot = _mot()
    gt, hyp, n_windows, iou_min, ref = _case(name)
    prep = mot.prepare(gt, hyp, n_windows, iou_min)
    a, b = _launch(prep, 0xA5), _launch(prep, 0x5A)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["counts"][:, 7].tolist() == [n_windows] * prep["n_sessions"]
    names = ("n_gt", "n_hyp", "tp", "fp", "fn", "idsw", "frag")
    assert [dict(zip(names, row[:7].tolist())) for row in a["counts"]] == [{k: s[k] for k in names} for s in ref["sessions"]]
    assert a["idtp"].tolist() == [s["idtp"] for s in ref["sessions"]]
    assert np.array_equal(a["present"], ref["gt_tracks"][:, 2]) and np.array_equal(a["matched"], ref["gt_tracks"][:, 3])


def test_end_to_end_track_rows_to_the_cli(tmp_path):
    """saved detections -> tracker.track_rows on both sides -> the CSVs detect.py writes -> evaluate_tracks.py's functions"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import detect
    import evaluate_tracks as cli
    from mm_distillnet_amd.tracker import TrackConfig, track_rows
    r = np.random.RandomState(3)
    W, rows, window = 40, [], []
    for w in range(W):
        for k in range(4):
            if r.rand() < 0.1:
                continue
            x, y = 4.0 * w + 2.0 * k, 45.0 * k
            rows.append([x, y, x + 30.0, y + 20.0, 0.9, 6.0 if k % 2 else 14.0])
            window.append(w)
    rows, window = np.array(rows, np.float32), np.array(window, np.int64)
    keep = r.rand(len(rows)) > 0.15
    noisy = (rows[keep] + np.concatenate([r.normal(0, 1.5, (int(keep.sum()), 4)), np.zeros((int(keep.sum()), 2))], axis=1)).astype(np.float32)
    gt_ids = track_rows(rows, window, W, TrackConfig(), DEV)
    hyp_ids = track_rows(noisy, window[keep], W, TrackConfig(iou_min=0.6, max_age=0), DEV)
    assert (gt_ids >= 0).all()
    detect.write_windows_csv(str(tmp_path / "gt.csv"), rows, window, 4410, gt_ids)
    detect.write_windows_csv(str(tmp_path / "pred.csv"), noisy, window[keep], 4410, hyp_ids)
    a = cli.parse_args(["--gt", str(tmp_path / "gt.csv"), "--pred", str(tmp_path / "pred.csv"), "--output", str(tmp_path / "m.csv")])
    got = cli.evaluate(a, DEV)
    gt, hyp, n_windows = cli.load_pair(a.gt, a.pred)
    ref = mot_ref.evaluate(gt, hyp, n_windows, 0.5, check_unique=True)
    assert ref["unique"], ref["margin"]
    assert ref["overall"]["tp"] > 50 and ref["overall"]["fn"] > 0 and ref["overall"]["idtp"] > 0
    _same_dicts(got["overall"], ref["overall"], ref["overall"]["tp"])
    assert np.array_equal(got["gt_tracks"], ref["gt_tracks"])
    assert cli.write_metrics_csv(a.output, got) == 2
