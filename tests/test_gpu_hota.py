"""HOTA on the GPU: mm_distillnet_amd.mot.hota_metrics (csrc/moteval.hip: mmd_hota_align, mmd_hota_match, mmd_hota_assoc) against the
numpy / scipy restatement tests/hota_ref.py.  P, hist, tp and loc are integers and are compared exactly.  The three numerators are
compared within a relative (n_cells + 2) * 2^-52: each term mc * mc / d has two roundings and the terms are nonnegative, so either
order of summation is within half of that of the exact sum.  The figures are compared within that bound plus 8 * 2^-52 (the divisions,
the square root and the mean of 19).  Every input passes the restatement's uniqueness check (tests/test_hota_ref_cpu.py asserts it for
all of tests/hota_cases.py; asserted here again): the kernels' float64 assignment then has to find the same pairs."""
import os
import sys

import numpy as np
import pytest
import torch

import hota_cases
import hota_ref
import mot_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


def _mot():
    from mm_distillnet_amd import mot
    return mot


def _flat(ref, key, dtype):
    """the per-session [G, H(, 19)] arrays of the restatement in the kernels' c_off layout"""
    parts = [np.asarray(a).reshape(-1) for a in ref[key]]
    flat = np.concatenate(parts) if sum(len(p) for p in parts) else np.zeros(0, np.int64)
    return flat.astype(dtype)


def _same_raw(raw, ref, name):
    S = len(ref["tp"])
    c_total = sum(ref["cells"])
    assert np.array_equal(raw["P"][:c_total], _flat(ref, "P", np.uint64)), name
    assert np.array_equal(raw["hist"].reshape(-1)[:c_total * 19], _flat(ref, "hist", np.int32)), name
    assert np.array_equal(raw["tp"], np.stack(ref["tp"])) and raw["tp"].dtype == np.int64, name
    assert [[int(v) for v in row] for row in raw["loc"]] == ref["loc"], name
    for s in range(S):
        bound = (ref["cells"][s] + 2) * EPS
        want = ref["num"][s]
        assert (np.abs(raw["num"][s] - want) <= bound * np.abs(want)).all(), (name, s, np.abs(raw["num"][s] - want).max())


def _same_figures(got, ref, name):
    mot = _mot()
    bound = (max(ref["cells"] + [0]) + 2) * EPS + 8 * EPS
    assert tuple(got["overall"]) == mot.HOTA_KEYS and len(got["sessions"]) == len(ref["sessions"])
    for a, b in zip([got["overall"]] + got["sessions"], [ref["overall"]] + ref["sessions"]):
        for k in mot.HOTA_KEYS:
            assert (a[k] != a[k] and b[k] != b[k]) or abs(a[k] - b[k]) <= bound * abs(b[k]), (name, k, a[k], b[k])
    for a, b in zip([got["alphas"]["overall"]] + got["alphas"]["sessions"], [ref["alphas"]["overall"]] + ref["alphas"]["sessions"]):
        assert np.array_equal(a["tp"], b["tp"])
        for k in mot.HOTA_KEYS:
            assert ((a[k] != a[k]) == (b[k] != b[k])).all() and (np.nan_to_num(np.abs(a[k] - b[k])) <= bound * np.nan_to_num(np.abs(b[k]))).all(), (name, k)
    assert np.array_equal(got["alphas"]["alpha"], ref["alphas"]["alpha"])


def _check(name):
    mot = _mot()
    gt, hyp, n_windows = hota_cases.case(name)
    ref = hota_cases.reference(name)
    assert ref["unique"], (name, ref["margin"])
    prep = mot.hota_prepare(gt, hyp, n_windows)
    raw = mot.hota_run_device(prep, DEV, intermediates=True)
    _same_raw(raw, ref, name)
    got = mot.hota_assemble(prep, raw)
    _same_figures(got, ref, name)
    return got, ref, raw


@pytest.mark.parametrize("name", hota_cases.HAND)
def test_hand_cases_through_the_kernels(name):
    """1 x 1, 2 x 1 and 3 x 1 cells, windows with one row, unequal labels, rows without a track, a session without hypothesis tracks"""
    got, ref, raw = _check(name)
    if name == "split_track":
        assert got["overall"]["assa"] == 0.5 and got["overall"]["deta"] == 1.0 and got["overall"]["asspr"] == 1.0
    if name == "alignment_wins":
        assert raw["tp"].tolist() == [[5] * 10 + [4] * 9]
    if name == "no_hyp_tracks":
        assert ref["cells"] == [2, 0, 0] and raw["tp"][1:].tolist() == [[0] * 19] * 2 and not raw["num"][1:].any()
        assert got["sessions"][1]["deta"] == 0.0 and got["sessions"][1]["loca"] == 1.0


def test_windows_without_rows_on_either_side():
    got, ref, _ = _check("traffic")
    assert 0.0 < got["overall"]["hota"] < 1.0 and ref["n_hyp"][0] > int(ref["tp"][0][0]) > 0


@pytest.mark.parametrize("name", sorted(hota_cases.CROWDS))
def test_crowded_windows(name):
    """both transpositions, more than one wave in the arg-min, augmenting paths longer than one, 256 rows on one side and on both"""
    got, ref, raw = _check(name)
    assert raw["tp"][0, 0] > 0


def test_257_rows_are_refused_on_the_host():
    mot = _mot()
    ok = mot_cases.rec([(0, 0, mot_cases.box(0))])
    with pytest.raises(ValueError, match="gt holds 257 rows in window 0 of session 0: at most 256"):
        mot.hota_metrics(mot_cases.rec([(0, k, mot_cases.box(20 * k)) for k in range(257)]), ok, 1, DEV)


@pytest.mark.parametrize("name", ["lanes_5x300", "lanes_300x5"])
def test_more_cells_than_the_association_kernel_has_threads(name):
    got, ref, raw = _check(name)
    used = np.nonzero(ref["hist"][0].reshape(1500, 19).sum(axis=1))[0]                  # a thread's second, third, .. cell counts too
    assert ref["cells"] == [1500] and len(used) > 200 and used.max() >= 5 * 256


def test_interleaved_sessions_equal_the_sessions_alone():
    mot = _mot()
    got, ref, raw = _check("bank")
    gt, hyp, n_windows = hota_cases.case("bank")
    assert len(got["sessions"]) == 4 and ref["cells"][2] == 0 and not raw["num"][2].any() and not raw["tp"][2].any()
    assert got["sessions"][2]["deta"] != got["sessions"][2]["deta"] and got["sessions"][2]["loca"] == 1.0
    for s in (0, 1, 3):
        alone = mot.hota_metrics(tuple(a[gt[3] == s] for a in gt[:3]), tuple(a[hyp[3] == s] for a in hyp[:3]), n_windows, DEV)
        assert alone["overall"] == got["sessions"][s]
    assert got["alphas"]["overall"]["tp"].tolist() == raw["tp"].sum(axis=0).tolist()


def _launch(prep, fill):
    """the three kernels through _lib.call: num, which needs no zeroing, is filled with the byte `fill`; P, hist, tp and loc are zeroed
    -> every output"""
    from mm_distillnet_amd import _lib
    G, H, S, W = prep["gt"], prep["hyp"], prep["n_sessions"], prep["n_windows"]
    T_g, T_h, c_total = int(G["trk_off"][-1]), int(H["trk_off"][-1]), prep["c_total"]

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if len(a) else None

    a = [dev(G["rows"]), dev(G["dense"]), dev(G["off"]), len(G["rows"]), dev(H["rows"]), dev(H["dense"]), dev(H["off"]), len(H["rows"]), S, W]
    g_toff, h_toff, c_off, gc, tc = dev(G["trk_off"]), dev(H["trk_off"]), dev(prep["c_off"][:-1]), dev(prep["gc"]), dev(prep["tc"])
    most = max(1, int(np.diff(G["trk_off"]).max()), int(np.diff(H["trk_off"]).max()))
    P = torch.zeros(c_total, dtype=torch.int64, device=DEV)
    hist = torch.zeros(c_total * 19, dtype=torch.int32, device=DEV)
    tp, loc = torch.zeros(S * 19, dtype=torch.int64, device=DEV), torch.zeros(S * 19, dtype=torch.int64, device=DEV)
    num = torch.full((S * 57 * 8,), fill, dtype=torch.uint8, device=DEV).view(torch.float64)
    _lib.call("mmd_hota_align", *a, g_toff, h_toff, most, c_off, c_total, P)
    _lib.call("mmd_hota_match", *a, g_toff, h_toff, most, c_off, c_total, P, gc, T_g, tc, T_h, hist, tp, loc)
    _lib.call("mmd_hota_assoc", hist, c_off, c_total, g_toff, h_toff, gc, T_g, tc, T_h, S, most, num)
    torch.cuda.synchronize()
    return {"P": P.cpu().numpy().view(np.uint64), "hist": hist.cpu().numpy().reshape(c_total, 19), "tp": tp.cpu().numpy().reshape(S, 19),
            "loc": loc.cpu().numpy().view(np.uint64).reshape(S, 19), "num": num.cpu().numpy().reshape(S, 19, 3)}


@pytest.mark.parametrize("name", ["bank", "crowd_70x70", "lanes_5x300"])
def test_raw_launches_dirty_buffers_and_two_runs_give_the_same_bits(name):
    mot = _mot()
    gt, hyp, n_windows = hota_cases.case(name)
    ref = hota_cases.reference(name)
    prep = mot.hota_prepare(gt, hyp, n_windows)
    a, b = _launch(prep, 0xA5), _launch(prep, 0x5A)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    _same_raw(a, ref, name)
    c = mot.hota_run_device(prep, DEV, intermediates=True)
    for k in a:
        assert a[k].tobytes() == c[k].tobytes(), k


def test_end_to_end_through_the_cli(tmp_path):
    """the CSVs detect.py writes -> evaluate_tracks.py --hota: the HOTA keys behind the others, the figures the restatement's"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import detect
    import evaluate_tracks as cli
    mot = _mot()
    gt, hyp, n_windows = hota_cases.case("bank")
    detect.write_windows_csv(str(tmp_path / "gt.csv"), gt[0], gt[1], 4410, gt[2], gt[3])
    detect.write_windows_csv(str(tmp_path / "pred.csv"), hyp[0], hyp[1], 4410, hyp[2], hyp[3])
    base = ["--gt", str(tmp_path / "gt.csv"), "--pred", str(tmp_path / "pred.csv")]
    plain = cli.evaluate(cli.parse_args(base), DEV)
    got = cli.evaluate(cli.parse_args(base + ["--hota", "--iou", "0.3"]), DEV)
    assert tuple(plain["overall"]) == mot.KEYS and tuple(got["overall"]) == mot.KEYS + mot.HOTA_KEYS
    ref = hota_cases.reference("bank")
    bound = (max(ref["cells"]) + 10) * EPS
    for a, b in zip([got["overall"]] + got["sessions"], [ref["overall"]] + ref["sessions"]):
        for k in mot.HOTA_KEYS:
            assert (a[k] != a[k] and b[k] != b[k]) or abs(a[k] - b[k]) <= bound * abs(b[k]), k
    assert cli.write_metrics_csv(str(tmp_path / "m.csv"), got) == 5
