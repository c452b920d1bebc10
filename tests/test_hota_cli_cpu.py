"""CPU: evaluate_tracks.py --hota, with the two device calls replaced by the restatements: the HOTA keys follow the other keys on every
line and row, --no_identity keeps them, and without --hota the output is what it was."""
import importlib
import math
import os
import sys

import pytest

import hota_ref
import mot_cases
import mot_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module(name)


@pytest.fixture()
def setup(tmp_path, monkeypatch):
    cli, det = _load("evaluate_tracks"), _load("detect")
    recs = [mot_cases.traffic(s)[:2] for s in (3, 4)]
    gt = mot_cases.interleave([r[0] for r in recs], 1)
    hyp = mot_cases.interleave([r[1] for r in recs], 2)
    det.write_windows_csv(str(tmp_path / "gt.csv"), gt[0], gt[1], 4410, gt[2], gt[3])
    det.write_windows_csv(str(tmp_path / "pred.csv"), hyp[0], hyp[1], 4410, hyp[2], hyp[3])
    from mm_distillnet_amd import mot
    seen = {"mot": [], "hota": []}

    def fake_mot(gt, hyp, n_windows, device, iou_min=0.5, identity=True):
        seen["mot"].append(dict(n_windows=n_windows, iou_min=iou_min, identity=identity, device=device))
        r = mot_ref.evaluate(gt, hyp, n_windows, iou_min, identity)
        return {k: r[k] for k in ("overall", "sessions", "gt_tracks")}

    def fake_hota(gt, hyp, n_windows, device):
        seen["hota"].append(dict(n_windows=n_windows, device=device))
        mot.hota_prepare(gt, hyp, n_windows)
        r = hota_ref.evaluate(gt, hyp, n_windows)
        return {k: r[k] for k in ("overall", "sessions", "alphas")}
    monkeypatch.setattr(mot, "mot_metrics", fake_mot)
    monkeypatch.setattr(mot, "hota_metrics", fake_hota)
    args = ["--gt", str(tmp_path / "gt.csv"), "--pred", str(tmp_path / "pred.csv")]
    return cli, mot, seen, args, tmp_path, hota_ref.evaluate(gt, hyp, 12)


def _csv(path):
    return open(path, newline="").read().split("\r\n")


def test_hota_appends_its_keys(setup, capsys):
    cli, mot, seen, args, tmp, ref = setup
    result = cli.main(args + ["--hota", "--iou", "0.4", "--output", str(tmp / "h.csv")])
    # mot_metrics is called as before; hota_metrics gets no iou
    assert seen["mot"] == [dict(n_windows=12, iou_min=0.4, identity=True, device="cuda:0")] and seen["hota"] == [dict(n_windows=12, device="cuda:0")]
    assert tuple(result["overall"]) == mot.KEYS + mot.HOTA_KEYS
    lines = capsys.readouterr().out.strip().split("\n")
    assert len(lines) == 3 and lines[0].startswith("session 0: n_gt ") and lines[2].startswith("overall: n_gt ")
    for line in lines:
        words = line.split(": ", 1)[1].split(" ")
        assert tuple(words[0::2]) == mot.KEYS + mot.HOTA_KEYS
    text = _csv(tmp / "h.csv")
    assert text[0] == "session," + ",".join(mot.KEYS + mot.HOTA_KEYS) and len(text) == 5 and text[4] == ""
    for row, want in zip(text[1:4], ref["sessions"] + [ref["overall"]]):
        cells = row.split(",")
        assert len(cells) == 1 + len(mot.KEYS) + len(mot.HOTA_KEYS)
        for k, v in zip(mot.HOTA_KEYS, cells[-len(mot.HOTA_KEYS):]):
            assert abs(float(v) - want[k]) <= 1e-8 * abs(want[k]) or (math.isnan(want[k]) and v == "nan"), k
    assert 0.0 < ref["overall"]["hota"] < 1.0


def test_hota_without_identity(setup):
    cli, mot, seen, args, tmp, ref = setup
    cli.main(args + ["--no_identity", "--hota", "--output", str(tmp / "n.csv")])
    assert seen["mot"][0]["identity"] is False and len(seen["hota"]) == 1
    text = _csv(tmp / "n.csv")
    assert text[0] == "session," + ",".join(mot.CLEAR_KEYS + mot.HOTA_KEYS)
    assert all(len(row.split(",")) == 1 + len(mot.CLEAR_KEYS) + len(mot.HOTA_KEYS) for row in text[1:4])


def test_without_the_flag_nothing_changes(setup, capsys):
    cli, mot, seen, args, tmp, ref = setup
    result = cli.main(args + ["--output", str(tmp / "m.csv")])
    assert seen["hota"] == [] and tuple(result["overall"]) == mot.KEYS
    plain = capsys.readouterr().out
    assert "hota" not in plain and "loca" not in plain
    # byte for byte what result_rows / write_metrics_csv make of mot_metrics' result alone, and the --hota file with its columns cut
    cli.write_metrics_csv(str(tmp / "direct.csv"), mot.mot_metrics(*cli.load_pair(args[1], args[3]), "cuda:0"))
    assert open(tmp / "m.csv", "rb").read() == open(tmp / "direct.csv", "rb").read()
    cli.main(args + ["--hota", "--output", str(tmp / "h.csv")])
    n = 1 + len(mot.KEYS)
    assert [",".join(r.split(",")[:n]) for r in _csv(tmp / "h.csv")[:4]] == _csv(tmp / "m.csv")[:4]
    assert _csv(tmp / "m.csv")[0] == "session," + ",".join(mot.KEYS)
    assert cli.parse_args(args).hota is False
    with pytest.raises(SystemExit):
        cli.parse_args(["--help"])
    assert "does not affect them" in " ".join(capsys.readouterr().out.split())       # --iou and HOTA's own thresholds
