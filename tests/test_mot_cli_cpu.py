"""CPU: evaluate_tracks.py - reading the two CSV layouts `detect.py --track` writes, its refusals and its output format, without a GPU."""
import importlib
import math
import os
import sys

import numpy as np
import pytest

import mot_cases
import mot_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module(name)


@pytest.fixture(scope="module")
def cli():
    return _load("evaluate_tracks")


def test_reads_what_detect_writes(cli, tmp_path):
    det = _load("detect")
    rows = np.array([[1, 2, 30, 40, 0.1 + 0.2, 6], [0, 0, 128, 127, np.float32(1) / 3, 6], [5, 6, 7, 8, 0.999999, 14]], np.float32)
    window, track, session = np.array([0, 0, 7], np.int32), np.array([0, -1, 12], np.int32), np.array([1, 0, 1], np.int32)
    det.write_windows_csv(str(tmp_path / "one.csv"), rows, window, 1531, track)
    got = cli.read_tracks_csv(str(tmp_path / "one.csv"))
    assert np.array_equal(got[0], rows) and got[0].dtype == np.float32             # 9 digits: float32 round-trips
    assert got[1].tolist() == [0, 0, 7] and got[2].tolist() == [0, -1, 12] and got[3] is None
    det.write_windows_csv(str(tmp_path / "bank.csv"), rows, window, 1531, track, session)
    got = cli.read_tracks_csv(str(tmp_path / "bank.csv"))
    assert np.array_equal(got[0], rows) and got[1].tolist() == [0, 0, 7] and got[2].tolist() == [0, -1, 12] and got[3].tolist() == [1, 0, 1]
    # an empty record
    det.write_windows_csv(str(tmp_path / "e.csv"), np.zeros((0, 6), np.float32), np.zeros(0, np.int32), 100, np.zeros(0, np.int32))
    got = cli.read_tracks_csv(str(tmp_path / "e.csv"))
    assert got[0].shape == (0, 6) and len(got[1]) == 0 and got[3] is None
    # the pair: n_windows from the larger window index of either file
    det.write_windows_csv(str(tmp_path / "gt.csv"), rows[:1], np.array([9]), 1531, np.array([3]))
    gt, hyp, n_windows = cli.load_pair(str(tmp_path / "gt.csv"), str(tmp_path / "one.csv"))
    assert n_windows == 10 and len(gt) == 3 and len(hyp) == 3 and gt[2].tolist() == [3]
    gt, hyp, n_windows = cli.load_pair(str(tmp_path / "bank.csv"), str(tmp_path / "bank.csv"))
    assert n_windows == 8 and len(gt) == 4


def test_refusals(cli, tmp_path):
    det = _load("detect")
    rows = np.array([[1, 2, 30, 40, 0.5, 6]], np.float32)
    det.write_windows_csv(str(tmp_path / "boxes.csv"), rows, np.array([0]), 1531)
    det.write_windows_csv(str(tmp_path / "one.csv"), rows, np.array([0]), 1531, np.array([0]))
    det.write_windows_csv(str(tmp_path / "bank.csv"), rows, np.array([0]), 1531, np.array([0]), np.array([0]))
    with pytest.raises(ValueError, match=r"boxes.csv: no `track` column.*--track"):
        cli.read_tracks_csv(str(tmp_path / "boxes.csv"))
    det.write_windows_csv(str(tmp_path / "bank_boxes.csv"), rows, np.array([0]), 1531, None, np.array([0]))
    with pytest.raises(ValueError, match="--track"):
        cli.read_tracks_csv(str(tmp_path / "bank_boxes.csv"))
    with pytest.raises(ValueError, match="differ in layout"):
        cli.load_pair(str(tmp_path / "one.csv"), str(tmp_path / "bank.csv"))
    (tmp_path / "clip.csv").write_text("clip,x1,y1,x2,y2,score,label\n0,1,2,3,4,0.5,6\n")
    with pytest.raises(ValueError, match="header"):
        cli.read_tracks_csv(str(tmp_path / "clip.csv"))
    (tmp_path / "short.csv").write_text(",".join(cli.STREAM_COLUMNS) + "\n0,0,1,2,3,4,0.5,6\n")
    with pytest.raises(ValueError, match="short.csv:2: 8 fields, the header has 9"):
        cli.read_tracks_csv(str(tmp_path / "short.csv"))
    (tmp_path / "word.csv").write_text(",".join(cli.STREAM_COLUMNS) + "\n0,0,1,2,3,4,0.5,car,1\n")
    with pytest.raises(ValueError, match="word.csv:2: not a row of numbers"):
        cli.read_tracks_csv(str(tmp_path / "word.csv"))
    with pytest.raises(ValueError, match="--iou"):
        cli.parse_args(["--gt", "a", "--pred", "b", "--iou", "0"])
    with pytest.raises(SystemExit):
        cli.parse_args(["--gt", "a"])
    a = cli.parse_args(["--gt", "a", "--pred", "b"])
    assert a.iou == 0.5 and not a.no_identity and a.output is None


def test_output_format(cli, tmp_path, capsys, monkeypatch):
    """main() with the device call replaced by the reference: the printed lines and the CSV"""
    det = _load("detect")
    recs = [mot_cases.traffic(s)[:2] for s in (3, 4)]
    gt = mot_cases.interleave([r[0] for r in recs], 1)
    hyp = mot_cases.interleave([r[1] for r in recs], 2)
    det.write_windows_csv(str(tmp_path / "gt.csv"), gt[0], gt[1], 4410, gt[2], gt[3])
    det.write_windows_csv(str(tmp_path / "pred.csv"), hyp[0], hyp[1], 4410, hyp[2], hyp[3])
    from mm_distillnet_amd import mot
    seen = {}

    def fake(gt, hyp, n_windows, device, iou_min=0.5, identity=True):
        seen.update(n_windows=n_windows, iou_min=iou_min, identity=identity, device=device)
        mot.prepare(gt, hyp, n_windows, iou_min, identity)
        r = mot_ref.evaluate(gt, hyp, n_windows, iou_min, identity)
        return {k: r[k] for k in ("overall", "sessions", "gt_tracks")}
    monkeypatch.setattr(mot, "mot_metrics", fake)
    result = cli.main(["--gt", str(tmp_path / "gt.csv"), "--pred", str(tmp_path / "pred.csv"), "--iou", "0.4", "--output", str(tmp_path / "m.csv")])
    assert seen == dict(n_windows=12, iou_min=0.4, identity=True, device="cuda:0")
    lines = capsys.readouterr().out.strip().split("\n")
    assert len(lines) == 3 and lines[0].startswith("session 0: n_gt ") and lines[1].startswith("session 1: n_gt ") and lines[2].startswith("overall: n_gt ")
    assert " idf1 " in lines[2] and " mota " in lines[2]
    text = open(tmp_path / "m.csv", newline="").read().split("\r\n")
    assert text[0] == "session," + ",".join(mot.KEYS) and len(text) == 5 and text[4] == ""
    assert text[1].startswith("0,") and text[2].startswith("1,") and text[3].startswith(",")
    o = text[3].split(",")
    assert len(o) == 1 + len(mot.KEYS)
    for k, v in zip(mot.KEYS, o[1:]):
        w = result["overall"][k]
        assert (int(v) == w) if isinstance(w, int) else (abs(float(v) - w) <= 1e-8 * abs(w) or (math.isnan(w) and v == "nan")), k
    # --no_identity: the id columns are gone
    cli.main(["--gt", str(tmp_path / "gt.csv"), "--pred", str(tmp_path / "pred.csv"), "--no_identity", "--output", str(tmp_path / "n.csv")])
    assert seen["identity"] is False and seen["iou_min"] == 0.5
    assert open(tmp_path / "n.csv", newline="").read().split("\r\n")[0] == "session," + ",".join(mot.CLEAR_KEYS)
