#!/usr/bin/env python3
"""Tracking evaluation of the CSVs `detect.py --track` writes: CLEAR-MOT counts and identity measures of predicted tracks against
ground-truth tracks, on the device (`mm_distillnet_amd.mot.mot_metrics`; the rule: DESIGN.md, tracking evaluation).

    python evaluate_tracks.py --gt gt.csv --pred tracks.csv [--iou 0.5] [--no_identity] [--hota] [--output metrics.csv]

Both files have one of the two layouts of `detect.py --track`:
    window,t_start_s,x1,y1,x2,y2,score,label,track                  one recording
    session,window,t_start_s,x1,y1,x2,y2,score,label,track          a bank of recordings (several --input)
and both must have the same one.  A ground-truth file can be made from saved teacher detections with `tracker.track_rows` and
`detect.write_windows_csv`.  Every ground-truth row needs a track (>= 0); predicted rows with track -1 stay in and count as false
positives.  n_windows is 1 + the largest window index of either file.  --iou: smallest IoU at which a ground-truth and a predicted box
may be paired (labels must be equal).  --no_identity: the CLEAR counts alone (the identity measures hold at most 1024 tracks per file
and session).  --hota: HOTA, DetA, AssA, DetRe, DetPr, AssRe, AssPr and LocA (`mot.hota_metrics`: the means over HOTA's own 19
thresholds 0.05 .. 0.95, which --iou does not affect) behind the other keys.  One line per session and one overall line are printed;
--output writes them as CSV, header `session` + the keys, the overall row with an empty session."""
import argparse
import csv
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

DEVICE = "cuda:0"
BOX_COLUMNS = ("x1", "y1", "x2", "y2", "score", "label")
STREAM_COLUMNS = ("window", "t_start_s") + BOX_COLUMNS + ("track",)
BANK_COLUMNS = ("session",) + STREAM_COLUMNS


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gt", required=True, help="ground-truth tracks: a CSV in the layout detect.py --track writes")
    ap.add_argument("--pred", required=True, help="predicted tracks: the CSV of detect.py --track")
    ap.add_argument("--iou", type=float, default=0.5, help="smallest IoU at which two boxes of equal label may be paired")
    ap.add_argument("--no_identity", action="store_true", help="CLEAR counts only: no IDTP / IDF1")
    ap.add_argument("--hota", action="store_true", help="append HOTA, DetA, AssA, DetRe, DetPr, AssRe, AssPr, LocA (means over the thresholds "
                                                        "0.05 .. 0.95; --iou does not affect them)")
    ap.add_argument("--output", default=None, help="write the per-session and overall figures as CSV")
    a = ap.parse_args(argv)
    if not (0.0 < a.iou <= 1.0):
        raise ValueError(f"--iou {a.iou}: 0 < iou <= 1")
    return a


def read_tracks_csv(path: str):
    """-> (rows float32 [R, 6], window int64 [R], track int64 [R], session int64 [R] or None)"""
    with open(path, newline="") as f:
        reader = csv.reader(f)
        header = tuple(next(reader, ()))
        if header in (STREAM_COLUMNS[:-1], BANK_COLUMNS[:-1]):
            raise ValueError(f"{path}: no `track` column: tracking evaluation needs the CSV detect.py writes with --track")
        if header not in (STREAM_COLUMNS, BANK_COLUMNS):
            raise ValueError(f"{path}: header {','.join(header)!r} is neither {','.join(STREAM_COLUMNS)} nor {','.join(BANK_COLUMNS)}")
        bank = header == BANK_COLUMNS
        rows, window, track, session = [], [], [], []
        for n, line in enumerate(reader, 2):
            if not line:
                continue
            if len(line) != len(header):
                raise ValueError(f"{path}:{n}: {len(line)} fields, the header has {len(header)}")
            try:
                q = line[1:] if bank else line
                if bank:
                    session.append(int(line[0]))
                window.append(int(q[0]))
                rows.append([float(v) for v in q[2:8]])
                track.append(int(q[8]))
            except ValueError:
                raise ValueError(f"{path}:{n}: not a row of numbers: {','.join(line)!r}") from None
    return (np.asarray(rows, np.float32).reshape(-1, 6), np.asarray(window, np.int64), np.asarray(track, np.int64),
            np.asarray(session, np.int64) if bank else None)


def load_pair(gt_path: str, pred_path: str):
    """-> (gt, hyp, n_windows): the two records as `mot_metrics` takes them"""
    g, h = read_tracks_csv(gt_path), read_tracks_csv(pred_path)
    if (g[3] is None) != (h[3] is None):
        raise ValueError(f"{gt_path} and {pred_path} differ in layout: one has a `session` column, the other has none")
    n_windows = 1 + max([int(r[1].max()) for r in (g, h) if len(r[1])] + [0])
    strip = (lambda r: r[:3]) if g[3] is None else (lambda r: r)
    return strip(g), strip(h), n_windows


def result_rows(result: dict):
    """-> (header, rows): `session` + the keys; one row per session, then the overall row with an empty session"""
    keys = list(result["overall"].keys())

    def cell(v):
        return str(v) if isinstance(v, (int, np.integer)) else ("nan" if v != v else "%.9g" % v)

    rows = [[str(s)] + [cell(d[k]) for k in keys] for s, d in enumerate(result["sessions"])]
    rows.append([""] + [cell(result["overall"][k]) for k in keys])
    return ["session"] + keys, rows


def write_metrics_csv(path: str, result: dict) -> int:
    header, rows = result_rows(result)
    with open(path, "w", newline="") as f:
        out = csv.writer(f)
        out.writerow(header)
        out.writerows(rows)
    return len(rows)


def format_lines(result: dict):
    header, rows = result_rows(result)
    return ["%s: %s" % ("session " + r[0] if r[0] else "overall", " ".join("%s %s" % kv for kv in zip(header[1:], r[1:]))) for r in rows]


def evaluate(a, device=DEVICE) -> dict:
    from mm_distillnet_amd.mot import mot_metrics
    gt, hyp, n_windows = load_pair(a.gt, a.pred)
    result = mot_metrics(gt, hyp, n_windows, device, iou_min=a.iou, identity=not a.no_identity)
    if a.hota:
        from mm_distillnet_amd import mot
        hota = mot.hota_metrics(gt, hyp, n_windows, device)
        for d, h in zip([result["overall"]] + result["sessions"], [hota["overall"]] + hota["sessions"]):
            d.update((k, h[k]) for k in mot.HOTA_KEYS)
    return result


def main(argv=None):
    a = parse_args(argv)
    result = evaluate(a)
    for line in format_lines(result):
        print(line)
    if a.output:
        write_metrics_csv(a.output, result)
    return result


if __name__ == "__main__":
    main()
