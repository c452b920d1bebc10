"""Tracking evaluation: the CLEAR-MOT counts (MOTA, MOTP, FP, FN, identity switches, fragmentations, MT / PT / ML) and the identity
measures (IDTP / IDFP / IDFN, IDP, IDR, IDF1) of a tracked record against a ground-truth record, on the device (csrc/moteval.hip:
`mmd_mot_clear`, `mmd_mot_id_counts`, `mmd_mot_id_assign`).

The rule is written out in DESIGN.md (tracking evaluation) and in include/mmdistill.h; tests/mot_ref.py restates it with numpy and
scipy.  A record is what `AudioDetector.track_stream`, `tracker.track_rows` or a `LiveBank` return: rows float32 [R, 6] (x1, y1, x2, y2,
score, label), window int [R], track int [R][, session int [R]].  The ground truth may be a record of tracks made from a teacher's boxes
with `tracker.track_rows`.  Validation, the stable sort by (session, window), the dense track ids and the offset tables are host work
(`prepare`); the device gets one upload, the kernels run on the current stream, and the host waits and copies once."""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np

ROWS_MAX = 256              # rows of one side in one window (the tracker's DET_MAX)
ID_TRACKS_MAX = 1024        # tracks per side and session of the identity measures
CLEAR_KEYS = ("n_gt", "n_hyp", "tp", "fp", "fn", "idsw", "frag", "mt", "pt", "ml", "mota", "motp", "precision", "recall")
ID_KEYS = ("idtp", "idfp", "idfn", "idp", "idr", "idf1")
KEYS = CLEAR_KEYS + ID_KEYS


def _ratio(a, b) -> float:
    return float(a) / float(b) if b else float("nan")


def derive(c: Dict[str, int], iou_sum: float, present, matched, idtp: Optional[int]) -> dict:
    """The figures of one session, or of all sessions from summed counts: c holds n_gt n_hyp tp fp fn idsw frag, present / matched the
    per-track window counts; idtp None: without the identity keys.  A ratio with a zero denominator is NaN."""
    present, matched = np.asarray(present, np.int64), np.asarray(matched, np.int64)
    share = matched / np.maximum(present, 1)
    mt, ml = int((share >= 0.8).sum()), int((share <= 0.2).sum())
    out = {k: int(c[k]) for k in ("n_gt", "n_hyp", "tp", "fp", "fn", "idsw", "frag")}
    out.update(mt=mt, pt=len(present) - mt - ml, ml=ml,
               mota=1.0 - _ratio(c["fn"] + c["fp"] + c["idsw"], c["n_gt"]) if c["n_gt"] else float("nan"),
               motp=_ratio(iou_sum, c["tp"]), precision=_ratio(c["tp"], c["tp"] + c["fp"]), recall=_ratio(c["tp"], c["n_gt"]))
    if idtp is not None:
        idtp = int(idtp)
        idfp, idfn = out["n_hyp"] - idtp, out["n_gt"] - idtp
        out.update(idtp=idtp, idfp=idfp, idfn=idfn, idp=_ratio(idtp, idtp + idfp), idr=_ratio(idtp, idtp + idfn),
                   idf1=_ratio(2 * idtp, 2 * idtp + idfp + idfn))
    return out


def _side(rec, name: str, n_windows: int, is_gt: bool):
    if not isinstance(rec, (tuple, list)) or len(rec) not in (3, 4):
        raise ValueError("mot_metrics: %s is (rows, window, track[, session]), got %d items" % (name, len(rec) if hasattr(rec, "__len__") else 0))
    rows = np.ascontiguousarray(np.asarray(rec[0], np.float32).reshape(-1, 6))
    window = np.asarray(rec[1]).reshape(-1).astype(np.int64)
    track = np.asarray(rec[2]).reshape(-1).astype(np.int64)
    session = np.zeros(len(rows), np.int64) if len(rec) == 3 else np.asarray(rec[3]).reshape(-1).astype(np.int64)
    R = len(rows)
    if not (len(window) == len(track) == len(session) == R):
        raise ValueError("mot_metrics: %s has %d rows, %d window indices, %d track ids, %d session indices"
                         % (name, R, len(window), len(track), len(session)))
    if R and (window.min() < 0 or window.max() >= n_windows):
        raise ValueError("mot_metrics: %s window indices must lie inside 0 .. n_windows-1 = %d" % (name, n_windows - 1))
    if R and (session.min() < 0 or session.max() >= 65535):
        raise ValueError("mot_metrics: %s session indices must lie inside 0 .. 65534" % name)
    if is_gt and R and track.min() < 0:
        raise ValueError("mot_metrics: gt row %d has track %d: every ground-truth row belongs to a track"
                         % (int(np.argmax(track < 0)), int(track.min())))
    if R and track.min() < -1:
        raise ValueError("mot_metrics: %s track ids are >= 0, or -1 for a row without a track" % name)
    return rows, window, track, session


def _sorted_side(side, name: str, n_sessions: int, n_windows: int) -> dict:
    rows, window, track, session = side
    key = session * n_windows + window
    order = np.argsort(key, kind="stable")
    rows, window, track, session, key = rows[order], window[order], track[order], session[order], key[order]
    off = np.searchsorted(key, np.arange(n_sessions * n_windows + 1)).astype(np.int32)
    per = np.diff(off)
    if len(per) and per.max() > ROWS_MAX:
        k = int(np.argmax(per))
        raise ValueError("mot_metrics: %s holds %d rows in window %d of session %d: at most %d rows of one side in one window"
                         % (name, int(per.max()), k % n_windows, k // n_windows, ROWS_MAX))
    has = track >= 0
    span = int(track.max()) + 1 if has.any() else 1
    wt = key[has] * span + track[has]
    if len(wt) and len(np.unique(wt)) != len(wt):
        u, n = np.unique(wt, return_counts=True)
        d = int(u[np.argmax(n > 1)])
        raise ValueError("mot_metrics: %s track %d occurs more than once in window %d of session %d"
                         % (name, d % span, (d // span) % n_windows, d // span // n_windows))
    # dense ids per session: the session's ids in rising order
    st = session[has] * span + track[has]
    uniq, inv = np.unique(st, return_inverse=True)
    u_sess, u_id = uniq // span, uniq % span
    trk_off = np.searchsorted(u_sess, np.arange(n_sessions + 1)).astype(np.int64)
    dense = np.full(len(track), -1, np.int64)
    dense[has] = inv.reshape(-1) - trk_off[session[has]]
    return {"rows": rows, "dense": dense.astype(np.int32), "off": off, "trk_off": trk_off.astype(np.int32), "u_sess": u_sess, "u_id": u_id,
            "session": session}


def prepare(gt, hyp, n_windows: int, iou_min: float = 0.5, identity: bool = True) -> dict:
    """The host side of `mot_metrics`: every check, the stable sort, the dense ids and the offset tables.  Touches neither the library
    nor the device; raises ValueError on every input `mot_metrics` refuses."""
    n_windows = int(n_windows)
    if n_windows < 1:
        raise ValueError("mot_metrics: n_windows = %d (at least 1)" % n_windows)
    if not (0.0 < float(iou_min) <= 1.0):
        raise ValueError("mot_metrics: iou_min = %r (0 < iou_min <= 1)" % (iou_min,))
    g, h = _side(gt, "gt", n_windows, True), _side(hyp, "hyp", n_windows, False)
    n_sessions = 1 + max([int(s[3].max()) for s in (g, h) if len(s[3])] + [0])
    if n_sessions * n_windows >= 2 ** 31 - 1:
        raise ValueError("mot_metrics: %d sessions of %d windows: the offset table is indexed with 32 bits" % (n_sessions, n_windows))
    G, H = _sorted_side(g, "gt", n_sessions, n_windows), _sorted_side(h, "hyp", n_sessions, n_windows)
    if identity:
        most = max(int(np.diff(G["trk_off"]).max()), int(np.diff(H["trk_off"]).max()))
        if most > ID_TRACKS_MAX:
            raise ValueError("mot_metrics: %d tracks of one side in one session: the identity measures hold at most %d "
                             "(identity=False evaluates the CLEAR counts alone)" % (most, ID_TRACKS_MAX))
    return {"gt": G, "hyp": H, "n_sessions": n_sessions, "n_windows": n_windows, "iou_min": float(iou_min), "identity": bool(identity)}


def _pack(arrays) -> Tuple[np.ndarray, List[Tuple[int, int]]]:
    """-> (one uint8 buffer holding every array at a 16-byte boundary, [(offset, bytes)])"""
    spans, at = [], 0
    for a in arrays:
        spans.append((at, a.nbytes))
        at += (a.nbytes + 15) // 16 * 16
    buf = np.zeros(max(at, 16), np.uint8)
    for a, (o, n) in zip(arrays, spans):
        buf[o:o + n] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return buf, spans


def run_device(prep: dict, device) -> dict:
    """The kernels on what `prepare` made: one upload, three launches on the current stream, one synchronise, one copy back.
    -> {"counts" int64 [S, 8], "iou_sum" float64 [S], "present" / "matched" int32 [tracks], "idtp" int64 [S] or None}"""
    import torch

    from . import _lib
    G, H, S, W = prep["gt"], prep["hyp"], prep["n_sessions"], prep["n_windows"]
    n_g, n_h, T = len(G["rows"]), len(H["rows"]), int(G["trk_off"][-1])
    nb = int(_lib.LIB.load().mmd_mot_clear_ws_bytes(T))
    if nb < 0:
        raise RuntimeError(f"mmd_mot_clear_ws_bytes({T}) failed with status {nb}")
    sizes = (np.diff(G["trk_off"]).astype(np.int64) * np.diff(H["trk_off"]).astype(np.int64))
    c_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    c_total = max(int(c_off[-1]), 1)
    host = [G["rows"], G["dense"], G["off"], H["rows"], H["dense"], H["off"], G["trk_off"], H["trk_off"], c_off[:-1]]
    buf, spans = _pack(host)
    dev = torch.from_numpy(buf).to(device)                                    # the one upload

    def part(k, dtype):
        o, n = spans[k]
        return dev[o:o + n].view(dtype) if n else None

    g_rows, g_trk, g_off = part(0, torch.float32), part(1, torch.int32), part(2, torch.int32)
    h_rows, h_trk, h_off = part(3, torch.float32), part(4, torch.int32), part(5, torch.int32)
    g_toff, h_toff, c_off_d = part(6, torch.int32), part(7, torch.int32), part(8, torch.int64)
    # outputs in one buffer: counts [S, 8] int64 | iou_sum [S] float64 | idtp [S] int64 | present [T] int32 | matched [T] int32
    o_cnt, o_iou, o_id, o_pre = 0, S * 64, S * 72, S * 80
    o_mat = o_pre + (max(T, 1) * 4 + 15) // 16 * 16
    out = torch.empty(o_mat + max(T, 1) * 4, dtype=torch.uint8, device=device)
    counts, iou_sum, idtp = out[o_cnt:o_iou].view(torch.int64), out[o_iou:o_id].view(torch.float64), out[o_id:o_pre].view(torch.int64)
    present, matched = out[o_pre:o_pre + max(T, 1) * 4].view(torch.int32), out[o_mat:o_mat + max(T, 1) * 4].view(torch.int32)
    ws = torch.empty(nb, dtype=torch.uint8, device=device)
    _lib.call("mmd_mot_clear", g_rows, g_trk, g_off, n_g, h_rows, h_trk, h_off, n_h, S, W, g_toff, T, prep["iou_min"], counts, iou_sum,
              present, matched, ws)
    if prep["identity"]:
        most = max(1, int(np.diff(G["trk_off"]).max()), int(np.diff(H["trk_off"]).max()))
        C = torch.zeros(c_total, dtype=torch.int32, device=device)
        _lib.call("mmd_mot_id_counts", g_rows, g_trk, g_off, n_g, h_rows, h_trk, h_off, n_h, S, W, g_toff, h_toff, most, c_off_d, c_total,
                  prep["iou_min"], C)
        _lib.call("mmd_mot_id_assign", C, c_off_d, c_total, g_toff, h_toff, S, most, idtp)
    torch.cuda.current_stream().synchronize()
    back = out.cpu().numpy()                                                  # the one copy
    res = {"counts": back[o_cnt:o_iou].view(np.int64).reshape(S, 8).copy(), "iou_sum": back[o_iou:o_id].view(np.float64).copy(),
           "present": back[o_pre:o_pre + T * 4].view(np.int32).copy(), "matched": back[o_mat:o_mat + T * 4].view(np.int32).copy(),
           "idtp": back[o_id:o_pre].view(np.int64).copy() if prep["identity"] else None}
    if res["idtp"] is not None and (res["idtp"] < 0).any():
        raise RuntimeError("mmd_mot_id_assign refused session %d" % int(np.argmax(res["idtp"] < 0)))
    return res


def mot_metrics(gt, hyp, n_windows: int, device, iou_min: float = 0.5, identity: bool = True) -> dict:
    """gt, hyp: (rows float32 [R, 6], window int [R], track int [R][, session int [R]]), windows 0 .. n_windows-1 per session.
    -> {"overall": {...}, "sessions": [{...}, ..], "gt_tracks": int64 [n, 4] rows (session, id, present, matched)}; each dict has the keys
    n_gt n_hyp tp fp fn idsw frag mt pt ml mota motp precision recall and, with identity, idtp idfp idfn idp idr idf1.  The overall
    figures come from summed counts.  Hypothesis rows with track -1 stay in and count as false positives.

    ValueError, before the library is loaded or the device touched: a ground-truth row with track < 0; a (session, window, track >= 0)
    that occurs twice on one side; more than 256 rows of one side in one window; with identity, more than 1024 tracks of one side in one
    session; window indices outside 0 .. n_windows-1; arrays of different lengths."""
    prep = prepare(gt, hyp, n_windows, iou_min, identity)
    return assemble(prep, run_device(prep, device))


def assemble(prep: dict, res: dict) -> dict:
    """the dictionaries of `mot_metrics` from the kernels' integer counts"""
    G, S = prep["gt"], prep["n_sessions"]
    names = ("n_gt", "n_hyp", "tp", "fp", "fn", "idsw", "frag")
    sessions, toff = [], G["trk_off"]
    for s in range(S):
        c = {k: int(res["counts"][s, i]) for i, k in enumerate(names)}
        sessions.append(derive(c, float(res["iou_sum"][s]), res["present"][toff[s]:toff[s + 1]], res["matched"][toff[s]:toff[s + 1]],
                               None if res["idtp"] is None else int(res["idtp"][s])))
    total = {k: int(res["counts"][:, i].sum()) for i, k in enumerate(names)}
    overall = derive(total, float(np.sum(res["iou_sum"])), res["present"], res["matched"],
                     None if res["idtp"] is None else int(res["idtp"].sum()))
    table = np.stack([G["u_sess"], G["u_id"], res["present"].astype(np.int64), res["matched"].astype(np.int64)], axis=1).astype(np.int64)
    return {"overall": overall, "sessions": sessions, "gt_tracks": table.reshape(-1, 4)}
