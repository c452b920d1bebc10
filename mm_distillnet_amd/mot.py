"""Tracking evaluation: the CLEAR-MOT counts (MOTA, MOTP, FP, FN, identity switches, fragmentations, MT / PT / ML) and the identity
measures (IDTP / IDFP / IDFN, IDP, IDR, IDF1) of a tracked record against a ground-truth record, on the device (csrc/moteval.hip:
`mmd_mot_clear`, `mmd_mot_id_counts`, `mmd_mot_id_assign`).

The rule is written out in DESIGN.md (tracking evaluation) and in include/mmdistill.h; tests/mot_ref.py restates it with numpy and
scipy.  A record is what `AudioDetector.track_stream`, `tracker.track_rows` or a `LiveBank` return: rows float32 [R, 6] (x1, y1, x2, y2,
score, label), window int [R], track int [R][, session int [R]].  The ground truth may be a record of tracks made from a teacher's boxes
with `tracker.track_rows`.  Validation, the stable sort by (session, window), the dense track ids and the offset tables are host work
(`prepare`); the device gets one upload, the kernels run on the current stream, and the host waits and copies once.

HOTA (Luiten et al., IJCV 2021) with DetA / AssA / LocA and the recall / precision pairs is `hota_metrics` (`mmd_hota_align`,
`mmd_hota_match`, `mmd_hota_assoc`), split the same way: `hota_prepare` / `hota_run_device` / `hota_assemble`; tests/hota_ref.py restates
it."""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np

ROWS_MAX = 256              # rows of one side in one window (the tracker's DET_MAX)
ID_TRACKS_MAX = 1024        # tracks per side and session of the identity measures
CLEAR_KEYS = ("n_gt", "n_hyp", "tp", "fp", "fn", "idsw", "frag", "mt", "pt", "ml", "mota", "motp", "precision", "recall")
ID_KEYS = ("idtp", "idfp", "idfn", "idp", "idr", "idf1")
KEYS = CLEAR_KEYS + ID_KEYS
HOTA_KEYS = ("hota", "deta", "assa", "detre", "detpr", "assre", "asspr", "loca")
HOTA_ALPHAS = 19            # thresholds alpha_k = float32((k + 1) / 20)
HOTA_WINDOWS_MAX = 2 ** 20  # the alignment sums stay below 2^52: exact in float64
HOTA_HIST_MAX = 2 ** 28     # histogram words: 19 per cell of the identity matrix's layout


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


# ---------------------------------------------------------------------------------------------------------------------------- HOTA
def hota_alphas() -> np.ndarray:
    """the 19 thresholds as the kernels compare them: float32((k + 1) / 20), returned as float64"""
    return np.array([np.float32((k + 1) / 20) for k in range(HOTA_ALPHAS)], np.float64)


def hota_derive(n_gt: int, n_hyp: int, tp, loc, num) -> Tuple[dict, dict]:
    """The figures of one session, or of all sessions from summed counts: tp int [19], loc int [19] (sums of q(s) = s * 2^32), num float64
    [19, 3] (the AssA / AssRe / AssPr numerators).  -> ({key: mean over the thresholds}, {"tp": int64 [19], key: float64 [19]})"""
    per = {k: np.zeros(HOTA_ALPHAS, np.float64) for k in HOTA_KEYS}
    for k in range(HOTA_ALPHAS):
        t = int(tp[k])
        fn, fp = int(n_gt) - t, int(n_hyp) - t
        per["deta"][k], per["detre"][k], per["detpr"][k] = _ratio(t, t + fn + fp), _ratio(t, t + fn), _ratio(t, t + fp)
        per["assa"][k], per["assre"][k], per["asspr"][k] = (float(num[k][q]) / max(1, t) for q in range(3))
        per["loca"][k] = float(int(loc[k])) / 4294967296.0 / t if t else 1.0
        per["hota"][k] = float(np.sqrt(per["deta"][k] * per["assa"][k]))
    means = {k: float(np.mean(per[k])) for k in HOTA_KEYS}
    per["tp"] = np.asarray([int(v) for v in tp], np.int64)
    return means, per


def hota_prepare(gt, hyp, n_windows: int) -> dict:
    """The host side of `hota_metrics`: `prepare`'s checks and tables (HOTA has no iou_min and always needs the per-session track
    tables), HOTA's own two limits, the rows per track and the rows per session.  Touches neither the library nor the device."""
    if int(n_windows) > HOTA_WINDOWS_MAX:
        raise ValueError("hota_metrics: n_windows = %d: at most 2^20 = %d windows per session (the alignment sums must stay exact in "
                         "float64)" % (int(n_windows), HOTA_WINDOWS_MAX))
    prep = prepare(gt, hyp, n_windows, 0.5, True)
    G, H, S, W = prep["gt"], prep["hyp"], prep["n_sessions"], prep["n_windows"]
    sizes = np.diff(G["trk_off"]).astype(np.int64) * np.diff(H["trk_off"]).astype(np.int64)
    c_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    if HOTA_ALPHAS * int(c_off[-1]) > HOTA_HIST_MAX:
        raise ValueError("hota_metrics: %d track pairs over all sessions need %d histogram cells: at most 2^28 = %d (19 per pair of a "
                         "ground-truth and a hypothesis track of one session)" % (int(c_off[-1]), HOTA_ALPHAS * int(c_off[-1]), HOTA_HIST_MAX))
    has = H["dense"] >= 0
    prep.update(c_off=c_off, c_total=max(int(c_off[-1]), 1),
                gc=np.bincount(G["trk_off"][G["session"]].astype(np.int64) + G["dense"], minlength=max(int(G["trk_off"][-1]), 1)).astype(np.int32),
                tc=np.bincount(H["trk_off"][H["session"][has]].astype(np.int64) + H["dense"][has],
                               minlength=max(int(H["trk_off"][-1]), 1)).astype(np.int32),
                n_gt=(G["off"][W::W] - G["off"][:-1:W]).astype(np.int64), n_hyp=(H["off"][W::W] - H["off"][:-1:W]).astype(np.int64))
    return prep


def hota_run_device(prep: dict, device, intermediates: bool = False, times: Optional[dict] = None) -> dict:
    """The kernels on what `hota_prepare` made: one upload, three launches on the current stream, one synchronise, one copy back.
    -> {"tp" int64 [S, 19], "loc" uint64 [S, 19], "num" float64 [S, 19, 3]}; intermediates: also "P" uint64 [c_total] and "hist" int32
    [c_total, 19] (two more copies: for tests).  times: a dict that receives the seconds of "upload", "align", "match", "assoc" and
    "copy", with a synchronise behind each (tools/dev/time_hota.py; the call is slower for it)"""
    import time

    import torch

    from . import _lib
    G, H, S, W, A = prep["gt"], prep["hyp"], prep["n_sessions"], prep["n_windows"], HOTA_ALPHAS
    n_g, n_h, T_g, T_h, c_total = len(G["rows"]), len(H["rows"]), int(G["trk_off"][-1]), int(H["trk_off"][-1]), prep["c_total"]
    host = [G["rows"], G["dense"], G["off"], H["rows"], H["dense"], H["off"], G["trk_off"], H["trk_off"], prep["c_off"][:-1], prep["gc"], prep["tc"]]
    buf, spans = _pack(host)
    clock = [time.perf_counter()]

    def lap(name):
        if times is not None:
            torch.cuda.current_stream().synchronize()
            clock.append(time.perf_counter())
            times[name] = clock[-1] - clock[-2]
    dev = torch.from_numpy(buf).to(device)                                    # the one upload

    def part(k, dtype):
        o, n = spans[k]
        return dev[o:o + n].view(dtype) if n else None

    g_rows, g_trk, g_off = part(0, torch.float32), part(1, torch.int32), part(2, torch.int32)
    h_rows, h_trk, h_off = part(3, torch.float32), part(4, torch.int32), part(5, torch.int32)
    g_toff, h_toff, c_off_d, gc, tc = part(6, torch.int32), part(7, torch.int32), part(8, torch.int64), part(9, torch.int32), part(10, torch.int32)
    most = max(1, int(np.diff(G["trk_off"]).max()), int(np.diff(H["trk_off"]).max()))
    # outputs in one buffer: tp [S, 19] int64 | loc [S, 19] uint64 (both zeroed) | num [S, 19, 3] float64 (needs no zeroing)
    o_loc, o_num, o_end = S * A * 8, S * A * 16, S * A * 40
    out = torch.zeros(o_end, dtype=torch.uint8, device=device)
    tp, loc, num = out[:o_loc].view(torch.int64), out[o_loc:o_num].view(torch.int64), out[o_num:].view(torch.float64)
    P = torch.zeros(c_total, dtype=torch.int64, device=device)               # unsigned on the device; the values stay below 2^52
    hist = torch.zeros(c_total * A, dtype=torch.int32, device=device)
    lap("upload")                                                             # .. and the zero fills
    _lib.call("mmd_hota_align", g_rows, g_trk, g_off, n_g, h_rows, h_trk, h_off, n_h, S, W, g_toff, h_toff, most, c_off_d, c_total, P)
    lap("align")
    _lib.call("mmd_hota_match", g_rows, g_trk, g_off, n_g, h_rows, h_trk, h_off, n_h, S, W, g_toff, h_toff, most, c_off_d, c_total, P,
              gc, T_g, tc, T_h, hist, tp, loc)
    lap("match")
    _lib.call("mmd_hota_assoc", hist, c_off_d, c_total, g_toff, h_toff, gc, T_g, tc, T_h, S, most, num)
    lap("assoc")
    torch.cuda.current_stream().synchronize()
    back = out.cpu().numpy()                                                  # the one copy
    lap("copy")
    res = {"tp": back[:o_loc].view(np.int64).reshape(S, A).copy(), "loc": back[o_loc:o_num].view(np.uint64).reshape(S, A).copy(),
           "num": back[o_num:].view(np.float64).reshape(S, A, 3).copy()}
    if intermediates:
        res["P"] = P.cpu().numpy().view(np.uint64)
        res["hist"] = hist.cpu().numpy().reshape(c_total, A)
    return res


def hota_assemble(prep: dict, res: dict) -> dict:
    """the dictionaries of `hota_metrics` from the kernels' sums; the overall figures come from the summed tp, n_gt, n_hyp, loc and
    numerators (TrackEval's combination over sequences)"""
    S = prep["n_sessions"]
    got = [hota_derive(int(prep["n_gt"][s]), int(prep["n_hyp"][s]), res["tp"][s], [int(v) for v in res["loc"][s]], res["num"][s]) for s in range(S)]
    loc = [sum(int(res["loc"][s][k]) for s in range(S)) for k in range(HOTA_ALPHAS)]
    overall, per = hota_derive(int(prep["n_gt"].sum()), int(prep["n_hyp"].sum()), res["tp"].sum(axis=0), loc, res["num"].sum(axis=0))
    return {"overall": overall, "sessions": [m for m, _ in got],
            "alphas": {"alpha": hota_alphas(), "overall": per, "sessions": [p for _, p in got]}}


def hota_metrics(gt, hyp, n_windows: int, device) -> dict:
    """HOTA of the records `mot_metrics` takes.  -> {"overall": {...}, "sessions": [{...}, ..], "alphas": {"alpha": float64 [19],
    "overall": {...}, "sessions": [{...}, ..]}}: the dicts have the keys hota deta assa detre detpr assre asspr loca, the means over the
    19 thresholds 0.05 .. 0.95; the dicts under "alphas" hold the same keys as float64 [19] and "tp" int64 [19].  There is no iou_min:
    the thresholds are HOTA's own.  Overall figures come from summed counts and numerators.  A ratio with a zero denominator is NaN; LocA
    is 1 at a threshold without a true positive.

    ValueError, before the library is loaded or the device touched: everything `mot_metrics` refuses (the 256 rows per window and the
    1024 tracks per side and session included), n_windows > 2^20, more than 2^28 histogram cells (19 per track pair of a session)."""
    prep = hota_prepare(gt, hyp, n_windows)
    return hota_assemble(prep, hota_run_device(prep, device))
