"""Helper (not a test): numpy / scipy restatement of the tracking evaluation that csrc/moteval.hip computes (mm_distillnet_amd/mot.py).

The reference tree ships no tracking metrics; the rule is this project's own (tracking evaluation).  Records are
(rows [R, 6], window [R], track [R][, session [R]]); the IoU is tests/track_ref.iou_matrix (float32, the tracker's expression); a pair is
allowed when the labels are equal and iou >= float32(iou_min).  Per session, windows in order, rows in record order (a stable sort):
  keep    a ground-truth row of track g with map[g] = h >= 0 keeps h when h has a row in the window, not taken, and the pair is allowed
  assign  scipy.optimize.linear_sum_assignment(W, maximize=True) on the rows left (hypothesis rows with track >= 0), W = IoU as float64
          on allowed pairs and 0 elsewhere; the pairs that are not allowed are dropped
  count   tp, iou_sum (float64), idsw when map[g] >= 0 and != h, map[g] = h; fn / fp the unpaired rows (track -1 included);
          present / matched / frag per ground-truth track
Identity: C[g][h] = windows in which g and h form an allowed pair; IDTP = the maximum-weight matching of C.

`evaluate(..., check_unique=True)` also proves each assign step's optimum unique with a margin: every allowed pair of the optimum is
forbidden in turn (its weight set to 0, i.e. the pair dropped) and the step solved again; another matching of equal weight must lack
one of those pairs - with all of them it would be a superset, and every allowed pair weighs >= iou_min > 0 - so when every re-solve
loses more than MARGIN the optimum is the only one within MARGIN.  The kernel's float64 path then has to find the same pairs."""
import numpy as np
from scipy.optimize import linear_sum_assignment

from track_ref import iou_matrix

F = np.float32
MARGIN = 1e-6
NAN = float("nan")


def _ratio(a, b):
    return float(a) / float(b) if b else NAN


def _figures(c, iou_sum, present, matched, idtp):
    share = np.asarray(matched, np.float64) / np.maximum(np.asarray(present, np.float64), 1)
    mt, ml = int((share >= 0.8).sum()), int((share <= 0.2).sum())
    out = dict(c)
    out.update(mt=mt, pt=len(share) - mt - ml, ml=ml, mota=(1.0 - (c["fn"] + c["fp"] + c["idsw"]) / c["n_gt"]) if c["n_gt"] else NAN,
               motp=_ratio(iou_sum, c["tp"]), precision=_ratio(c["tp"], c["tp"] + c["fp"]), recall=_ratio(c["tp"], c["n_gt"]))
    if idtp is not None:
        idfp, idfn = c["n_hyp"] - idtp, c["n_gt"] - idtp
        out.update(idtp=int(idtp), idfp=idfp, idfn=idfn, idp=_ratio(idtp, idtp + idfp), idr=_ratio(idtp, idtp + idfn),
                   idf1=_ratio(2 * idtp, 2 * idtp + idfp + idfn))
    return out


def _record(rec):
    rows = np.asarray(rec[0], np.float32).reshape(-1, 6)
    window, track = np.asarray(rec[1], np.int64).reshape(-1), np.asarray(rec[2], np.int64).reshape(-1)
    session = np.zeros(len(rows), np.int64) if len(rec) == 3 else np.asarray(rec[3], np.int64).reshape(-1)
    return rows, window, track, session


def evaluate(gt, hyp, n_windows, iou_min=0.5, identity=True, check_unique=False):
    """-> the dictionary of mot.mot_metrics plus "iou_sums" (float64 per session), "pairs" (tp per session, for the tolerance),
    "unique" (True / False; None without check_unique) and "margin" (the smallest loss of a re-solve, inf when there was none)"""
    g_rows, g_win, g_trk, g_ses = _record(gt)
    h_rows, h_win, h_trk, h_ses = _record(hyp)
    S = 1 + max([int(s.max()) for s in (g_ses, h_ses) if len(s)] + [0])
    thr = F(iou_min)
    sessions, tables, iou_sums, margin = [], [], [], np.inf
    totals = {k: 0 for k in ("n_gt", "n_hyp", "tp", "fp", "fn", "idsw", "frag")}
    all_present, all_matched, id_total = [], [], 0
    for s in range(S):
        gs, hs = np.nonzero(g_ses == s)[0], np.nonzero(h_ses == s)[0]
        g_ids = sorted(set(g_trk[gs].tolist()))
        h_ids = sorted(set(t for t in h_trk[hs].tolist() if t >= 0))
        gi, hi = {t: k for k, t in enumerate(g_ids)}, {t: k for k, t in enumerate(h_ids)}
        mp = {t: -1 for t in g_ids}
        present, matched = np.zeros(len(g_ids), np.int64), np.zeros(len(g_ids), np.int64)
        ever, last = {t: False for t in g_ids}, {t: False for t in g_ids}
        C = np.zeros((len(g_ids), len(h_ids)), np.int64)
        c = {k: 0 for k in totals}
        iou_sum = 0.0
        gs, hs = gs[np.argsort(g_win[gs], kind="stable")], hs[np.argsort(h_win[hs], kind="stable")]      # record order inside a window
        g_at, h_at = np.searchsorted(g_win[gs], np.arange(n_windows + 1)), np.searchsorted(h_win[hs], np.arange(n_windows + 1))
        for w in range(n_windows):
            ga, ha = gs[g_at[w]:g_at[w + 1]], hs[h_at[w]:h_at[w + 1]]
            ng, nh = len(ga), len(ha)
            c["n_gt"] += ng
            c["n_hyp"] += nh
            gt_t, hy_t = g_trk[ga], h_trk[ha]
            pair = np.full(ng, -1, np.int64)
            taken = np.zeros(nh, bool)
            if ng and nh:
                iou = iou_matrix(g_rows[ga, :4], h_rows[ha, :4])
                with np.errstate(invalid="ignore"):
                    allowed = (g_rows[ga, 5][:, None] == h_rows[ha, 5][None, :]) & (iou >= thr)
                for a, b in zip(*np.nonzero(allowed & (hy_t >= 0)[None, :])):
                    C[gi[int(gt_t[a])], hi[int(hy_t[b])]] += 1
                for a in range(ng):                                   # keep
                    h = mp[int(gt_t[a])]
                    if h < 0:
                        continue
                    where = np.nonzero(hy_t == h)[0]
                    if len(where) and not taken[where[0]] and allowed[a, where[0]]:
                        pair[a] = where[0]
                        taken[where[0]] = True
                L, M = np.nonzero(pair < 0)[0], np.nonzero(~taken & (hy_t >= 0))[0]
                if len(L) and len(M):                                 # assign
                    Wm = np.where(allowed, iou, F(0)).astype(np.float64)[np.ix_(L, M)]
                    ok = allowed[np.ix_(L, M)]
                    r, cc = linear_sum_assignment(Wm, maximize=True)
                    best = Wm[r, cc].sum()
                    for a, b in zip(r, cc):
                        if not ok[a, b]:
                            continue
                        pair[L[a]] = M[b]
                        taken[M[b]] = True
                        if check_unique:
                            W2 = Wm.copy()
                            W2[a, b] = 0.0
                            r2, c2 = linear_sum_assignment(W2, maximize=True)
                            margin = min(margin, best - W2[r2, c2].sum())
                for a in range(ng):                                   # count
                    if pair[a] >= 0:
                        g, h = int(gt_t[a]), int(hy_t[pair[a]])
                        c["tp"] += 1
                        iou_sum += float(iou[a, pair[a]])
                        if mp[g] >= 0 and mp[g] != h:
                            c["idsw"] += 1
                        mp[g] = h
            c["fn"] += int((pair < 0).sum())
            c["fp"] += int((~taken).sum())
            for a in range(ng):
                g, p = int(gt_t[a]), bool(pair[a] >= 0)
                present[gi[g]] += 1
                if p:
                    matched[gi[g]] += 1
                    if ever[g] and not last[g]:
                        c["frag"] += 1
                last[g] = p
                ever[g] = ever[g] or p
        idtp = None
        if identity:
            idtp = 0
            if C.size:
                r, cc = linear_sum_assignment(C.astype(np.float64), maximize=True)
                idtp = int(C[r, cc].sum())
            id_total += idtp
        sessions.append(_figures(c, iou_sum, present, matched, idtp))
        iou_sums.append(iou_sum)
        for k in totals:
            totals[k] += c[k]
        all_present.append(present)
        all_matched.append(matched)
        tables.append(np.stack([np.full(len(g_ids), s, np.int64), np.asarray(g_ids, np.int64).reshape(-1), present, matched], axis=1).reshape(-1, 4))
    present, matched = np.concatenate(all_present), np.concatenate(all_matched)
    return {"overall": _figures(totals, float(np.sum(iou_sums)), present, matched, id_total if identity else None), "sessions": sessions,
            "gt_tracks": np.concatenate(tables).astype(np.int64).reshape(-1, 4), "iou_sums": np.asarray(iou_sums, np.float64),
            "pairs": [x["tp"] for x in sessions], "unique": (bool(margin > MARGIN) if check_unique else None), "margin": float(margin)}


def id_matrix_idtp(C):
    """IDTP of one integer matrix C [G, H]: the weight of its maximum-weight matching"""
    C = np.asarray(C, np.int64)
    if not C.size:
        return 0
    r, c = linear_sum_assignment(C.astype(np.float64), maximize=True)
    return int(C[r, c].sum())
