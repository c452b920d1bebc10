"""Helper (not a test): numpy / scipy restatement of HOTA (Luiten et al., IJCV 2021) as csrc/moteval.hip computes it (mm_distillnet_amd.mot:
hota_metrics; the rule: DESIGN.md, tracking evaluation, HOTA).  It follows the published algorithm and TrackEval's conventions, with
every accumulated quantity an integer so that nothing depends on an order of summation.

Per session, track ids dense in rising order, hypothesis rows with track -1 left out of both passes (they stay in n_hyp):
  s(i, j)   tests/track_ref.iou_matrix (float32) where the labels are equal, else 0
  q(x)      floor(float64(x) * 2^32 + 0.5) as an integer;  alpha_k = float32((k + 1) / 20), k = 0 .. 18;  bins(s) = #{k: s >= alpha_k}
  pass 1    per window R_i = sum_j q(s), C_j = sum_i q(s); every pair with q(s) > 0: P[g][h] += q(float64(q(s)) / float64(R_i + C_j - q(s)))
  pass 2    per window score = gas[g][h] * float64(s), gas = float64(P) / (2^32 * float64(gc + tc) - float64(P)), gc / tc the rows per
            track; scipy.optimize.linear_sum_assignment(score, maximize=True); every assigned pair with b = bins(s) > 0:
            hist[g][h][b - 1] += 1, and for k < b: tp[k] += 1, loc[k] += q(s)
  pass 3    per cell mc[k] = hist[g][h][k:].sum(); per k the sums over the cells with mc > 0 of mc * mc / (gc + tc - mc), mc * mc / gc,
            mc * mc / tc in float64
  figures   per k: FN = n_gt - TP, FP = n_hyp - TP, DetA = TP / (TP + FN + FP), DetRe = TP / (TP + FN), DetPr = TP / (TP + FP) (NaN for a
            zero denominator), AssA / AssRe / AssPr = numerator / max(1, TP), LocA = loc / 2^32 / TP (1 where TP = 0),
            HOTA = sqrt(DetA * AssA); reported: the means over the 19 thresholds; overall: from the summed TP, n_gt, n_hyp, loc, numerators.

`evaluate(..., check_unique=True)` also proves each window's matching unique with a margin, as mot_ref does for CLEAR: every pair of
the optimum with a positive score is forbidden in turn (its score set to 0) and the window solved again.  Another assignment of equal
score must lack one of those pairs - with all of them it could only add pairs of score 0, which have q(s) = 0 or s = 0, hence bins = 0,
and are not counted.  So when every re-solve loses more than the margin, the counted pairs are the only ones within the margin.  The
margin is RELATIVE to the window's largest score: loss > MARGIN * max(score).  MARGIN = 1e-9: the kernel's shortest-augmenting-path
routine sums at most 2 * 256 float64 costs and potentials of magnitude <= max(score) per path and 256 paths, an error below
256 * 512 * 2^-53 = 1.5e-11 of that scale; 1e-9 leaves two orders of magnitude.  "margin" reports the smallest relative loss seen."""
import numpy as np
from scipy.optimize import linear_sum_assignment

from track_ref import iou_matrix

F = np.float32
NA = 19
TWO32 = 4294967296.0
MARGIN = 1e-9
NAN = float("nan")
KEYS = ("hota", "deta", "assa", "detre", "detpr", "assre", "asspr", "loca")
ALPHA32 = np.array([F((k + 1) / 20) for k in range(NA)], F)


def q(x):
    """float array in [0, 1] (or a little above) -> int64 array"""
    return np.floor(np.asarray(x, np.float64) * TWO32 + 0.5).astype(np.int64)


def bins(s):
    return int((F(s) >= ALPHA32).sum())


def _ratio(a, b):
    return float(a) / float(b) if b else NAN


def figures(n_gt, n_hyp, tp, loc, num):
    """-> ({key: mean over the thresholds}, {"tp": int64 [19], key: float64 [19]})"""
    per = {k: np.zeros(NA, np.float64) for k in KEYS}
    for k in range(NA):
        t = int(tp[k])
        fn, fp = n_gt - t, n_hyp - t
        per["deta"][k], per["detre"][k], per["detpr"][k] = _ratio(t, t + fn + fp), _ratio(t, t + fn), _ratio(t, t + fp)
        per["assa"][k], per["assre"][k], per["asspr"][k] = (float(num[k][c]) / max(1, t) for c in range(3))
        per["loca"][k] = float(int(loc[k])) / TWO32 / t if t else 1.0
        per["hota"][k] = float(np.sqrt(per["deta"][k] * per["assa"][k]))
    means = {k: float(np.mean(per[k])) for k in KEYS}
    per["tp"] = np.asarray([int(v) for v in tp], np.int64)
    return means, per


def _record(rec):
    rows = np.asarray(rec[0], np.float32).reshape(-1, 6)
    window, track = np.asarray(rec[1], np.int64).reshape(-1), np.asarray(rec[2], np.int64).reshape(-1)
    session = np.zeros(len(rows), np.int64) if len(rec) == 3 else np.asarray(rec[3], np.int64).reshape(-1)
    return rows, window, track, session


def evaluate(gt, hyp, n_windows, check_unique=False):
    """-> the dictionary of mot.hota_metrics ("overall", "sessions", "alphas") plus, per session in lists: "P" int64 [G, H], "hist" int64
    [G, H, 19], "tp" int64 [19], "loc" Python ints [19], "num" float64 [19, 3], "cells" (G * H, for the tolerance), "n_gt", "n_hyp"; and
    "unique" (True / False; None without check_unique), "margin" (the smallest relative loss of a re-solve, inf when there was none)"""
    g_rows, g_win, g_trk, g_ses = _record(gt)
    h_rows, h_win, h_trk, h_ses = _record(hyp)
    S = 1 + max([int(s.max()) for s in (g_ses, h_ses) if len(s)] + [0])
    out = {k: [] for k in ("P", "hist", "tp", "loc", "num", "cells", "n_gt", "n_hyp")}
    margin = np.inf
    for s in range(S):
        gs, hs_all = np.nonzero(g_ses == s)[0], np.nonzero(h_ses == s)[0]
        hs = hs_all[h_trk[hs_all] >= 0]
        g_ids, h_ids = np.unique(g_trk[gs]), np.unique(h_trk[hs])
        G, H = len(g_ids), len(h_ids)
        gs, hs = gs[np.argsort(g_win[gs], kind="stable")], hs[np.argsort(h_win[hs], kind="stable")]      # record order inside a window
        g_at, h_at = np.searchsorted(g_win[gs], np.arange(n_windows + 1)), np.searchsorted(h_win[hs], np.arange(n_windows + 1))
        g_dense, h_dense = np.searchsorted(g_ids, g_trk[gs]), np.searchsorted(h_ids, h_trk[hs])
        gc, tc = np.bincount(g_dense, minlength=G).astype(np.int64), np.bincount(h_dense, minlength=H).astype(np.int64)
        P = np.zeros((G, H), np.int64)
        wins = []
        for w in range(n_windows):                                    # pass 1
            ga, ha = slice(g_at[w], g_at[w + 1]), slice(h_at[w], h_at[w + 1])
            if ga.stop == ga.start or ha.stop == ha.start:
                continue
            gr, hr = g_rows[gs[ga]], h_rows[hs[ha]]
            sim = np.where(gr[:, 5][:, None] == hr[:, 5][None, :], iou_matrix(gr[:, :4], hr[:, :4]), F(0))
            Q = np.where(sim > 0, q(sim), 0)
            R, C = Q.sum(axis=1), Q.sum(axis=0)
            a, b = np.nonzero(Q > 0)
            if len(a):
                c = Q[a, b].astype(np.float64) / (R[a] + C[b] - Q[a, b]).astype(np.float64)
                np.add.at(P, (g_dense[ga][a], h_dense[ha][b]), q(c))
            wins.append((g_dense[ga], h_dense[ha], sim, Q))
        with np.errstate(invalid="ignore", divide="ignore"):
            gas = P.astype(np.float64) / (TWO32 * (gc[:, None] + tc[None, :]).astype(np.float64) - P.astype(np.float64))
        hist = np.zeros((G, H, NA), np.int64)
        tp, loc = np.zeros(NA, np.int64), [0] * NA
        for gd, hd, sim, Q in wins:                                   # pass 2
            score = gas[np.ix_(gd, hd)] * sim.astype(np.float64)
            if not (score > 0).any():
                continue
            r, cc = linear_sum_assignment(score, maximize=True)
            best, scale = score[r, cc].sum(), score.max()
            for a, b in zip(r, cc):
                if check_unique and score[a, b] > 0:
                    s2 = score.copy()
                    s2[a, b] = 0.0
                    r2, c2 = linear_sum_assignment(s2, maximize=True)
                    margin = min(margin, (best - s2[r2, c2].sum()) / scale)
                n = bins(sim[a, b])
                if n > 0:
                    hist[gd[a], hd[b], n - 1] += 1
                    tp[:n] += 1
                    for k in range(n):
                        loc[k] += int(Q[a, b])
        num = np.zeros((NA, 3), np.float64)                           # pass 3
        for g, h in zip(*np.nonzero(hist.sum(axis=2))):
            mc = np.cumsum(hist[g, h, ::-1])[::-1]
            for k in range(NA):
                m = int(mc[k])
                if m > 0:
                    m2 = float(m) * float(m)
                    num[k, 0] += m2 / float(int(gc[g]) + int(tc[h]) - m)
                    num[k, 1] += m2 / float(int(gc[g]))
                    num[k, 2] += m2 / float(int(tc[h]))
        for k, v in (("P", P), ("hist", hist), ("tp", tp), ("loc", loc), ("num", num), ("cells", G * H), ("n_gt", len(gs)), ("n_hyp", len(hs_all))):
            out[k].append(v)
    got = [figures(out["n_gt"][s], out["n_hyp"][s], out["tp"][s], out["loc"][s], out["num"][s]) for s in range(S)]
    loc = [sum(out["loc"][s][k] for s in range(S)) for k in range(NA)]
    overall, per = figures(sum(out["n_gt"]), sum(out["n_hyp"]), np.sum(out["tp"], axis=0), loc, np.sum(out["num"], axis=0))
    out.update(overall=overall, sessions=[m for m, _ in got],
               alphas={"alpha": ALPHA32.astype(np.float64), "overall": per, "sessions": [p for _, p in got]},
               unique=(bool(margin > MARGIN) if check_unique else None), margin=float(margin))
    return out
