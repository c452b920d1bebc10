"""Host restatements of the weighted box fusion the device runs (csrc/postproc.hip pp_wbf_kernel; the rule: include/mmdistill.h,
mmd_wbf_merge_n), and the seeded scenes the tests fuse.

  wbf_f32   numpy float32, the rule operation for operation (every product, sum, difference and quotient rounded on its own, fmaxf /
            fminf as np.fmax / np.fmin): the kernel must match it bit for bit
  wbf_f64   the same rule in plain float64, with the smallest distance of any decision from its boundary, so that a generator can keep
            only scenes whose clustering does not hang on the last bits

Sources are given as the NMS reference takes them: srcs[s][b] = array [n, 6] (x1, y1, x2, y2, score, label) of source s, image b.
"""
from types import SimpleNamespace

import numpy as np

F = np.float32
FLT_MIN = F(1.17549435e-38)
MAX_ROWS = 1024


def gather(srcs, b, B, merge01):
    """-> (rows [n, 6] float32 in gather order, source index [n], cut): the sources' rows of image b in source order; with merge01 (and
    B >= 2) image 1 takes image 0's rows in front of its own when it has rows itself.  More than 1024 rows are cut to the first 1024."""
    def image(i):
        rows = [np.asarray(s[i], dtype=F).reshape(-1, 6) for s in srcs]
        return rows, [np.full(len(r), k, dtype=np.int64) for k, r in enumerate(rows)]
    rows, src = image(b)
    if merge01 and B >= 2 and b == 1 and sum(len(r) for r in rows) > 0:
        r0, s0 = image(0)
        rows, src = r0 + rows, s0 + src
    rows, src = np.concatenate(rows, 0), np.concatenate(src, 0)
    return rows[:MAX_ROWS], src[:MAX_ROWS], len(rows) > MAX_ROWS


def _order(rows):
    return sorted(range(len(rows)), key=lambda i: (-float(rows[i, 4]), i))


def _iou32(r, ra, c, ca):
    xx1, yy1 = np.fmax(r[0], c[0]), np.fmax(r[1], c[1])
    xx2, yy2 = np.fmin(r[2], c[2]), np.fmin(r[3], c[3])
    ww, hh = np.fmax(F(0), xx2 - xx1), np.fmax(F(0), yy2 - yy1)
    inter = ww * hh
    return inter / ((ra + ca) - inter)


def _fuse32(rows, src, thr, inclusive):
    thr = F(thr)
    cl = []
    for i in _order(rows):
        r, lb = rows[i, :4], rows[i, 5]
        ra = (r[2] - r[0]) * (r[3] - r[1])
        best, bc = None, -1
        for c, k in enumerate(cl):
            if k.label != lb:
                continue
            ovr = _iou32(r, ra, k.box, k.area)
            if (ovr >= thr if inclusive else ovr > thr) and (bc < 0 or ovr > best):
                best, bc = ovr, c
        if bc < 0:
            cl.append(SimpleNamespace(label=lb, W=F(0), S=np.zeros(4, F), n=0, bits=0, members=[], box=None, area=None))
        k = cl[bc]
        w = np.fmax(rows[i, 4], FLT_MIN)
        k.W = k.W + w
        k.S = np.array([k.S[j] + w * r[j] for j in range(4)], dtype=F)
        k.n += 1
        k.bits |= 1 << int(src[i])
        k.members.append(i)
        k.box = np.array([k.S[j] / k.W for j in range(4)], dtype=F)
        k.area = (k.box[2] - k.box[0]) * (k.box[3] - k.box[1])
    return cl


def _iou64(r, ra, c, ca):
    ww, hh = max(0.0, min(r[2], c[2]) - max(r[0], c[0])), max(0.0, min(r[3], c[3]) - max(r[1], c[1]))
    inter = ww * hh
    den = ra + ca - inter
    return inter / den if den != 0 else float("nan")


def _fuse64(rows, src, thr, inclusive):
    """-> (clusters, margin): margin = the smallest of |IoU - thr| over every comparison made and of the lead of a winning cluster over the
    runner-up"""
    thr = float(F(thr))
    rows = rows.astype(np.float64)
    cl, margin = [], float("inf")
    for i in _order(rows):
        r, lb = [float(v) for v in rows[i, :4]], rows[i, 5]
        ra = (r[2] - r[0]) * (r[3] - r[1])
        cands = []
        for c, k in enumerate(cl):
            if k.label != lb:
                continue
            ovr = _iou64(r, ra, k.box, k.area)
            margin = min(margin, abs(ovr - thr))
            if ovr >= thr if inclusive else ovr > thr:
                cands.append((-ovr, c))
        cands.sort()
        if len(cands) > 1:
            margin = min(margin, cands[1][0] - cands[0][0])
        if not cands:
            cl.append(SimpleNamespace(label=lb, W=0.0, S=[0.0] * 4, n=0, bits=0, members=[], box=None, area=None))
        k = cl[cands[0][1] if cands else -1]
        w = max(float(rows[i, 4]), float(FLT_MIN))
        k.W += w
        k.S = [k.S[j] + w * r[j] for j in range(4)]
        k.n += 1
        k.bits |= 1 << int(src[i])
        k.members.append(i)
        k.box = [k.S[j] / k.W for j in range(4)]
        k.area = (k.box[2] - k.box[0]) * (k.box[3] - k.box[1])
    return cl, margin


def _run(fuse, dtype, srcs, B, thr, inclusive, merge01, min_votes, max_boxes):
    out = SimpleNamespace(boxes=[], aux=[], members=[], overflow=False, margin=float("inf"))
    with np.errstate(all="ignore"):
        for b in range(B):
            rows, src, cut = gather(srcs, b, B, merge01)
            got = fuse(rows, src, thr, inclusive)
            if isinstance(got, tuple):
                got, m = got
                out.margin = min(out.margin, m)
            keep = [k for k in got if bin(k.bits).count("1") >= min_votes]
            if max_boxes is not None and len(keep) > max_boxes:
                keep, cut = keep[:max_boxes], True
            out.overflow |= cut
            out.boxes.append(np.array([list(k.box) + [k.label] for k in keep], dtype=dtype).reshape(-1, 5))
            out.aux.append(np.array([[k.W / dtype(k.n), k.n, bin(k.bits).count("1")] for k in keep], dtype=dtype).reshape(-1, 3))
            out.members.append([list(k.members) for k in keep])
    return out


def wbf_f32(srcs, B, thr=0.5, inclusive=False, merge01=False, min_votes=1, max_boxes=None):
    """-> namespace: boxes[b] [k, 5] float32 (fused x1, y1, x2, y2, label), aux[b] [k, 3] float32 (W / n, n, distinct sources), members[b]
    (per emitted cluster the gather indices of its rows, in arrival order), overflow (more than 1024 rows or than max_boxes clusters)"""
    return _run(_fuse32, F, srcs, B, thr, inclusive, merge01, min_votes, max_boxes)


def wbf_f64(srcs, B, thr=0.5, inclusive=False, merge01=False, min_votes=1, max_boxes=None):
    """As wbf_f32 in float64, plus `margin`: how far the closest decision of the run lay from its boundary."""
    return _run(_fuse64, np.float64, srcs, B, thr, inclusive, merge01, min_votes, max_boxes)


def coordinate_bound(m, S):
    """|fp32 fused coordinate - float64's| for a cluster of m members at image size S: m rounded products and m - 1 rounded additions of
    positive terms in the numerator, m - 1 additions in the denominator, one division - each at most 2^-24 relative, on values <= S"""
    return (2 * m + 6) * 2.0 ** -24 * S


def draw_scene(rng, B, nsrc, S=512.0, max_objects=12, labels=(0.0, 1.0)):
    """One random scene: per image a few objects, each seen by every source with probability 0.8 as a jittered copy with its own score;
    plus a few boxes only one source reports.  -> srcs[s][b] [n, 6] float32"""
    srcs = [[None] * B for _ in range(nsrc)]
    for b in range(B):
        rows = [[] for _ in range(nsrc)]
        for _ in range(int(rng.integers(0, max_objects + 1))):
            w, h = rng.uniform(0.05, 0.4, 2) * S
            x1, y1 = rng.uniform(0, S - w), rng.uniform(0, S - h)
            lb = labels[int(rng.integers(0, len(labels)))]
            for s in range(nsrc):
                if rng.random() < 0.8:
                    j = rng.normal(0, 0.04, 4) * np.array([w, h, w, h])
                    box = np.clip(np.array([x1, y1, x1 + w, y1 + h]) + j, 0, S)
                    rows[s].append(list(box) + [rng.uniform(0.3, 1.0), lb])
        for s in range(nsrc):
            for _ in range(int(rng.integers(0, 3))):
                w, h = rng.uniform(0.05, 0.3, 2) * S
                x1, y1 = rng.uniform(0, S - w), rng.uniform(0, S - h)
                rows[s].append([x1, y1, x1 + w, y1 + h, rng.uniform(0.3, 1.0), labels[int(rng.integers(0, len(labels)))]])
            order = rng.permutation(len(rows[s]))
            srcs[s][b] = np.array([rows[s][i] for i in order], dtype=F).reshape(-1, 6)
    return srcs


def clear_scene(seed, B, nsrc, thr, inclusive=False, merge01=False, S=512.0, min_margin=1e-3):
    """The first scene of the seed's stream in which every decision of the float64 run - each IoU against the threshold, each winner
    against its runner-up - lies more than min_margin from its boundary: decided here, by redrawing, by the reference alone.
    -> (srcs, the float64 result)"""
    rng = np.random.default_rng(seed)
    for _ in range(1000):
        srcs = draw_scene(rng, B, nsrc, S)
        ref = wbf_f64(srcs, B, thr, inclusive, merge01)
        if ref.margin > min_margin:
            return srcs, ref
    raise RuntimeError("no scene clear of the threshold in 1000 draws")
