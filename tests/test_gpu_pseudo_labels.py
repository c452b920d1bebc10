"""GPU parity of the pseudo-label kernels (csrc/postproc.hip) and of the focal loss on what they produce (csrc/loss.hip)
against the CPU oracle (oracle/postproc_ref.py, oracle/losses_ref.py), at the classes, ties, capacities and buffer states the
engine can reach: several valid classes, non-identity label maps, inclusive NMS, 1..4 merge sources, every overflow branch,
workspaces that hold the previous step's bytes.

Two rules hold for every kernel call here (class Harness):
  * guarded outputs - every output and workspace array has a sentinel tail behind the capacity the kernel is told; the tail
    must be bit-unchanged after the call;
  * dirty buffers - every call runs twice, once on zeroed buffers and once with every workspace and output filled with garbage
    (NaN floats, random integer bits) and every input row at or behind its count poisoned with NaN; the two results must be
    equal bit for bit.  Only the sticky flags (`overflow`, `any_boxes`) are zeroed by the caller, as include/mmdistill.h says.
Integer, order, label and score comparisons are assert_array_equal (on the bit patterns where signed zeros could hide)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mm_distillnet_amd import _lib
from oracle import effdet_ref as O
from oracle import losses_ref as L
from oracle import postproc_ref as P

call = _lib.call
DEV = "cuda"
VP = ctypes.c_void_p
PP_CAP = 1024
U = 2.0 ** -24          # half an ulp of a float32 in [1, 2): the relative error bound of one correctly rounded fp32 operation

_SENT = {torch.float32: (torch.int32, 0x7FDA5A5A), torch.int32: (torch.int32, 0x5A5A5A5A), torch.uint8: (torch.uint8, 0x5A),
         torch.int64: (torch.int64, 0x5A5A5A5A5A5A5A5A), torch.float64: (torch.int64, 0x7FF85A5A5A5A5A5A)}


def bits(a):
    """numpy float array -> its bit pattern (so that assert_array_equal tells -0.0 from 0.0 and compares NaNs)"""
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def eq(got, want, msg=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (msg, got.shape, want.shape)
    np.testing.assert_array_equal(bits(got), bits(want.astype(got.dtype)), err_msg=str(msg))


def same(a, b, path="result"):
    """clean-buffer result == dirty-buffer result, bit for bit (nested lists / tuples / dicts of arrays and ints)"""
    if isinstance(a, dict):
        assert a.keys() == b.keys()
        for k in a:
            same(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, f"{path}[{i}]")
    elif a is None:
        assert b is None, path
    else:
        eq(np.asarray(a), np.asarray(b), path + " (zeroed buffers vs dirty buffers)")


class Harness:
    """Allocates the buffers of one kernel call: zeroed (dirty=False) or full of garbage (dirty=True), always with a sentinel tail."""

    def __init__(self, dirty):
        self.dirty, self.guards = dirty, []

    def buf(self, shape, dtype=torch.float32, tail=64):
        n = int(np.prod(shape))
        full = torch.empty(n + tail, dtype=dtype, device=DEV)
        idt, sent = _SENT[dtype]
        body = full[:n].view(idt)
        if not self.dirty:
            body.zero_()
        elif dtype.is_floating_point:
            body.fill_(0x7FC12345 if dtype == torch.float32 else 0x7FF8000000012345)      # NaN
        elif dtype == torch.uint8:
            body.copy_(torch.randint(1, 256, (n,), dtype=torch.int16, device=DEV).to(torch.uint8))
        else:
            body.copy_(torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), dtype=torch.int64, device=DEV).to(idt) | 1)
        full[n:].view(idt).fill_(sent)
        self.guards.append((full[n:].view(idt), sent))
        return full[:n].view(shape)

    def flag(self):
        """a sticky flag: the one thing the header tells the caller to zero"""
        t = self.buf((1,), torch.int32)
        t.zero_()
        return t

    def rows(self, per_image, cap, cols, counts=None):
        """[B, cap, cols] input array from per-image row lists; the rows at and behind each count are NaN when dirty"""
        t = torch.full((len(per_image), cap) + ((cols,) if cols else ()), float("nan") if self.dirty else 0.0)
        for i, r in enumerate(per_image):
            r = np.asarray(r, dtype=np.float32).reshape((-1, cols) if cols else (-1,))
            k = min(r.shape[0], cap)
            t[i, :k] = torch.from_numpy(r[:k])
        return t.to(DEV)

    def check(self):
        torch.cuda.synchronize()
        for i, (g, sent) in enumerate(self.guards):
            assert bool((g == sent).all()), f"guard tail of buffer {i} was written"


def both(fn, *args, **kw):
    """run `fn(harness, ...)` on zeroed and on dirty buffers; the results must be bit-identical.  -> the dirty run's result"""
    out = []
    for dirty in (False, True):
        h = Harness(dirty)
        out.append(fn(h, *args, **kw))
        h.check()
    same(out[0], out[1])
    return out[1]


def nms_ws_floats(nmax):
    return int(_lib.LIB.load().mmd_nms_ws_floats(nmax))


def i32(x):
    return torch.tensor(list(x), dtype=torch.int32, device=DEV)


def r6(a):
    return np.asarray(a, dtype=np.float32).reshape(-1, 6)


def r5(a):
    return np.asarray(a, dtype=np.float32).reshape(-1, 5)


# =====================================================================================================================
# A. mmd_decode_filter against the front half of post_process
# =====================================================================================================================
THR = float(np.float32(0.3))
REAL_ANCHORS = {3069: 128, 12276: 256}


def synth_anchors(A, S, seed):
    if A in REAL_ANCHORS:
        return O.anchors_for(REAL_ANCHORS[A], 2)[0].contiguous().clone(), REAL_ANCHORS[A]
    gen = torch.Generator().manual_seed(seed)
    y1 = torch.rand(A, generator=gen) * (S - 24) - 8
    x1 = torch.rand(A, generator=gen) * (S - 24) - 8
    h = torch.rand(A, generator=gen) * 56 + 8
    w = torch.rand(A, generator=gen) * 56 + 8
    return torch.stack([y1, x1, y1 + h, x1 + w], 1).contiguous(), S


def decode_inputs(B, A, NC, ids, seed, zero_wh):
    """image 0: mixed (scores exactly AT the threshold, rows whose maximum two classes share); image 1: all below the threshold;
    image 2: every anchor above it; further images: mixed"""
    anchors, S = synth_anchors(A, 128, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    cls = torch.rand(B, A, NC, generator=gen) * 0.25
    hot = torch.rand(B, A, generator=gen) < 0.4
    pool = torch.tensor(sorted(set(list(ids) + [0, NC - 1, NC // 2])))
    k = pool[torch.randint(0, len(pool), (B, A), generator=gen)]
    val = 0.3 + 0.7 * torch.rand(B, A, generator=gen)
    cls.scatter_(2, k[..., None], torch.where(hot, val, cls.gather(2, k[..., None])[..., 0])[..., None])
    at = torch.arange(A) % 7 == 3                              # exactly the threshold: `>` is strict, must not pass
    cls[0, at] = cls[0, at].clamp(max=0.2)
    cls[0, at, int(pool[0])] = THR
    if NC > 1:                                                 # a maximum shared by two classes
        tie = torch.arange(A) % 11 == 5
        c0, c1 = int(pool[0]), int(pool[-1])
        cls[0, tie] = cls[0, tie].clamp(max=0.2)
        cls[0, tie, c0] = 0.75
        cls[0, tie, c1] = 0.75
    if B > 1:
        cls[1] = cls[1].clamp(max=0.29)
        cls[1, ::5, int(pool[0])] = THR
    if B > 2:
        cls[2, :, int(pool[-1])] = 0.5 + 0.5 * torch.rand(A, generator=gen)
    reg = torch.randn(B, A, 4, generator=gen) * 0.4
    if zero_wh:
        reg[..., 2:] = 0.0
    return cls, reg, anchors, S


def run_decode(h, cls, reg, anchors, S, ids, cap):
    B, A, NC = cls.shape
    mask = 0
    for i in ids:
        mask |= 1 << i
    score = h.buf((B * A,)); clsid = h.buf((B * A,), torch.uint8); flags = h.buf((B * A,), torch.uint8)
    over = h.buf((B, cap), tail=A + 64); cand = h.buf((B, cap, 6), tail=6 * (A + 64))
    n_over = h.buf((B,), torch.int32); n_keep = h.buf((B,), torch.int32)
    ovf = h.flag()
    call("mmd_decode_filter", cls.to(DEV), reg.to(DEV), anchors.to(DEV), B, A, NC, THR, mask, float(S), score, clsid, flags,
         over, cand, n_over, n_keep, ovf, cap)
    no, nk = n_over.cpu().tolist(), n_keep.cpu().tolist()
    assert all(0 <= a <= cap for a in no) and all(0 <= a <= cap for a in nk), (no, nk, cap)
    return {"n_over": no, "n_keep": nk, "overflow": int(ovf.item()),
            "over": [over[b, :no[b]].cpu().numpy() for b in range(B)], "cand": [cand[b, :nk[b]].cpu().numpy() for b in range(B)]}


def check_decode(got, cls, reg, anchors, S, ids, cap, exact):
    """exact (dh = dw = 0): every column bit-equal to the oracle.  General inputs: the box columns within the bound below.

    Bound of a box edge, e.g. x1 = xc - w / 2 with xc = dx * wa + xca, w = exp(dw) * wa, wa = a3 - a1, xca = (a1 + a3) / 2, against the
    same formula in float64.  Every fp32 operation is correctly rounded (relative error <= U = 2^-24 of its result; the divisions
    by 2 are exact), HIP's expf is documented at 1 ulp = 2 U.  To first order the absolute error of x1 is at most
        centre path  : U |a1 + a3| / 2  +  U |dx wa| (from wa)  +  U |dx wa| (product)  +  U |xc| (sum)        = 4 U M
        extent path  : (U (from wa) + 2 U (expf) + U (product)) w / 2                                          = 4 U M
        last op      : U |x1|                                                                                  = 1 U M
    with M the largest magnitude among the intermediates xca, dx wa, xc, w / 2, x1 (and their y / x2 / y2 counterparts) of the
    row: 9 U M, times (1 + 2^-10) for the second-order terms.  The clamp to [0, S] never increases an error."""
    B, A, NC = cls.shape
    ref = P.filter_candidates(cls, reg, anchors[None], S, THR, ids, cap)
    n_valid = [len(r[1]) for r in P.filter_candidates(cls, reg, anchors[None], S, THR, ids)]
    assert got["overflow"] == (1 if any(n > cap for n in n_valid) else 0), (n_valid, cap)
    if not exact:
        ref64 = P.filter_candidates(cls, reg.double(), anchors[None].double(), S, THR, ids, cap)
        a64, r64 = anchors.double(), reg.double()
    for b in range(B):
        bx, sc, cl, over, idx = ref[b]
        assert got["n_over"][b] == over.shape[0], (b, got["n_over"][b], over.shape)
        assert got["n_keep"][b] == sc.shape[0], (b, got["n_keep"][b], sc.shape)
        eq(got["over"][b], over, ("over_scores", b))
        c = got["cand"][b]
        eq(c[:, 4], sc, ("cand score", b))
        eq(c[:, 5], cl.astype(np.float32), ("cand class", b))
        if exact:
            eq(c[:, 0:4], bx, ("cand box", b))
        if exact or len(idx) == 0:
            continue
        want = torch.from_numpy(ref64[b][0])
        an, r = a64[idx], r64[b, idx]
        ha, wa = an[:, 2] - an[:, 0], an[:, 3] - an[:, 1]
        yca, xca = (an[:, 0] + an[:, 2]) / 2, (an[:, 1] + an[:, 3]) / 2
        pieces = [yca, xca, r[:, 0] * ha, r[:, 1] * wa, r[:, 0] * ha + yca, r[:, 1] * wa + xca, r[:, 2].exp() * ha / 2, r[:, 3].exp() * wa / 2]
        u64 = P.decode_boxes(a64[None], r64[[b]])[0][idx]
        M = torch.stack([p.abs() for p in pieces] + [u64[:, k].abs() for k in range(4)]).max(0)[0]
        err = (torch.from_numpy(c[:, 0:4]).double() - want).abs().max(1)[0]
        bound = 9 * U * M * (1 + 2.0 ** -10)
        print("decode image %d: max err %.3g, bound at that row %.3g" % (b, float(err.max()), float(bound[err.argmax()])))
        assert bool((err <= bound).all()), (b, float((err / bound).max()))


def _ids(kind, NC):
    return {"single": [min(6, NC - 1)], "three": sorted({0, NC // 2, NC - 1}), "high": [40], "high3": [3, 40, 63], "none": []}[kind]


DECODE_CASES = ([(A, 20, "single") for A in (5, 255, 256, 1024, 1025, 3069, 12276)] +
                [(1025, NC, kind) for NC in (1, 3, 7, 20, 64) for kind in ("single", "three")] +
                [(1025, 64, "high"), (3069, 64, "high3"), (1025, 20, "none"), (3069, 7, "none")])


@pytest.mark.parametrize("zero_wh", [True, False], ids=["exact", "general"])
@pytest.mark.parametrize("A,NC,kind", DECODE_CASES)
def test_decode_filter(A, NC, kind, zero_wh):
    ids = _ids(kind, NC)
    cls, reg, anchors, S = decode_inputs(3, A, NC, ids, 100 + A + NC, zero_wh)
    got = both(run_decode, cls, reg, anchors, S, ids, A)
    check_decode(got, cls, reg, anchors, S, ids, A, zero_wh)
    assert got["overflow"] == 0
    assert got["n_over"][1] == 0 and got["n_over"][2] == A
    if kind == "none":
        assert got["n_keep"] == [0, 0, 0] and got["n_over"][0] > 0


@pytest.mark.parametrize("A,NC,kind", [(1025, 20, "single"), (3069, 7, "three"), (12276, 64, "high3")])
def test_decode_filter_cap_below_valid_candidates(A, NC, kind):
    """cap below the number of valid candidates: overflow raised, n_keep == cap, the first cap rows are the oracle's"""
    ids = _ids(kind, NC)
    cls, reg, anchors, S = decode_inputs(3, A, NC, ids, 7 + A, True)
    n_valid = [len(r[1]) for r in P.filter_candidates(cls, reg, anchors[None], S, THR, ids)]
    cap = max(n_valid) // 2 + 1
    assert cap < max(n_valid)
    got = both(run_decode, cls, reg, anchors, S, ids, cap)
    assert got["overflow"] == 1
    assert got["n_keep"] == [min(n, cap) for n in n_valid] and cap in got["n_keep"]
    check_decode(got, cls, reg, anchors, S, ids, cap, True)


@pytest.mark.parametrize("A,NC", [(1025, 20), (3069, 64)])
def test_decode_filter_cap_between_keep_and_over(A, NC):
    """n_keep <= cap < n_over: not an overflow (only over_scores[< n_keep] is ever indexed); n_over == cap"""
    ids = [min(6, NC - 1)]
    cls, reg, anchors, S = decode_inputs(3, A, NC, ids, 31 + A, True)
    cls[2, :, NC - 1] = 0.2                                     # image 2: every anchor over the threshold, in a class that is not valid
    cls[2, :, 0] = 0.9
    cls[2, ::9, ids[0]] = 0.95
    full = P.filter_candidates(cls, reg, anchors[None], S, THR, ids)
    cap = max(len(r[1]) for r in full) + 3
    assert all(len(r[1]) <= cap for r in full) and len(full[2][3]) == A > cap and len(full[0][3]) > cap
    got = both(run_decode, cls, reg, anchors, S, ids, cap)
    assert got["overflow"] == 0 and got["n_over"][2] == cap and got["n_over"][0] == cap
    check_decode(got, cls, reg, anchors, S, ids, cap, True)


# =====================================================================================================================
# B. mmd_nms_teacher on synthetic candidate rows
# =====================================================================================================================
def run_teacher(h, cands, label_map, thr, inclusive, S, cap, big=True):
    """cands: per image (rows [n,6], over_scores [m])"""
    B = len(cands)
    cand = h.rows([c[0] for c in cands], cap, 6)
    over = h.rows([c[1] for c in cands], cap, 0)
    n_keep = i32([len(c[0]) for c in cands])
    out = h.buf((B, cap, 6), tail=6 * 64); cnt = h.buf((B,), torch.int32)
    mask = h.buf((B * 1024 * 16,), torch.int64)
    nf = nms_ws_floats(cap)
    big_ws = h.buf((B * nf,)) if (big and nf) else None
    ovf = h.flag()
    call("mmd_nms_teacher", cand, n_keep, over, i32(label_map), float(thr), int(inclusive), float(S), B, out, cnt, mask, ovf, cap, big_ws)
    n = cnt.cpu().tolist()
    assert all(0 <= k <= cap for k in n), n
    return {"rows": [out[b, :n[b]].cpu().numpy() for b in range(B)], "overflow": int(ovf.item())}


def check_teacher(cands, ids, label_map, thr=0.5, inclusive=0, S=16384, cap=None, expect=None):
    cap = cap or max(max(len(c[1]) for c in cands), 1) + 3
    got = both(run_teacher, cands, label_map, thr, inclusive, S, cap)
    assert got["overflow"] == 0
    want = P.candidates_to_ground_truth(cands, S, thr, P.make_valid(ids, label_map), bool(inclusive))
    for b in range(len(cands)):
        eq(got["rows"][b], r6(want[b]), ("image", b))
        if expect is not None:
            assert got["rows"][b].shape[0] == expect[b], (b, got["rows"][b].shape, expect[b])
    return got


def with_over(rows, seed=0, extra=5):
    """candidate rows -> (rows, over_scores): the over-threshold list is longer than the valid list and holds OTHER values than
    column 4, so that the score a kept row is given must come from over_scores[its index] (the reference's quirk)"""
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 6)
    rng = np.random.RandomState(seed + 77)
    return rows, (0.3 + 0.7 * rng.permutation(rows.shape[0] + extra) / (rows.shape[0] + extra + 1)).astype(np.float32)


def distinct_scores(n, rng):
    return (0.31 + 0.68 * rng.permutation(n) / max(n, 1)).astype(np.float32)


def geometry(family, n, seed, cls_ids=(6,)):
    """n candidate rows in shuffled order.  disjoint: a grid, everything is kept.  identical: one box, one row kept per class.
    staircase: box k = [4k, 0, 4k + 16, 16] with scores falling in k: neighbours overlap at IoU 0.6, boxes two apart at 1/3, so
    every other box survives and row k lives exactly when row k-1 is dead."""
    rng = np.random.RandomState(seed)
    k = np.arange(n, dtype=np.float32)
    if family == "disjoint":
        x, y = (k % 64) * 16 + 1.25, (k // 64) * 16 + 0.5
        box = np.stack([x, y, x + 9.5, y + 11.25], 1)
        sc = distinct_scores(n, rng)
    elif family == "identical":
        box = np.tile(np.float32([10.5, 12.25, 50.75, 61.0]), (n, 1))
        sc = distinct_scores(n, rng)
    else:
        box = np.stack([4 * k, 0 * k, 4 * k + 16, 0 * k + 16], 1)
        sc = (0.999 - 0.6 * k / max(n, 1)).astype(np.float32)
        assert n < 2 or (np.diff(sc) < 0).all()
    lab = np.asarray(cls_ids, dtype=np.float32)[np.arange(n) % len(cls_ids)] if family != "staircase" else np.full(n, cls_ids[0], np.float32)
    rows = np.concatenate([box, sc[:, None], lab[:, None]], 1).astype(np.float32)
    return rows[rng.permutation(n)]


def kept_count(family, n, ncls=1):
    return {"disjoint": n, "identical": min(n, ncls), "staircase": (n + 1) // 2}[family]


COUNT_BATCHES = [(63, 0, 64, 1), (65, 2, 448, 449), (1023, 0, 1024, 1025), (2048, 0, 2049, 3000)]


@pytest.mark.parametrize("counts", COUNT_BATCHES, ids=lambda c: "n" + "_".join(map(str, c)))
@pytest.mark.parametrize("family", ["disjoint", "identical", "staircase"])
def test_nms_teacher_row_counts(family, counts):
    """bitonic widths, the LDS / global switch of the mask (448 / 449), one-pass / chunked (1024 / 1025), chunked sort width
    (2048 / 2049), a suppression chain across chunk boundaries; an empty image between full ones"""
    cands = [with_over(geometry(family, n, 10 * n + i), i) for i, n in enumerate(counts)]
    label_map = list(range(20))
    check_teacher(cands, [6], label_map, expect=[kept_count(family, n) for n in counts])


@pytest.mark.parametrize("ids", [(2, 9), (2, 6, 9)])
@pytest.mark.parametrize("n", [7, 200, 1100])
def test_nms_teacher_identical_boxes_in_several_classes(ids, n):
    """identical boxes: one survives per class, whatever the number of rows of each class"""
    cands = [with_over(geometry("identical", n, n, ids)), with_over(geometry("disjoint", n, n + 1, ids), 1)]
    check_teacher(cands, list(ids), list(range(20)), expect=[len(ids), n])


@pytest.mark.parametrize("n,special", [(1025, 1024), (1024, 15 * 64 + 5), (2049, 2048), (70, 69)])
def test_nms_teacher_class_offset_needs_the_global_max(n, special):
    """The class offset is label * (max coordinate over ALL rows + 1).  Every row but one is the class-2 box [0,0,10,10]; row
    `special` (the last row of a chunked list, a row of wave 15) is the class-1 box [11,11,21,21] with the lowest score.  With the
    true maximum (21) the two classes land 22 apart and both survive; with a maximum that misses that row (10) both classes
    land on [22,22,32,32] and the class-1 box is suppressed."""
    rows = np.zeros((n, 6), np.float32)
    rows[:, 0:4] = [0, 0, 10, 10]
    rows[:, 4] = distinct_scores(n, np.random.RandomState(n))
    rows[:, 5] = 2
    rows[special] = [11, 11, 21, 21, 0.305, 1]
    got = check_teacher([with_over(rows)], [1, 2], list(range(20)), expect=[2])
    eq(got["rows"][0][:, 5], np.float32([2, 1]))


@pytest.mark.parametrize("n", [2, 65, 1100])
def test_nms_teacher_class_offset_plus_one(n):
    """The `+ 1` of the class offset only shows where a coordinate is negative (x2 / y2 are never clipped from below): with
    M the maximum coordinate, the class-1 box [M-2,M-2,M,M] and the class-2 box [-2,-2,0,0] land one pixel apart (IoU 1/7, both
    kept) with the offset label * (M + 1), and on top of each other with label * M."""
    M = 50.0
    rows = np.zeros((n, 6), np.float32)
    rows[:, 0:4] = [M - 2, M - 2, M, M]
    rows[:, 4] = distinct_scores(n, np.random.RandomState(n))
    rows[:, 5] = 1
    rows[n // 2] = [-2, -2, 0, 0, 0.305, 2]
    got = check_teacher([with_over(rows)], [1, 2], list(range(20)), expect=[2])
    eq(got["rows"][0][:, 5], np.float32([1, 2]))


@pytest.mark.parametrize("name,label_map", [("permutation", [(3 * i + 1) % 20 for i in range(20)]),
                                             ("many_to_one", [i // 7 for i in range(20)]),
                                             ("above_nc", [100 + 2 * i for i in range(20)])])
def test_nms_teacher_label_map(name, label_map):
    ids = [2, 6, 9, 19]
    cands = [with_over(geometry("disjoint", 90, 1, ids)), with_over(geometry("identical", 40, 2, ids), 1),
             with_over(geometry("disjoint", 1100, 3, ids), 2)]
    got = check_teacher(cands, ids, label_map, expect=[90, 4, 1100])
    assert set(np.unique(got["rows"][0][:, 5]).tolist()) == {float(label_map[i]) for i in ids}


def threshold_pairs():
    """pairs at IoU exactly 1/2 ([0,0,2,2] against [0,0,2,1]: 2 / (4 + 2 - 2)), moved copies and dyadic multiples, each pair far
    from the others; the lower-score row of a pair is the [.., 2m, m] box"""
    rows, k = [], 0
    for m in (1, 4, 64):
        for ox, oy in ((0, 0), (3, 5), (1000, 2000)):
            x, y = ox + 300 * k, oy + 300 * k
            rows.append([x, y, x + 2 * m, y + 2 * m, 0.9 - 0.01 * k, 6])
            rows.append([x, y, x + 2 * m, y + m, 0.5 - 0.01 * k, 6])
            k += 1
    return np.float32(rows)


THR_EDGE = [(float(np.nextafter(np.float32(0.5), np.float32(0))), "below"), (0.5, "at"),
            (float(np.nextafter(np.float32(0.5), np.float32(1))), "above")]


@pytest.mark.parametrize("inclusive", [0, 1])
@pytest.mark.parametrize("thr,where", THR_EDGE, ids=[w for _, w in THR_EDGE])
def test_nms_teacher_threshold_equality(thr, where, inclusive):
    """IoU == threshold is the one case where `inclusive` matters; one ulp either side of it the flag must not matter"""
    rows = threshold_pairs()
    npairs = rows.shape[0] // 2
    suppressed = where == "below" or (where == "at" and inclusive)
    check_teacher([with_over(rows), with_over(rows[::-1].copy(), 1)], [6], list(range(20)), thr=thr, inclusive=inclusive,
                  expect=[npairs if suppressed else 2 * npairs] * 2)


@pytest.mark.parametrize("n", [64, 300, 1100, 2100])
@pytest.mark.parametrize("pattern", ["all_equal", "blocks", "signed_zero"])
def test_nms_teacher_score_ties(pattern, n):
    """equal scores sort index-ascending: on the staircase (in row order) that decides which half survives.  Ties straddle the
    1024-row chunk boundary for n > 1024; -0.0 and 0.0 are the same score."""
    rows = geometry("staircase", n, 0)
    rows = rows[np.argsort(rows[:, 0], kind="stable")]
    if pattern == "all_equal":
        rows[:, 4] = 0.5
    elif pattern == "blocks":
        rows[:, 4] = np.float32(0.9) - np.float32(0.1) * ((np.arange(n) * 7 // 1000) % 5).astype(np.float32)
    else:
        rows[:, 4] = np.where(np.arange(n) % 3 == 0, np.float32(-0.0), np.float32(0.0))
    rev = rows[::-1].copy()
    got = check_teacher([with_over(rows), with_over(rev, 1)], [6], list(range(20)))
    if pattern != "blocks":
        eq(got["rows"][0][:, 0], np.arange(0, n, 2, dtype=np.float32) * 4)        # rows 0, 2, 4, ... in that order
        eq(got["rows"][1][:, 0], np.arange(n - 1, -1, -2, dtype=np.float32) * 4)


def test_nms_teacher_zero_area_boxes():
    """x2 == x1: the IoU of two such boxes is 0 / 0 = NaN, which suppresses nothing - on both sides"""
    rng = np.random.RandomState(4)
    rows = []
    for k in range(40):
        rows.append([30, 40, 30, 90, 0, 6])            # zero width, all identical
        rows.append([50, 60, 80, 60, 0, 6])            # zero height
        rows.append([70, 70, 70, 70, 0, 9])            # a point
        rows.append([30, 40, 60, 90, 0, 6])            # a real box over the first ones
    rows = np.float32(rows)
    rows[:, 4] = distinct_scores(rows.shape[0], rng)
    check_teacher([with_over(rows)], [6, 9], list(range(20)), expect=[121])


def test_nms_teacher_coordinate_truncation():
    """fractional parts, negatives (clipped at 0), values above and exactly at image_size in the emitted rows"""
    S = 128
    rng = np.random.RandomState(8)
    n = 400
    x1 = rng.uniform(-20, 120, n); y1 = rng.uniform(-20, 120, n)
    rows = np.stack([x1, y1, x1 + rng.uniform(1, 60, n), y1 + rng.uniform(1, 60, n), distinct_scores(n, rng),
                     rng.choice([6, 9], n)], 1).astype(np.float32)
    rows[0, 0:4] = [-0.5, -3.75, 128.0, 128.0]
    rows[1, 0:4] = [127.99, 0.999, 128.5, 1000.0]
    rows[2, 0:4] = [-0.0, 5.5, 127.999, 128.001]
    got = check_teacher([with_over(rows)], [6, 9], [(3 * i + 1) % 20 for i in range(20)], S=S)
    out = got["rows"][0]
    assert out[:, 0:2].min() == 0 and out[:, 2:4].max() == S and (out[:, 0:4] == np.floor(out[:, 0:4])).all()
    assert out[:, 2:4].min() < 0          # x2 / y2 are only clipped from above, as in the reference


@pytest.mark.parametrize("n", [1025, 1300])
def test_nms_teacher_overflow_without_workspace(n):
    """big_ws = NULL and more than 1024 rows: overflow raised, the result is the NMS of the first 1024 rows in source order"""
    cands = [with_over(geometry("staircase", n, 1)), with_over(geometry("disjoint", 100, 2), 1), with_over(geometry("disjoint", n, 3), 2)]
    cap = 1500
    got = both(run_teacher, cands, list(range(20)), 0.5, 0, 16384, cap, big=False)
    assert got["overflow"] == 1
    cut = [(r[:PP_CAP], o) for r, o in cands]
    want = P.candidates_to_ground_truth(cut, 16384, 0.5, P.make_valid([6], list(range(20))))
    for b in range(3):
        eq(got["rows"][b], r6(want[b]), b)
    assert got["rows"][2].shape[0] == PP_CAP


# =====================================================================================================================
# C. mmd_nms_merge / mmd_nms_merge_n against merge_teacher_labels
# =====================================================================================================================
def teacher_rows(n, seed, S=400):
    """n per-teacher output rows: integer boxes that overlap a lot, distinct scores, labels of several classes"""
    rng = np.random.RandomState(seed)
    x1 = rng.randint(0, S, n); y1 = rng.randint(0, S, n)
    return np.stack([x1, y1, x1 + rng.randint(8, 72, n), y1 + rng.randint(8, 72, n), distinct_scores(n, rng),
                     rng.choice([1, 5, 7, 19], n)], 1).astype(np.float32)


def run_merge(h, srcs, thr, inclusive, maxg, merge01, cap, entry="n", big=True, cnt_add=None):
    """srcs: per source, per image [n,6] rows.  cnt_add: per source, per image number added to the count handed to the kernel"""
    nsrc, B = len(srcs), len(srcs[0])
    t = [h.rows(s, cap, 6) for s in srcs]
    c = [i32([min(len(a), cap) + (cnt_add[k][i] if cnt_add else 0) for i, a in enumerate(s)]) for k, s in enumerate(srcs)]
    boxes = h.buf((B, maxg, 5), tail=5 * 64); nbox = h.buf((B,), torch.int32)
    mask = h.buf((B * 1024 * 16,), torch.int64)
    nf = nms_ws_floats(nsrc * cap * (2 if (merge01 and B >= 2) else 1))
    big_ws = h.buf((B * nf,)) if (big and nf) else None
    ovf = h.flag()
    if entry == "n":
        call("mmd_nms_merge_n", (VP * nsrc)(*[x.data_ptr() for x in t]), (VP * nsrc)(*[x.data_ptr() for x in c]), nsrc, float(thr),
             int(inclusive), B, boxes, nbox, maxg, mask, ovf, int(merge01), cap, big_ws)
    else:
        t3, c3 = t + [None] * (3 - nsrc), c + [None] * (3 - nsrc)
        call("mmd_nms_merge", t3[0], c3[0], t3[1], c3[1], t3[2], c3[2], nsrc, float(thr), int(inclusive), B, boxes, nbox, maxg, mask,
             ovf, int(merge01), cap, big_ws)
    n = nbox.cpu().tolist()
    assert all(0 <= k <= maxg for k in n), n
    return {"boxes": [boxes[b, :n[b]].cpu().numpy() for b in range(B)], "overflow": int(ovf.item())}


def check_merge(srcs, thr=0.5, inclusive=0, maxg=None, merge01=0, cap=None, cnt_add=None, overflow=0):
    nsrc, B = len(srcs), len(srcs[0])
    cap = cap or max(max(len(a) for a in s) for s in srcs) + 2
    full = nsrc * cap * (2 if merge01 else 1)
    maxg_ = maxg or full
    got = both(run_merge, srcs, thr, inclusive, maxg_, merge01, cap, "n", True, cnt_add)
    if nsrc <= 3:      # the three-pointer entry: the same bits
        same(got, both(run_merge, srcs, thr, inclusive, maxg_, merge01, cap, "3", True, cnt_add))
    assert got["overflow"] == overflow
    want = P.merge_teacher_labels([[a[:cap] for a in s] for s in srcs], B, thr, bool(inclusive), bool(merge01), max_boxes=maxg)
    for b in range(B):
        eq(got["boxes"][b], r5(want[b]), ("image", b))
    return got, want


# per image, the total row count of the concatenation; the split over the sources leaves some sources empty for some images
MERGE_TOTALS = {"small": (0, 3, 40), "boundary": (1024, 1025, 2049), "mixed": (700, 0, 1500)}


def split_counts(total, nsrc, img):
    if nsrc == 1 or total == 0:
        return [total] + [0] * (nsrc - 1)
    parts = [total // nsrc] * nsrc
    parts[img % nsrc] = 0                       # one source has nothing for this image
    parts[(img + 1) % nsrc] += total - sum(parts)
    return parts


@pytest.mark.parametrize("totals", list(MERGE_TOTALS), ids=list(MERGE_TOTALS))
@pytest.mark.parametrize("nsrc", [1, 2, 3, 4])
def test_nms_merge_sources_and_counts(nsrc, totals):
    tot = MERGE_TOTALS[totals]
    per = [split_counts(t, nsrc, i) for i, t in enumerate(tot)]
    srcs = [[teacher_rows(per[i][k], 1000 * k + i, S=1500) for i in range(len(tot))] for k in range(nsrc)]
    got, _ = check_merge(srcs)
    labels = np.concatenate([b[:, 4] for b in got["boxes"]])
    assert len(np.unique(labels)) > 1                  # class-agnostic: several labels pass through


def test_nms_merge_count_above_cap_is_clamped():
    """cnt[] larger than cap: the kernel reads cap rows of that source, not more"""
    srcs = [[teacher_rows(50, 10 * k + i) for i in range(2)] for k in range(3)]
    check_merge(srcs, cap=50, cnt_add=[[5, 0], [0, 1000], [7, 7]])
    srcs = [[teacher_rows(n, 10 * k + i) for i, n in enumerate((30, 50))] for k in range(2)]
    check_merge(srcs, cap=50, cnt_add=[[0, 9], [0, 1]])


@pytest.mark.parametrize("merge01", [0, 1])
@pytest.mark.parametrize("empty", ["none", "image0", "image1"])
@pytest.mark.parametrize("B", [1, 2, 3])
def test_nms_merge_merge01(B, empty, merge01):
    """image 1 takes image 0's rows in front of its own when both have rows; ignored for B = 1"""
    n = [60, 45, 30][:B]
    if empty == "image0":
        n[0] = 0
    if empty == "image1" and B > 1:
        n[1] = 0
    srcs = [[teacher_rows(n[i] + k, 100 * k + i) if n[i] else np.zeros((0, 6), np.float32) for i in range(B)] for k in range(3)]
    got, want = check_merge(srcs, merge01=merge01)
    if B > 1 and empty == "none":
        plain = P.merge_teacher_labels(srcs, B, 0.5, False, False)
        assert (len(want[1]) != len(plain[1])) == bool(merge01)


@pytest.mark.parametrize("nsrc", [2, 4])
def test_nms_merge_merge01_crosses_1024(nsrc):
    """image 0 (600 rows) stays on the one-pass path, image 1 (600 + 500 rows) takes the chunked one"""
    per = [600 // nsrc, 500 // nsrc, 20]
    srcs = [[teacher_rows(per[i], 50 * k + i, S=1200) for i in range(3)] for k in range(nsrc)]
    check_merge(srcs, merge01=1)


def test_nms_merge_equal_scores_across_sources():
    """the same row from two teachers (and the same score on different boxes): the earlier source wins, then the lower index"""
    a = teacher_rows(300, 1)
    b = a.copy(); b[:, 5] = 3                      # same boxes and scores, another label: the label tells which source's row was kept
    c = teacher_rows(300, 2); c[:, 4] = a[:, 4]     # other boxes, the same scores
    z = np.zeros((0, 6), np.float32)
    got, _ = check_merge([[a, b, z], [b, a, a], [c, c, c]])
    assert (got["boxes"][0][:, 4] != 3).all()      # image 0: every row of `b` loses against its copy in the earlier source
    got, _ = check_merge([[a], [b]])
    assert (got["boxes"][0][:, 4] != 3).all()
    got, _ = check_merge([[b], [a]])
    assert (got["boxes"][0][:, 4] == 3).all()


@pytest.mark.parametrize("ntot", [300, 1500])
def test_nms_merge_maxg_below_kept_count(ntot):
    """max_boxes below the kept count: overflow raised, nbox == maxg, the rows are the first maxg kept rows"""
    srcs = [[teacher_rows(ntot // 3, 10 * k + i, S=1500) for i in range(2)] for k in range(3)]
    kept = [len(w) for w in P.merge_teacher_labels(srcs, 2, 0.5)]
    maxg = min(kept) // 2
    got, _ = check_merge(srcs, maxg=maxg, overflow=1)
    assert [len(b) for b in got["boxes"]] == [maxg, maxg]


@pytest.mark.parametrize("inclusive", [0, 1])
@pytest.mark.parametrize("thr,where", THR_EDGE, ids=[w for _, w in THR_EDGE])
def test_nms_merge_threshold_equality(thr, where, inclusive):
    rows = threshold_pairs()
    npairs = rows.shape[0] // 2
    suppressed = where == "below" or (where == "at" and inclusive)
    got, _ = check_merge([[rows[0::2], rows[1::2]], [rows[1::2], rows[0::2]]], thr=thr, inclusive=inclusive)
    assert [len(b) for b in got["boxes"]] == [npairs if suppressed else 2 * npairs] * 2


def test_nms_merge_argument_checks():
    """bad arguments are refused before anything is launched: the outputs keep their bytes"""
    h = Harness(True)
    cap, B, maxg = 8, 2, 16
    t = [h.rows([teacher_rows(4, i), teacher_rows(3, i + 9)], cap, 6) for i in range(4)]
    c = [i32([4, 3]) for _ in range(4)]
    boxes = h.buf((B, maxg, 5)); nbox = h.buf((B,), torch.int32); mask = h.buf((B * 1024 * 16,), torch.int64); ovf = h.flag()
    before = (bits(boxes.cpu().numpy()).copy(), nbox.cpu().numpy().copy())
    tp = lambda n, null=None: (VP * n)(*[None if i == null else t[i % 4].data_ptr() for i in range(n)])
    cp = lambda n, null=None: (VP * n)(*[None if i == null else c[i % 4].data_ptr() for i in range(n)])
    bad = [(tp(1), cp(1), 0, maxg), (tp(5), cp(5), 5, maxg), (tp(2, 1), cp(2), 2, maxg), (tp(3), cp(3, 2), 3, maxg), (tp(2), cp(2), 2, 0),
           (None, cp(2), 2, maxg)]
    for srcs, cnts, nsrc, mg in bad:
        with pytest.raises(RuntimeError, match="mmd_nms_merge_n failed with status -22"):
            call("mmd_nms_merge_n", srcs, cnts, nsrc, 0.5, 0, B, boxes, nbox, mg, mask, ovf, 0, cap, None)
    for nt in (0, 4):
        with pytest.raises(RuntimeError, match="mmd_nms_merge failed with status -22"):
            call("mmd_nms_merge", t[0], c[0], t[1], c[1], t[2], c[2], nt, 0.5, 0, B, boxes, nbox, maxg, mask, ovf, 0, cap, None)
    with pytest.raises(RuntimeError, match="status -22"):
        call("mmd_nms_merge", t[0], c[0], None, c[1], t[2], c[2], 2, 0.5, 0, B, boxes, nbox, maxg, mask, ovf, 0, cap, None)
    h.check()
    eq(bits(boxes.cpu().numpy()), before[0]); eq(nbox.cpu().numpy(), before[1])
    assert int(ovf.item()) == 0


# =====================================================================================================================
# D. mmd_focal_loss on what the merge produces
# =====================================================================================================================
def assert_focal_inputs_decidable(anchors, ann):
    """A condition on the INPUTS (float64, CPU): no anchor's best IoU lies within 1e-5 of the 0.4 / 0.5 thresholds, and where an
    anchor is not a plain negative no other box comes within 1e-6 of its best one unless it is an exact duplicate of it (the
    duplicates placed on purpose; 'first maximum wins' then decides).  With that the assignment needs no tolerance."""
    a = anchors.double()
    for i, rows in enumerate(ann):
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, 5)
        if rows.shape[0] == 0:
            continue
        b = torch.from_numpy(rows[:, :4])
        iou = L.calc_iou(a, b)
        mx, arg = iou.max(1)
        assert float((mx - 0.4).abs().min()) > 1e-5 and float((mx - 0.5).abs().min()) > 1e-5, i
        near = (iou >= mx[:, None] - 1e-6) & (mx[:, None] >= 0.4 - 1e-5)
        for k in torch.nonzero(near.sum(1) > 1).reshape(-1).tolist():
            js = torch.nonzero(near[k]).reshape(-1)
            assert bool((b[js] == b[arg[k]]).all()), (i, k, js.tolist())


def anchor_boxes(anchors, n, seed, NC, S):
    """n integer boxes, each a rounded and nudged copy of a random anchor inside the image (so that anchors are positive).  A
    candidate box is dropped when it would leave an anchor undecidable (see assert_focal_inputs_decidable; the level-3 anchors have
    integer corners, so exact IoUs of 1/2 against integer boxes are common)."""
    rng = np.random.RandomState(seed)
    an = anchors.numpy()
    a64 = anchors.double()
    inside = np.nonzero((an[:, 0] >= 0) & (an[:, 1] >= 0) & (an[:, 2] <= S) & (an[:, 3] <= S) & (an[:, 2] - an[:, 0] < S / 2))[0]
    out, best = [], torch.zeros(an.shape[0], dtype=torch.float64)
    while len(out) < n:
        p = an[rng.choice(inside)]
        d = rng.randint(-2, 3, 4)
        box = np.clip([np.floor(p[1]) + d[0], np.floor(p[0]) + d[1], np.ceil(p[3]) + d[2], np.ceil(p[2]) + d[3]], 0, S)
        iou = L.calc_iou(a64, torch.from_numpy(box[None, :]).double())[:, 0]
        top = torch.maximum(iou, best)
        if float(torch.minimum((iou - 0.4).abs(), (iou - 0.5).abs()).min()) < 1e-4 or bool(((top >= 0.39) & ((iou - best).abs() < 1e-5)).any()):
            continue
        best = top
        out.append(list(box) + [rng.randint(0, NC)])
    return np.float32(out)


def student_outputs(B, A, NC, seed):
    gen = torch.Generator().manual_seed(seed)
    cls = torch.sigmoid(torch.randn(B, A, NC, generator=gen) * 2 - 2)
    cls[0, :50] = 0.0
    cls[-1, :50] = 1.0
    return cls, torch.randn(B, A, 4, generator=gen) * 0.3


def run_focal(h, cls, reg, anchors, ann, maxg, to_logit=0, grads=True, nbox=None):
    """ann: per image [n,5] rows handed to the kernel (nbox: the counts it is told, default n); rows behind the count are NaN when dirty"""
    B, A, NC = cls.shape
    boxes = h.rows(ann, maxg, 5)
    nb = i32(nbox if nbox is not None else [len(a) for a in ann])
    assign = h.buf((B * A,), torch.int32); npos = h.buf((B,), torch.int32); acc = h.buf((2 * B,), torch.float64)
    out = h.buf((2,))
    dcls = h.buf((B, A, NC)) if grads else None
    dreg = h.buf((B, A, 4)) if grads else None
    anyb = h.flag()
    call("mmd_focal_loss", cls.to(DEV), reg.to(DEV), anchors.to(DEV), boxes, nb, maxg, B, A, NC, assign, npos, acc, out, dcls, dreg, 1.0,
         int(to_logit), anyb)
    return {"loss": out.cpu().numpy(), "dcls": dcls.cpu().numpy() if grads else None, "dreg": dreg.cpu().numpy() if grads else None,
            "any": int(anyb.item())}


def check_focal(cls, reg, anchors, ann_kernel, ann_oracle, maxg, nbox=None, to_logits=(0, 1), null_grads=True):
    """tolerances of test_focal_golden: loss rtol 2e-4, atol 1e-7; gradients 2e-3 * max|ref| + 1e-9"""
    assert_focal_inputs_decidable(anchors, ann_oracle)
    c2, r2 = cls.clone().requires_grad_(True), reg.clone().requires_grad_(True)
    rl, cl = L.focal_loss(c2, r2, anchors[None], ann_oracle)
    has = rl.requires_grad or cl.requires_grad
    if has:
        (rl.sum() + cl.sum()).backward()
    gc = c2.grad if has else torch.zeros_like(cls)
    gr = r2.grad if (has and r2.grad is not None) else torch.zeros_like(reg)
    for to_logit in to_logits:
        got = both(run_focal, cls, reg, anchors, ann_kernel, maxg, to_logit, True, nbox)
        np.testing.assert_allclose(got["loss"][0], rl.item(), rtol=2e-4, atol=1e-7)
        np.testing.assert_allclose(got["loss"][1], cl.item(), rtol=2e-4, atol=1e-7)
        ref = gc * cls * (1 - cls) if to_logit else gc
        print("focal to_logit=%d: dcls err %.3g (ref max %.3g), dreg err %.3g (ref max %.3g)" % (
            to_logit, (torch.from_numpy(got["dcls"]) - ref).abs().max(), ref.abs().max(), (torch.from_numpy(got["dreg"]) - gr).abs().max(),
            gr.abs().max()))
        assert (torch.from_numpy(got["dcls"]) - ref).abs().max().item() <= 2e-3 * ref.abs().max().item() + 1e-9
        assert (torch.from_numpy(got["dreg"]) - gr).abs().max().item() <= 2e-3 * gr.abs().max().item() + 1e-9
        assert got["any"] == (1 if any(len(a) for a in ann_oracle) else 0)
    if null_grads:      # loss only
        got0 = both(run_focal, cls, reg, anchors, ann_kernel, maxg, 0, False, nbox)
        eq(got0["loss"], got["loss"])
    return got


FOCAL_S = 128


def focal_setup(NC, seed, B=3):
    anchors = O.anchors_for(FOCAL_S, 2)[0].contiguous().clone()           # A = 3069 = 11 * 256 + 253
    assert anchors.shape[0] % 256 != 0
    cls, reg = student_outputs(B, anchors.shape[0], NC, seed)
    return anchors, cls, reg


@pytest.mark.parametrize("NC", [3, 7, 20])
def test_focal_classes_and_empty_middle_image(NC):
    """scalar (NC % 4 != 0) and float4 class paths, A not a multiple of 256, B = 3 with the middle image empty"""
    anchors, cls, reg = focal_setup(NC, 40 + NC)
    ann = [anchor_boxes(anchors, 25, 1 + NC, NC, FOCAL_S), np.zeros((0, 5), np.float32), anchor_boxes(anchors, 7, 2 + NC, NC, FOCAL_S)]
    check_focal(cls, reg, anchors, ann, ann, 40)


@pytest.mark.parametrize("NC", [7, 20])
def test_focal_nbox_above_maxg(NC):
    """nbox[b] > maxg is clamped: only the first maxg boxes count (the rows behind them are not there at all)"""
    anchors, cls, reg = focal_setup(NC, 50 + NC)
    maxg = 12
    ann = [anchor_boxes(anchors, maxg, 3, NC, FOCAL_S), anchor_boxes(anchors, 5, 4, NC, FOCAL_S), anchor_boxes(anchors, maxg, 5, NC, FOCAL_S)]
    check_focal(cls, reg, anchors, ann, ann, maxg, nbox=[maxg + 30, 5, maxg + 1])


@pytest.mark.parametrize("NC", [3, 20])
def test_focal_duplicates_and_degenerate_boxes(NC):
    """exact duplicate boxes with different labels (the first wins), zero-width / zero-height / point boxes (never positive; first in
    the list, where the disjoint-pair shortcut does not apply), a NaN row behind nbox"""
    anchors, cls, reg = focal_setup(NC, 60 + NC)
    real = anchor_boxes(anchors, 20, 6, NC, FOCAL_S)
    dup = real[:8].copy()
    dup[:, 4] = (dup[:, 4] + 1) % NC
    degenerate = np.float32([[40, 30, 40, 90, 1], [20, 64, 100, 64, 2], [64, 64, 64, 64, 0]])
    ann0 = np.concatenate([degenerate, real[:10], dup, real[10:], degenerate])
    ann2 = np.concatenate([dup[::-1], real])
    ann = [ann0, degenerate, ann2]
    check_focal(cls, reg, anchors, ann, ann, 64)


def test_focal_more_boxes_than_the_lds_stage_holds():
    """1100 boxes in one image (max_boxes = 0 sizes G to nt * cap): the first 1060 are 1-pixel boxes no anchor can match, the boxes
    that make anchors positive have indices >= 1024"""
    NC = 20
    anchors, cls, reg = focal_setup(NC, 77)
    rng = np.random.RandomState(9)
    px = rng.permutation(FOCAL_S * FOCAL_S)[:1060]
    tiny = np.stack([px % FOCAL_S, px // FOCAL_S, px % FOCAL_S + 1, px // FOCAL_S + 1, rng.randint(0, NC, 1060)], 1).astype(np.float32)
    ann = [np.concatenate([tiny, anchor_boxes(anchors, 40, 10, NC, FOCAL_S)]), anchor_boxes(anchors, 3, 11, NC, FOCAL_S),
           np.zeros((0, 5), np.float32)]
    iou = L.calc_iou(anchors.double(), torch.from_numpy(ann[0][:, :4]).double())
    mx, arg = iou.max(1)
    assert int(((mx >= 0.5) & (arg >= 1024)).sum()) >= 20 and int(((mx >= 0.5) & (arg < 1024)).sum()) == 0
    check_focal(cls, reg, anchors, ann, ann, 1100, to_logits=(0,))


def test_focal_any_boxes_is_sticky():
    """an all-empty batch: zero loss, zero gradients, any_boxes stays 0; once raised it stays raised over an empty batch"""
    NC = 7
    anchors, cls, reg = focal_setup(NC, 5)
    empty = [np.zeros((0, 5), np.float32)] * 3
    got = check_focal(cls, reg, anchors, empty, empty, 16)
    assert got["any"] == 0 and not got["loss"].any() and not got["dcls"].any() and not got["dreg"].any()
    h = Harness(True)
    B, A = cls.shape[0], cls.shape[1]
    anyb = h.flag()
    res = []
    for ann in (empty, [anchor_boxes(anchors, 5, 1, NC, FOCAL_S)] + empty[:2], empty):
        out = h.buf((2,))
        call("mmd_focal_loss", cls.to(DEV), reg.to(DEV), anchors.to(DEV), h.rows(ann, 16, 5), i32([len(a) for a in ann]), 16, B, A, NC,
             h.buf((B * A,), torch.int32), h.buf((B,), torch.int32), h.buf((2 * B,), torch.float64), out, None, None, 1.0, 0, anyb)
        res.append(int(anyb.item()))
    h.check()
    assert res == [0, 1, 1]


# =====================================================================================================================
# E. the chain: decode -> per-teacher NMS x 3 -> merge_n -> focal loss, one stream, one dirty bump allocation
# =====================================================================================================================
class Bump:
    """One allocation handed out in slices, as the engine's arena does, pre-filled with a NaN bit pattern; 256 untouched bytes
    between two slices serve as guards."""
    FILL = 0x7FDA5A5A

    def __init__(self, nbytes):
        self.raw = torch.full((nbytes // 4,), self.FILL, dtype=torch.int32, device=DEV)
        self.off, self.used = 64, []

    def alloc(self, shape, dtype=torch.float32):
        nb = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        words = (nb + 3) // 4
        assert self.off + words + 64 <= self.raw.numel()
        t = self.raw[self.off:self.off + words].view(torch.uint8)[:nb].view(dtype).view(shape)
        self.used.append((self.off, words))
        self.off = (self.off + words + 64 + 63) // 64 * 64
        return t

    def put(self, x):
        t = self.alloc(tuple(x.shape), x.dtype)
        t.copy_(x)
        return t

    def check(self):
        live = torch.zeros(self.raw.numel(), dtype=torch.bool, device=DEV)
        for off, words in self.used:
            live[off:off + words] = True
        assert bool((self.raw[~live] == self.FILL).all()), "bytes between the arena's slices were written"


def chain_inputs(seed, B, A, NC, ids):
    """a teacher's head outputs: ~40 anchors per image over the threshold in a valid class (some of them on top of each other, so
    that the NMS has work), ~60 in a class that is not valid (so that over_scores and the candidate list differ)"""
    gen = torch.Generator().manual_seed(seed)
    cls = torch.sigmoid(torch.randn(B, A, NC, generator=gen) * 1.5 - 3.0).clamp(max=0.29)
    for b in range(B):
        perm = torch.randperm(A, generator=gen)
        hot = torch.cat([perm[:30], (perm[:10] + 1) % A])
        cls[b, hot, ids[0]] = 0.5 + 0.4 * torch.rand(40, generator=gen)
        cls[b, hot[::3], ids[1]] = 0.95
        cls[b, perm[100:160], 0] = 0.6
    reg = torch.randn(B, A, 4, generator=gen) * 0.4
    reg[..., 2:] = 0.0                      # dh = dw = 0: exp(0) is exact, the decode is bit-exact
    return cls, reg


def test_chain_on_one_dirty_arena():
    S, B, NC, ids = 128, 2, 20, [6, 14]
    label_map = [(3 * i + 1) % NC for i in range(NC)]
    valid = P.make_valid(ids, label_map)
    mask_bits = sum(1 << i for i in ids)
    anchors = O.anchors_for(S, 2)
    A = anchors.shape[1]
    teachers = [chain_inputs(3600 + t, B, A, NC, ids) for t in range(3)]      # (seeds for which the merged boxes are decidable, asserted below)
    cls_s, reg_s = student_outputs(B, A, NC, 9)
    # ---- oracle chain
    gts = [P.logits_to_ground_truth([c, r, anchors], S, THR, 0.5, valid) for c, r in teachers]
    merged = P.merge_teacher_labels(gts, B, 0.5)
    assert all(20 <= len(g) <= 60 for t in gts for g in t) and len({float(x) for m in merged for x in r5(m)[:, 4]}) == 2
    assert_focal_inputs_decidable(anchors[0], merged)
    c2, r2 = cls_s.clone().requires_grad_(True), reg_s.clone().requires_grad_(True)
    rl, cl = L.focal_loss(c2, r2, anchors, merged)
    (rl.sum() + cl.sum()).backward()
    # ---- device chain
    cap, G = A, 3 * A
    arena = Bump(48 << 20)
    d_anchors, d_map = arena.put(anchors[0].contiguous()), arena.put(torch.tensor(label_map, dtype=torch.int32))
    d_t = [(arena.put(c), arena.put(r)) for c, r in teachers]
    d_cls, d_reg = arena.put(cls_s), arena.put(reg_s)
    ovf, anyb = arena.alloc((1,), torch.int32), arena.alloc((1,), torch.int32)
    per = []
    for _ in range(3):
        per.append(dict(score=arena.alloc((B * A,)), clsid=arena.alloc((B * A,), torch.uint8), flags=arena.alloc((B * A,), torch.uint8),
                        over=arena.alloc((B, cap)), cand=arena.alloc((B, cap, 6)), n_over=arena.alloc((B,), torch.int32),
                        n_keep=arena.alloc((B,), torch.int32), rows=arena.alloc((B, cap, 6)), cnt=arena.alloc((B,), torch.int32),
                        mask=arena.alloc((B * 1024 * 16,), torch.int64), big=arena.alloc((B * nms_ws_floats(cap),))))
    boxes, nbox = arena.alloc((B, G, 5)), arena.alloc((B,), torch.int32)
    mmask, mbig = arena.alloc((B * 1024 * 16,), torch.int64), arena.alloc((B * nms_ws_floats(3 * cap),))
    assign, npos, acc = arena.alloc((B * A,), torch.int32), arena.alloc((B,), torch.int32), arena.alloc((2 * B,), torch.float64)
    out, dcls, dreg = arena.alloc((2,)), arena.alloc((B, A, NC)), arena.alloc((B, A, 4))
    srcs = (VP * 3)(*[p["rows"].data_ptr() for p in per]); cnts = (VP * 3)(*[p["cnt"].data_ptr() for p in per])

    def run():
        ovf.zero_(); anyb.zero_()               # the sticky flags: all the caller has to zero
        for (c, r), p in zip(d_t, per):
            call("mmd_decode_filter", c, r, d_anchors, B, A, NC, THR, mask_bits, float(S), p["score"], p["clsid"], p["flags"], p["over"],
                 p["cand"], p["n_over"], p["n_keep"], ovf, cap)
            call("mmd_nms_teacher", p["cand"], p["n_keep"], p["over"], d_map, 0.5, 0, float(S), B, p["rows"], p["cnt"], p["mask"], ovf, cap,
                 p["big"])
        call("mmd_nms_merge_n", srcs, cnts, 3, 0.5, 0, B, boxes, nbox, G, mmask, ovf, 0, cap, mbig)
        call("mmd_focal_loss", d_cls, d_reg, d_anchors, boxes, nbox, G, B, A, NC, assign, npos, acc, out, dcls, dreg, 1.0, 0, anyb)
        torch.cuda.synchronize()                # (the only synchronisation: after the last launch)
        nb = nbox.cpu().tolist()
        return {"cnt": [p["cnt"].cpu().numpy() for p in per], "rows": [[p["rows"][b, :int(p["cnt"][b])].cpu().numpy() for b in range(B)] for p in per],
                "nbox": nb, "boxes": [boxes[b, :nb[b]].cpu().numpy() for b in range(B)], "loss": out.cpu().numpy(),
                "dcls": dcls.cpu().numpy(), "dreg": dreg.cpu().numpy(), "overflow": int(ovf.item()), "any": int(anyb.item())}

    first = run()
    arena.check()
    assert first["overflow"] == 0 and first["any"] == 1
    for t in range(3):
        for b in range(B):
            eq(first["rows"][t][b], r6(gts[t][b]), ("teacher", t, "image", b))
    for b in range(B):
        eq(first["boxes"][b], r5(merged[b]), ("merged image", b))
    np.testing.assert_allclose(first["loss"][0], rl.item(), rtol=2e-4, atol=1e-7)
    np.testing.assert_allclose(first["loss"][1], cl.item(), rtol=2e-4, atol=1e-7)
    assert np.abs(first["dcls"] - c2.grad.numpy()).max() <= 2e-3 * c2.grad.abs().max().item() + 1e-9
    assert np.abs(first["dreg"] - r2.grad.numpy()).max() <= 2e-3 * r2.grad.abs().max().item() + 1e-9
    second = run()                              # on what the first run left in every buffer
    arena.check()
    same(first, second, "second run on the same buffers")
