"""GPU: the weighted box fusion kernel (csrc/postproc.hip pp_wbf_kernel through postproc.wbf_merge) against its float32 restatement bit for
bit - boxes, counts, the per-box record and the overflow flag - on cases built to reach every path of the rule; against the float64
restatement on seeded random scenes; and through DistillEngine with cfg label_merge = wbf."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import wbf_ref as R
from mm_distillnet_amd.postproc import wbf_merge

DEV = "cuda"
F = np.float32
NONE = np.zeros((0, 6), F)


def rows(*r):
    return np.array(r, dtype=F).reshape(-1, 6)


class DirtyArena:
    """hands out buffers full of NaN (floats) or of a number no count can be (integers): the kernel must write whatever is read later"""

    def alloc(self, shape, dtype=torch.float32):
        return torch.full(tuple(shape), float("nan") if dtype.is_floating_point else -7777, dtype=dtype, device=DEV)


def pack(srcs, B, cap, cnt_add=0):
    """srcs[s][b] [n, 6] -> per source (rows [B, cap, 6], cnt [B]) on the device; the rows behind a count hold garbage (NaN, huge and
    negative boxes with the best scores: nothing may read them); cnt_add is added to the counts of full images (clamped by the kernel)"""
    out_r, out_c = [], []
    for s in srcs:
        r = np.empty((B, cap, 6), F)
        r[:, :, 0::2] = np.nan; r[:, :, 1] = -3e38; r[:, :, 3] = 3e38; r[:, :, 4] = 9.0; r[:, :, 5] = 0.0
        c = np.zeros(B, np.int32)
        for b in range(B):
            a = np.asarray(s[b], F).reshape(-1, 6)
            assert len(a) <= cap
            r[b, :len(a)] = a
            c[b] = len(a) + (cnt_add if len(a) == cap else 0)
        out_r.append(torch.from_numpy(r).to(DEV)); out_c.append(torch.from_numpy(c).to(DEV))
    return out_r, out_c


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def fuse(srcs, B, cap, thr=0.5, inclusive=False, maxg=None, min_votes=1, merge01=False, cnt_add=0):
    """the kernel on srcs -> (boxes [b] [k, 5], aux [b] [k, 3], overflow flag); checks that nothing behind the counts was written"""
    r, c = pack(srcs, B, cap, cnt_add)
    G = maxg if maxg is not None else len(srcs) * cap * (2 if merge01 else 1)
    ovf = torch.zeros(1, dtype=torch.int32, device=DEV)
    boxes, nbox, aux = wbf_merge(DirtyArena(), r, c, B, cap, thr, inclusive, G, min_votes, ovf, merge01=merge01)
    torch.cuda.synchronize()
    nb = nbox.cpu().numpy()
    assert nb.min() >= 0 and nb.max() <= G, nb
    bx, ax = boxes.cpu().numpy(), aux.cpu().numpy()
    for b in range(B):
        assert np.isnan(bx[b, nb[b]:]).all() and np.isnan(ax[b, nb[b]:]).all()
    return [bx[b, :nb[b]] for b in range(B)], [ax[b, :nb[b]] for b in range(B)], int(ovf.item())


def check(srcs, B, cap, thr=0.5, inclusive=False, maxg=None, min_votes=1, merge01=False, cnt_add=0, overflow=False):
    """kernel == wbf_f32, bit for bit; -> the reference's result"""
    ref = R.wbf_f32(srcs, B, thr, inclusive, merge01, min_votes, maxg)
    bx, ax, ovf = fuse(srcs, B, cap, thr, inclusive, maxg, min_votes, merge01, cnt_add)
    assert ovf == int(ref.overflow) == int(overflow)
    for b in range(B):
        assert bx[b].shape == ref.boxes[b].shape, (b, bx[b].shape, ref.boxes[b].shape)
        assert np.array_equal(bits(bx[b]), bits(ref.boxes[b])), (b, bx[b], ref.boxes[b])
        assert np.array_equal(bits(ax[b]), bits(ref.aux[b])), (b, ax[b], ref.aux[b])
    return ref


@pytest.mark.parametrize("nsrc", [1, 2, 3, 4])
def test_every_source_empty(nsrc):
    ref = check([[NONE] * 3 for _ in range(nsrc)], 3, 8, merge01=bool(nsrc % 2))
    assert [len(b) for b in ref.boxes] == [0, 0, 0]


@pytest.mark.parametrize("nsrc,cap", [(1, 16), (3, 16), (4, 33)])
def test_one_source_only(nsrc, cap):
    """the rows of one source, alone or among empty ones: what overlaps within it still fuses, with one vote"""
    one = R.draw_scene(np.random.default_rng(11), 3, 1)[0]
    one[1] = np.concatenate([one[1], one[1][:3] + F([1, 1, 1, 1, -0.01, 0])])          # a sure overlap
    srcs = [[NONE] * 3 for _ in range(nsrc)]
    srcs[nsrc - 1] = one
    ref = check(srcs, 3, cap)
    assert all((a[:, 2] == 1).all() for a in ref.aux) and max(a[:, 1].max() for a in ref.aux if len(a)) >= 2


def test_three_sources_nearly_identical_boxes():
    base = rows([10, 20, 110, 220, 0.9, 1], [300, 300, 400, 380, 0.8, 0], [5, 400, 60, 500, 0.7, 1])
    rng = np.random.default_rng(5)
    srcs = []
    for s in range(3):
        a = base.copy()
        a[:, :4] += rng.uniform(-1e-3, 1e-3, (3, 4)).astype(F)
        a[:, 4] -= F(0.01 * s)
        srcs.append([a, a[::-1].copy(), a[:2].copy()])
    ref = check(srcs, 3, 8)
    assert [a[:, 1:].tolist() for a in ref.aux] == [[[3, 3]] * 3, [[3, 3]] * 3, [[3, 3]] * 2]
    check(srcs, 3, 8, min_votes=3)


def test_equal_scores_index_order_decides():
    """four overlapping boxes of one score: the walk takes them in gather order (source, then row), and each order fuses differently"""
    a, b, c, d = [0, 0, 10, 10, 0.5, 0], [3, 0, 13, 10, 0.5, 0], [6, 0, 16, 10, 0.5, 0], [9, 0, 19, 10, 0.5, 0]
    r1 = check([[rows(a, b), rows(b, c), rows(a)], [rows(c, d), rows(a, d), rows(a)]], 3, 8)
    assert r1.members[0] == [[0, 1], [2, 3]] and r1.members[1] == [[0, 1], [2], [3]]
    assert r1.boxes[0][:, 0].tolist() == [1.5, 7.5] and r1.boxes[1][:, 0].tolist() == [4.5, 0, 9]


def test_two_labels_overlapping_do_not_fuse():
    a = rows([10, 10, 60, 60, 0.9, 0], [100, 100, 180, 160, 0.6, 1])
    b = rows([11, 10, 61, 60, 0.8, 1], [101, 100, 181, 160, 0.5, 1])
    ref = check([[a, a, b], [b, b, a]], 3, 8)
    assert ref.aux[0][:, 1].tolist() == [1, 1, 2] and ref.boxes[0][:, 4].tolist() == [0, 1, 1]


def test_chain_and_its_mirror():
    """A + B fuse to about (21.4, 0, 31.4, 10).  C reaches IoU 0.38 with A alone and 0.53 with the fused box: it joins only because the box
    moved.  D reaches 0.504 with A alone and 0.36 with the fused box: it stays out only because the box moved."""
    A, Bx = [20, 0, 30, 10, 0.9, 0], [23, 0, 33, 10, 0.8, 0]
    C, D = [24.5, 0, 34.5, 10, 0.3, 0], [16.7, 0, 26.7, 10, 0.3, 0]
    ref = check([[rows(A), rows(A), rows(A), rows(A)], [rows(Bx, C), rows(C), rows(Bx, D), rows(D)]], 4, 8)
    assert ref.members == [[[0, 1, 2]], [[0], [1]], [[0, 1], [2]], [[0, 1]]]


@pytest.mark.parametrize("lo,hi", [(2, 68), (5, 69), (10, 65), (0, 64), (63, 127)])
def test_tie_between_clusters_in_different_lanes(lo, hi):
    """130 lone clusters of one label; a last box overlaps clusters `lo` and `hi` at IoU 0.25 exactly (scores k / 256 and small integer
    coordinates keep every lone fused box (w x) / w exact).  The clusters sit in different lanes of the walk, or in one lane's stride -
    (10, 65): the lower cluster in the HIGHER lane - and the lower index must win."""
    n = 130
    a = np.zeros((n + 1, 6), F)
    for j in range(n):
        a[j] = [20 * j, 100, 20 * j + 4, 104, (256 - j) / 256, 3]
    a[lo, :4] = [0, 0, 4, 4]; a[hi, :4] = [6, 0, 10, 4]
    a[n] = [2, 0, 8, 4, 0.25, 3]
    perm = np.random.default_rng(lo).permutation(n + 1)
    srcs = [[a[perm[:64]], NONE, NONE], [a[perm[64:128]], NONE, NONE], [a[perm[128:]], NONE, NONE]]
    ref = check(srcs, 3, 64, thr=0.2)
    assert [len(m) for m in ref.members[0]] == [2 if j == lo else 1 for j in range(n)]
    assert ref.boxes[0][hi, :4].tolist() == [6, 0, 10, 4]


@pytest.mark.parametrize("inclusive", [0, 1])
def test_integer_boxes_at_iou_exactly_half(inclusive):
    a, b = rows([0, 0, 4, 4, 0.5, 0], [8, 8, 16, 12, 0.25, 1]), rows([0, 0, 4, 2, 0.25, 0], [8, 8, 16, 16, 0.5, 1])
    ref = check([[a, a, NONE], [b, NONE, b]], 3, 8, thr=0.5, inclusive=bool(inclusive))
    assert [len(x) for x in ref.boxes] == ([2, 2, 2] if inclusive else [4, 2, 2])


@pytest.mark.parametrize("fill", ["image0_empty", "image1_empty", "both"])
@pytest.mark.parametrize("B", [2, 3])
def test_merge01(fill, B):
    sc = R.draw_scene(np.random.default_rng(21), 3, 3)
    for s in sc:
        s[0] = np.concatenate([s[0], rows([40, 40, 90, 90, 0.95, 1])])
        s[1] = np.concatenate([s[1], rows([42, 41, 91, 92, 0.9, 1])])          # fuses with image 0's box, and with its own source bit
        if fill == "image0_empty":
            s[0] = NONE
        if fill == "image1_empty":
            s[1] = NONE
    srcs = [s[:B] for s in sc]
    cap = max(len(x) for s in srcs for x in s)
    plain = check(srcs, B, cap)
    ref = check(srcs, B, cap, merge01=True)
    assert (len(ref.boxes[1]) != len(plain.boxes[1])) == (fill == "both")
    assert all(np.array_equal(ref.boxes[b], plain.boxes[b]) for b in range(B) if b != 1)
    if fill == "both":
        assert ref.aux[1][:, 1].max() >= 6 and check(srcs, B, cap, merge01=True, min_votes=3).aux[1][:, 2].min() == 3


@pytest.mark.parametrize("votes", [1, 2, 3])
def test_min_votes(votes):
    srcs, _ = R.clear_scene(31, 3, 3, 0.5)
    cap = max(len(x) for s in srcs for x in s)
    ref = check(srcs, 3, cap, min_votes=votes)
    assert all((a[:, 2] >= votes).all() for a in ref.aux)
    n = sum(len(a) for a in ref.aux)
    assert 0 < n and (votes == 1 or n < sum(len(a) for a in R.wbf_f32(srcs, 3, 0.5).aux))


def test_maxg_too_small_keeps_the_first_clusters():
    srcs, _ = R.clear_scene(32, 3, 3, 0.5)
    cap = max(len(x) for s in srcs for x in s)
    full = check(srcs, 3, cap)
    g = max(len(b) for b in full.boxes) - 2
    assert g >= 1
    cut = check(srcs, 3, cap, maxg=g, overflow=True)
    assert all(np.array_equal(c, f[:g]) for c, f in zip(cut.boxes, full.boxes))
    check(srcs, 3, cap, maxg=g + 2)          # exactly enough: no flag


def test_1024_rows_fit_and_1025_set_the_flag():
    """image 0: 1024 rows in three sources (the full LDS carve, no flag); image 1: 1025 (the flag, and the fusion of the first 1024 in
    gather order: the last row of the last source takes no part); image 2: a count above cap, clamped.  16 labels and boxes that overlap
    their neighbours, so that clusters grow while a thousand rows go by."""
    cap = 352
    rng = np.random.default_rng(41)

    def image(n):
        a = np.zeros((n, 6), F)
        x = rng.uniform(0, 100, n); y = rng.uniform(0, 100, n)
        a[:, 0] = x; a[:, 1] = y; a[:, 2] = x + rng.uniform(24, 32, n); a[:, 3] = y + rng.uniform(24, 32, n)
        a[:, 4] = rng.uniform(0.3, 1, n); a[:, 5] = rng.integers(0, 16, n)
        return a
    i0, i1, i2 = image(1024), image(1025), image(cap + 30)
    srcs = [[i0[:352], i1[:352], i2[:352]], [i0[352:704], i1[352:704], i2[352:372]], [i0[704:], i1[704:], i2[372:]]]
    bx, ax, ovf = fuse(srcs, 3, cap, cnt_add=5)
    ref = R.wbf_f32(srcs, 3)
    assert ovf == 1 and ref.overflow
    assert R.wbf_f32([[s[1][:-1] if k == 2 else s[1]] for k, s in enumerate(srcs)], 1).boxes[0].tobytes() == ref.boxes[1].tobytes()
    for b in range(3):
        assert np.array_equal(bits(bx[b]), bits(ref.boxes[b])) and np.array_equal(bits(ax[b]), bits(ref.aux[b])), b
    assert max(a[:, 1].max() for a in ref.aux) >= 3
    # without image 1 the flag stays down
    keep = [[s[0], s[2]] for s in srcs]
    assert fuse(keep, 2, cap, cnt_add=5)[2] == 0


@pytest.mark.parametrize("seed,nsrc,thr,inclusive,merge01", [(1, 3, 0.5, False, False), (2, 4, 0.55, True, True), (3, 2, 0.4, False, True),
                                                             (4, 1, 0.5, False, False), (5, 3, 0.6, False, False)])
def test_kernel_against_float64_on_random_scenes(seed, nsrc, thr, inclusive, merge01):
    """Seeded scenes at S = 512 in which every decision of the float64 run lies more than 1e-3 from its boundary (the generator redraws
    until one does: tests/wbf_ref.py clear_scene).  Membership: the kernel equals wbf_f32 bit for bit, whose clusters hold the rows the
    float64 run put there, and the kernel's own member and source counts equal float64's.  Coordinates: within (2 m + 6) 2^-24 S of
    float64's for a cluster of m members."""
    S, B = 512.0, 3
    srcs, ref = R.clear_scene(seed, B, nsrc, thr, inclusive, merge01, S)
    cap = max(8, max(len(x) for s in srcs for x in s))
    r32 = check(srcs, B, cap, thr, inclusive, merge01=merge01)
    assert r32.members == ref.members
    bx, ax, _ = fuse(srcs, B, cap, thr, inclusive, merge01=merge01)
    worst = 0.0
    for b in range(B):
        assert np.array_equal(bx[b][:, 4], ref.boxes[b][:, 4]) and np.array_equal(ax[b][:, 1:], ref.aux[b][:, 1:])
        for k, m in enumerate(ref.members[b]):
            err = np.abs(bx[b][k, :4].astype(np.float64) - ref.boxes[b][k, :4]).max()
            worst = max(worst, err / R.coordinate_bound(len(m), S))
            assert err <= R.coordinate_bound(len(m), S), (b, k, len(m), err)
    print("largest coordinate error: %.3f of the bound" % worst)


# ---------------------------------------------------------------- through the engine
OBJECTS = {0: [((10, 12, 40, 44), 1, (0.9, 0.88, 0.86)), ((60, 8, 100, 50), 0, (0.7, 0.68, None)), ((20, 70, 70, 120), 1, (None, 0.5, None))],
           1: [((64, 64, 120, 118), 0, (0.8, None, 0.78)), ((5, 5, 50, 50), 1, (0.6, 0.58, 0.56))]}


def injected_rows():
    """per teacher and image [n, 6]: every object's box seen by some of the three teachers, moved by a fraction of a pixel; objects
    pairwise disjoint, and their score bands strictly descending, so that the fused boxes come out in object order"""
    rng = np.random.default_rng(7)
    per = [[[], []] for _ in range(3)]
    for b, objs in OBJECTS.items():
        for box, lb, scores in objs:
            for t, sc in enumerate(scores):
                if sc is not None:
                    per[t][b].append(list(np.array(box) + rng.uniform(-0.5, 0.5, 4)) + [sc, lb])
    return [[np.array(r, F).reshape(-1, 6) for r in t] for t in per]


def test_engine_label_merge_wbf():
    from mm_distillnet_amd.step import DistillEngine, StepConfig
    from mm_distillnet_amd.synth import synth_inputs
    from helpers import make_state
    S, B = 128, 2
    mods = {"rgb": (3, 21), "depth": (3, 22), "thermal": (1, 23)}
    teachers = {k: make_state(2, cin, seed, k, cls_bias=-2.0) for k, (cin, seed) in mods.items()}
    spec_s, st_s = make_state(2, 8, 24, "audio")

    def engine(**kw):
        e = DistillEngine(spec_s, {k: v[0] for k, v in teachers.items()}, DEV, StepConfig(image_size=S, **kw))
        e.load(st_s, {k: v[1] for k, v in teachers.items()})
        return e
    eng_w, eng_n = engine(label_merge="wbf"), engine()
    batch = {k: v.to(DEV) for k, v in synth_inputs(B, S, seed=5).items()}
    ds = eng_w.make_drop_scale(B, torch.Generator(device=DEV).manual_seed(1))
    A = eng_w.student.anchors(S).shape[0]
    per = injected_rows()
    ref = R.wbf_f32(per, B, 0.5)
    assert [a[:, 1].tolist() for a in ref.aux] == [[3, 2, 1], [2, 3]]
    labels = eng_w.labels_from_rows(per, A)

    def same_as_ref(boxes, nbox, aux):
        torch.cuda.synchronize()
        nb = nbox.cpu().tolist()
        assert nb == [len(x) for x in ref.boxes]
        for b in range(B):
            assert np.array_equal(bits(boxes[b, :nb[b]].cpu().numpy()), bits(ref.boxes[b]))
            assert np.array_equal(bits(aux[b, :nb[b]].cpu().numpy()), bits(ref.aux[b]))

    # (a) the merge alone, eager
    same_as_ref(*eng_w.merge_labels([r for r, _ in labels], [c for _, c in labels]))
    # (c) a wbf step against an nms step that is handed the fused boxes as its first teacher's rows (disjoint, scores descending: the NMS
    # keeps all of them in this order); tolerance: test_gpu_step.py test_graph_replay_matches_eager, two runs of one step
    fused = [[np.concatenate([ref.boxes[b][:, :4], (0.9 - 0.1 * np.arange(len(ref.boxes[b]), dtype=F))[:, None], ref.boxes[b][:, 4:]], 1)
              for b in range(B)], [NONE] * B, [NONE] * B]
    ow = eng_w.step_body(batch, ds, teacher_labels=labels)
    on = eng_n.step_body(batch, ds, teacher_labels=eng_n.labels_from_rows(fused, A))
    torch.cuda.synchronize()
    eng_w.check_overflow(); eng_n.check_overflow()
    same_as_ref(ow["boxes"], ow["nbox"], ow["label_aux"])
    assert on["label_aux"] is None and on["nbox"].tolist() == ow["nbox"].tolist()
    for b in range(B):
        assert torch.equal(on["boxes"][b, :len(ref.boxes[b])], ow["boxes"][b, :len(ref.boxes[b])])
    for k in ("reg", "cls", "kd"):
        print(k, ow[k].cpu().numpy(), on[k].cpu().numpy())
        np.testing.assert_allclose(ow[k].cpu().numpy(), on[k].cpu().numpy(), rtol=1e-4, atol=1e-6)
    # (a) again, from the captured step
    eng_w.capture(batch, teacher_labels=labels)
    oc = eng_w.replay(batch, ds)
    same_as_ref(oc["boxes"], oc["nbox"], oc["label_aux"])
    eng_w.check_overflow()
