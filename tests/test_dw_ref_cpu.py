"""CPU checks of tests/dw_ref.py, the float64 references of the depthwise kernels (csrc/dwconv.hip):
  1. hand checks of the references: 1x1 maps, the asymmetric TF-SAME padding at stride 2, delta inputs, float64 autograd of F.conv2d and
     of the composed block swish(BN(conv(swish(BN(x))))) with a squeeze-excite gate;
  2. the tolerance constants K of dw_ref are calibrated here: the same formulas evaluated in fp32 torch on the CPU, on every (case, mode)
     the GPU test runs, stay within K / 4 of the float64 reference in units of 2^-24 * A (K = max(8, 4 * K32));
  3. DW_CASES reaches, by the copy of the host dispatch in dw_ref.route, every branch the GPU test exists for."""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

import dw_ref as R
from elt_ref import EPS

D, S32 = torch.float64, torch.float32
KS = [(3, 1), (5, 1), (3, 2), (5, 2)]


def within(got, ref, A, name, rtol=1e-12):
    got, ref = got.detach().double(), ref.detach().double()
    assert got.shape == ref.shape, name
    assert bool(((got - ref).abs() <= rtol * A + 1e-300).all()), "%s: worst %.3e of A" % (name, float(((got - ref).abs() / A.clamp_min(1e-300)).max()))
    assert bool((A >= ref.abs() * (1 - 1e-12)).all()), name + ": A below |value|"


# ------------------------------------------------------------------------------------------------ 1. hand checks
@pytest.mark.parametrize("k,s", KS)
def test_one_by_one_map_sees_the_centre_tap(k, s):
    g = R.rng(31, k, s)
    x, w, dy = (torch.randn(*sh, generator=g, dtype=D) for sh in ((2, 1, 1, 4), (k * k, 4), (2, 1, 1, 4)))
    c = (k // 2) * k + k // 2
    assert R.same_pad_lo(1, k, s) == (1, k // 2)
    y, A = R.conv(x, x.abs(), w, k, s)
    assert torch.equal(y, x * w[c]) and torch.equal(A, (x * w[c]).abs())
    dx, _ = R.conv_bwd_data(dy, dy.abs(), w, 1, 1, k, s)
    assert torch.equal(dx, dy * w[c])
    dw, _ = R.conv_bwd_weight(x, dy, k, s, torch.zeros(k * k, 4, dtype=D))
    want = torch.zeros(k * k, 4, dtype=D)
    want[c] = (x * dy).sum((0, 1, 2))
    assert torch.equal(dw, want)


def test_stride_two_pads_even_sizes_on_the_high_side_only():
    """n = 4, k = 3, s = 2: extra = 1, low 0, high 1; n = 5: extra = 2, one each; k = 5: n = 4 -> extra 3 (1, 2), n = 5 -> extra 4 (2, 2)"""
    assert [R.same_pad_lo(n, 3, 2) for n in (4, 5)] == [(2, 0), (3, 1)]
    assert [R.same_pad_lo(n, 5, 2) for n in (4, 5)] == [(2, 1), (3, 2)]
    assert [R.same_pad_lo(n, 3, 1) for n in (4, 5)] == [(4, 1), (5, 1)]
    w = torch.tensor([0., 0, 0, 1, 10, 100, 0, 0, 0], dtype=D).view(9, 1).repeat(1, 4)      # only the middle tap row (i = 1; H = 1 pads one row above)
    x4 = torch.tensor([1., 2, 3, 4], dtype=D).view(1, 1, 4, 1).repeat(1, 1, 1, 4)
    x5 = torch.tensor([1., 2, 3, 4, 5], dtype=D).view(1, 1, 5, 1).repeat(1, 1, 1, 4)
    y4, _ = R.conv(x4, x4.abs(), w, 3, 2)
    y5, _ = R.conv(x5, x5.abs(), w, 3, 2)
    assert y4[0, 0, :, 0].tolist() == [321.0, 43.0]                    # windows (x0, x1, x2), (x2, x3, pad)
    assert y5[0, 0, :, 0].tolist() == [210.0, 432.0, 54.0]             # windows (pad, x0, x1), (x1, x2, x3), (x3, x4, pad)
    # the same along H (tap column j = 1)
    wh = torch.tensor([0., 1, 0, 0, 10, 0, 0, 100, 0], dtype=D).view(9, 1).repeat(1, 4)
    yh, _ = R.conv(x4.transpose(1, 2).contiguous(), x4.transpose(1, 2).abs().contiguous(), wh, 3, 2)
    assert yh[0, :, 0, 0].tolist() == [321.0, 43.0]
    # the input gradient scatters through the same windows
    dx4, _ = R.conv_bwd_data(torch.tensor([1., 2], dtype=D).view(1, 1, 2, 1).repeat(1, 1, 1, 4), torch.ones(1, 1, 2, 4, dtype=D), w, 1, 4, 3, 2)
    assert dx4[0, 0, :, 0].tolist() == [1.0, 10.0, 102.0, 20.0]


@pytest.mark.parametrize("k,s", KS)
def test_delta_inputs_reproduce_the_taps(k, s):
    """forward: a delta at (h0, w0) puts tap (i, j) at output (h0 + pad_t - i, w0 + pad_l - j) for stride 1 - the taps, flipped about the
    centre; input gradient: a delta in dy at (oh, ow) puts tap (i, j) at input (oh*s + i - pad_t, ow*s + j - pad_l) - the taps as stored."""
    C, H, W = 4, 11, 12
    g = R.rng(32, k, s)
    w = torch.randn(k * k, C, generator=g, dtype=D)
    (OH, pt), (OW, pl) = R.same_pad_lo(H, k, s), R.same_pad_lo(W, k, s)
    oh0, ow0 = 2, 3
    dy = torch.zeros(1, OH, OW, C, dtype=D); dy[0, oh0, ow0] = 1
    dx, _ = R.conv_bwd_data(dy, dy.abs(), w, H, W, k, s)
    want = torch.zeros(1, H, W, C, dtype=D)
    for i in range(k):
        for j in range(k):
            want[0, oh0 * s + i - pt, ow0 * s + j - pl] = w[i * k + j]
    assert torch.equal(dx, want)
    h0, w0 = 6, 6
    x = torch.zeros(1, H, W, C, dtype=D); x[0, h0, w0] = 1
    y, _ = R.conv(x, x.abs(), w, k, s)
    want = torch.zeros(1, OH, OW, C, dtype=D)
    for i in range(k):
        for j in range(k):
            nh, nw = h0 + pt - i, w0 + pl - j
            if nh % s == 0 and nw % s == 0:
                want[0, nh // s, nw // s] = w[i * k + j]
    assert torch.equal(y, want) and int((want != 0).sum()) >= C * ((k + s - 1) // s) ** 2 - C * k


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _conv2d(a_nhwc, w, k, s):
    """F.conv2d with the explicit TF-SAME padding, NHWC in and out, taps [k*k, C]"""
    C = w.shape[1]
    ap = R._padded(a_nhwc, k, s)[0]
    return F.conv2d(_nchw(ap), w.t().reshape(C, 1, k, k), stride=s, groups=C).permute(0, 2, 3, 1)


@pytest.mark.parametrize("k,s", KS)
@pytest.mark.parametrize("B,H,W,C", [(2, 7, 6, 8), (1, 4, 9, 4), (3, 1, 2, 4)])
def test_conv_references_match_float64_autograd(k, s, B, H, W, C):
    g = R.rng(33, k, s, H, W)
    x = torch.randn(B, H, W, C, generator=g, dtype=D).requires_grad_(True)
    w = torch.randn(k * k, C, generator=g, dtype=D).requires_grad_(True)
    y = _conv2d(x, w, k, s)
    dy = torch.randn(y.shape, generator=g, dtype=D)
    y.backward(dy)
    xd, wd = x.detach(), w.detach()
    yr, A = R.conv(xd, xd.abs(), wd, k, s)
    within(yr, y, A, "conv")
    dx, A = R.conv_bwd_data(dy, dy.abs(), wd, H, W, k, s)
    within(dx, x.grad, A, "input gradient")
    dw0 = torch.randn(k * k, C, generator=g, dtype=D)
    dw, A = R.conv_bwd_weight(xd, dy, k, s, dw0)
    within(dw - dw0, w.grad, A, "weight gradient")


@pytest.mark.parametrize("k,s", KS)
def test_block_references_match_float64_autograd(k, s):
    """z0 -> BN0 (batch statistics) -> swish -> depthwise conv -> z1 -> BN1 -> swish -> * gate[img, c], plus a pooled term add[img, c] on the
    activation: the forward sums, the `bz` sums, the weight gradient riding on the input gradient and (stride 1) the BatchNorm-1 backward in the
    prologue, against autograd."""
    B, H, W, C = 3, 6, 7, 8
    g = R.rng(34, k, s)
    rn = lambda *sh: torch.randn(*sh, generator=g, dtype=D)
    z0 = (rn(B, H, W, C) * 1.5 + 0.3).requires_grad_(True)
    w = (rn(k * k, C) / k).requires_grad_(True)
    ga0, be0, ga1, be1 = ((torch.rand(C, generator=g, dtype=D) + 0.5).requires_grad_(True), (rn(C) * 0.2).requires_grad_(True),
                          (torch.rand(C, generator=g, dtype=D) + 0.5).requires_grad_(True), (rn(C) * 0.2).requires_grad_(True))
    bn = lambda z, ga, be: F.batch_norm(z.reshape(-1, C), None, None, ga, be, True, 0.0, EPS).view(z.shape)
    a0 = R.swish(bn(z0, ga0, be0)); a0.retain_grad()
    z1 = _conv2d(a0, w, k, s); z1.retain_grad()
    a1 = R.swish(bn(z1, ga1, be1))
    gate, add, g1 = torch.rand(B, 1, 1, C, generator=g, dtype=D), rn(B, 1, 1, C) * 0.1, rn(*z1.shape)
    ((a1 * gate * g1).sum() + (a1 * add).sum()).backward()
    z0d, z1d, wd = z0.detach(), z1.detach(), w.detach()
    st = lambda z: torch.cat([z.sum((0, 1, 2)), (z * z).sum((0, 1, 2))])
    c0, _ = R.bn_finalize(st(z0d), B * H * W, ga0.detach(), be0.detach())
    c1, _ = R.bn_finalize(st(z1d), z1d.numel() // C, ga1.detach(), be1.detach())
    zero2, zero_w = torch.zeros(2 * C, dtype=D), torch.zeros(k * k, C, dtype=D)
    # forward with the producer transform and the raw sums
    o = R.dw_fwd(z0d, wd, k, s, c0["scale"], c0["shift"], None, 1, stats0=zero2)
    within(o["y"][0], z1, o["y"][1], "z1")
    within(o["stats"][0], st(z1d), o["stats"][1], "forward sums")
    # input gradient with the `bz` sums of BN0 and the weight gradient
    bn0 = (z0d, c0["scale"], c0["shift"], c0["mean"], c0["invstd"])
    b = R.dw_bwd_data(z1.grad, wd, H, W, k, s, bn0, zero2, zero_w)
    within(b["dx"][0], a0.grad, b["dx"][1], "dx")
    within(b["bn_sums"][0], torch.cat([be0.grad, ga0.grad]), b["bn_sums"][1], "bz sums = [dbeta0, dgamma0]")
    within(b["dw_grad"][0], w.grad, b["dw_grad"][1], "dw_grad")
    wg = R.dw_bwd_weight(z0d, z1.grad, k, s, zero_w, c0["scale"], c0["shift"], 1)
    within(wg[0], w.grad, wg[1], "bwd_weight")
    if s == 1:
        q_sums = torch.cat([be1.grad, ga1.grad])
        pre = torch.full((C,), 0.75, dtype=D)
        q = R.dw_bwd_data_bn1(g1, z1d, wd, k, c1["scale"], c1["shift"], c1["mean"], c1["invstd"], q_sums, B * H * W, gate.view(B, C),
                              add.view(B, C), bn0, zero2, zero_w, pre, -pre)
        within(q["dx"][0], a0.grad, q["dx"][1], "bn1 dx")
        within(q["bn_sums"][0], torch.cat([be0.grad, ga0.grad]), q["bn_sums"][1], "bn1 bz sums")
        within(q["dw_grad"][0], w.grad, q["dw_grad"][1], "bn1 dw_grad")
        within(q["q_dgamma"][0] - pre, ga1.grad, q["q_dgamma"][1], "q_dgamma accumulates")
        within(q["q_dbeta"][0] + pre, be1.grad, q["q_dbeta"][1], "q_dbeta accumulates")


def test_pool_reference_is_the_mean_of_the_stored_output():
    g = R.rng(35)
    x, w = torch.randn(2, 5, 6, 8, generator=g, dtype=D), torch.randn(9, 8, generator=g, dtype=D)
    osc, osh = torch.rand(8, generator=g, dtype=D) + 0.5, torch.randn(8, generator=g, dtype=D)
    p0 = torch.randn(2, 8, generator=g, dtype=D)
    o = R.dw_fwd(x, w, 3, 1, osc=osc, osh=osh, out_act=1, pool0=p0, nblocks=3)
    yy = R.swish(_conv2d(x, w, 3, 1) * osc + osh)
    within(o["y"][0], yy, o["y"][1], "folded epilogue")
    assert bool(((o["pool"][0] - p0 - yy.mean((1, 2))).abs() <= 1e-7 * o["pool"][1]).all())      # (pool_scale is the fp32 1 / 30)
    assert bool((o["pool"][1] >= p0.abs() + 3 / R.Q36).all())


# ------------------------------------------------------------------------------------------------ 2. calibration of K
@functools.lru_cache(maxsize=None)
def _k32():
    """K32 per family over every (case, mode) of DW_CASES and the group cases, and where each family's worst sits"""
    k32 = {f: (0.0, "") for f in R.K_BY_FAMILY}

    def take(fam, name, r64, r32):
        for out in r64:
            f = fam(out)
            r = R.ratio(r32[out][0], r64[out][0], r64[out][1])
            if r > k32[f][0]:
                k32[f] = (r, "%s %s" % (name, out))

    for case in R.DW_CASES:
        inp = R.case_inputs(case)
        for mode in case["modes"]:
            take(lambda o: R.FAMILY[(case["entry"], o)], "%s %s" % (case["name"], R.mode_label(mode)), R.case_ref(case, mode, inp, D),
                 R.case_ref(case, mode, inp, S32))
    for name, shape, k, s, pro, _ in R.GROUP_CASES:
        inp = R.group_inputs(shape, k, s)
        take(lambda o: R.FAMILY[("fwd", o)], name, R.group_ref(shape, k, s, pro, inp, D), R.group_ref(shape, k, s, pro, inp, S32))
    return k32


@pytest.mark.parametrize("family", sorted(R.K_BY_FAMILY))
def test_fp32_cpu_evaluation_is_within_a_quarter_of_K(family):
    """K = max(8, 4 * K32): the constant in dw_ref is the one this measurement gives, and the fp32 CPU run stays within K / 4"""
    k32, where = _k32()[family]
    K = R.K_BY_FAMILY[family]
    print("K32 %-10s %.3f  (K %.1f)  worst at %s" % (family, k32, K, where))
    assert k32 <= K / 4
    assert K == 8.0 or K <= 4 * k32 * 1.25 + 1, "K is larger than max(8, 4 * K32) calls for"
    assert abs(R.K32[family] - k32) <= 0.05 * k32 + 0.01, "the K32 recorded in dw_ref.py is not the one measured"


# ------------------------------------------------------------------------------------------------ 3. coverage
def test_no_dispatch_override_in_the_environment():
    """MMD_DW_LANES, MMD_DW_ROWS, MMD_DW_ROWS_RH, MMD_DW_ROWS_PYR, MMD_DW_NOSWZ change the dispatch that dw_ref.route copies"""
    assert not [k for k in os.environ if k.startswith("MMD_DW_")]


def _recs():
    return [(c, m, R.route_mode(c, m)) for c in R.DW_CASES for m in c["modes"]]


def _has(recs, entry=None, **want):
    def ok(c, m, r):
        if entry and c["entry"] != entry:
            return False
        for key, v in want.items():
            got = r.get(key, c.get(key)) if key not in ("H", "pro", "epi", "kind") else None
            if key == "H":
                got = c["shape"][1]
            elif key == "pro":
                got = m[0] if c["entry"] == "fwd" else None
            elif key == "kind":
                got = m[0] if c["entry"] == "bwd_data" else None
            if callable(v):
                if not v(got):
                    return False
            elif got != v:
                return False
        return True
    return any(ok(*x) for x in recs)


def test_cases_reach_every_branch():
    recs = _recs()
    has = functools.partial(_has, recs)
    missing = []

    def need(what, **kw):
        if not has(**kw):
            missing.append(what)

    # rows kernel, rh > 4
    for rh, epi, last in ((5, 0, 1), (6, 1, None), (7, 3, None), (9, 1, None)):
        need("rows R1 rh %d EPI %d" % (rh, epi), entry="fwd", kernel="dw3_rows", R=1, LW=16, PRO=0, EPI=epi, rh=rh,
             **({"last_rows": last} if last else {}))
    need("rows R2 rh 5 ragged", entry="fwd", kernel="dw3_rows", R=2, rh=5, last_chunk_quads=lambda q: q < 16)
    need("rows flipped EPI 2 rh 6", entry="bwd_data", kernel="dw3_rows", EPI=2, rh=6)
    need("rows flipped EPI 0 rh 5", entry="bwd_data", kernel="dw3_rows", EPI=0, rh=5)
    for pro in ("given", "live"):
        need("rows R4 LW16 PRO rh 5 " + pro, entry="fwd", kernel="dw3_rows", R=4, LW=16, PRO=1, EPI=1, rh=5, pro=pro)
    need("wgrad rows rh 5", entry="bwd_weight", kernel="dw3_wgrad_rows", rh=5, last_rows=1, PRO=1)
    # rows kernel, other edges
    for H in (1, 2, 3):
        for epi in (0, 1, 3):
            need("rows rh = H = %d EPI %d" % (H, epi), entry="fwd", kernel="dw3_rows", rh=H, H=H, EPI=epi)
    need("rows R4 rh = H = 3", kernel="dw3_rows", R=4, rh=3, colblocks=2)
    need("rows PRO rh = H < 4", kernel="dw3_rows", PRO=1, rh=2)
    for name, kern, geo in (("w15", "dw_fwd", {"LANES": 16}), ("w16", "dw3_rows", {"R": 1}), ("w31", "dw3_rows", {"R": 1, "colblocks": 2}),
                            ("w32", "dw3_rows", {"R": 2}), ("w63", "dw3_rows", {"R": 2, "colblocks": 2}), ("w64", "dw3_rows", {"R": 4}),
                            ("w63_pro", "dw_fwd", {"PRO": 1}), ("w127_c24", "dw_fwd", {"LANES": 8}), ("w128_c24", "dw3_rows", {"R": 4, "LW": 8}),
                            ("w255_c12", "dw_fwd", {"LANES": 4}), ("w256_c12", "dw3_rows", {"R": 4, "LW": 4}),
                            ("c144_pro", "dw_fwd", {"PRO": 1}), ("c128_pro", "dw3_rows", {"PRO": 1, "R": 4}),
                            ("lw8_ragged", "dw3_rows", {"LW": 8, "colblocks": 2}), ("lw4_ragged", "dw3_rows", {"LW": 4, "colblocks": 2})):
        for m in R.CASE[name]["modes"]:
            r = R.route_mode(R.CASE[name], m)
            if r["kernel"] != kern or any(r[k_] != v for k_, v in geo.items()):
                missing.append("%s %s -> %s" % (name, m, r))
    for lw in (4, 8, 16):
        need("rows LW %d PRO 1 EPI 3" % lw, kernel="dw3_rows", LW=lw, PRO=1, EPI=3)
    # tile kernel: PRO x EPI for every (K, S, LANES), each with given and with live coefficients
    for K, S, L in ((3, 1, 4), (3, 1, 8), (3, 1, 16), (5, 1, 16), (3, 2, 16), (5, 2, 16)):
        for epi in (0, 1, 3, 4):
            for pro in ("none", "given", "live"):
                need("tile <%d,%d,%d> %s EPI %d" % (K, S, L, pro, epi), entry="fwd", kernel="dw_fwd", K=K, S=S, LANES=L, EPI=epi, pro=pro,
                     PRO=int(pro != "none"))
    need("tile 1x1 map", entry="fwd", kernel="dw_fwd", tiles=1, H=1)
    need("tile C = 144 with a producer", entry="fwd", kernel="dw_fwd", K=3, S=1, PRO=1, cchunks=3, tiles=lambda t: t > 20)
    need("tile slotted sums EPI 1", entry="fwd", kernel="dw_fwd", slotted=True, EPI=1)
    need("tile slotted sums EPI 4", entry="fwd", kernel="dw_fwd", slotted=True, EPI=4)
    for K in (3, 5):
        need("tile flipped WG k%d" % K, entry="bwd_data", kernel="dw_fwd", K=K, EPI=2, WG=True, PRO=0)
        need("tile flipped EPI 2 k%d" % K, entry="bwd_data", kernel="dw_fwd", K=K, EPI=2, WG=False)
        need("tile flipped EPI 0 k%d" % K, entry="bwd_data", kernel="dw_fwd", K=K, EPI=0)
        need("bn1 k%d" % K, entry="bn1", kernel="dw_fwd", K=K, PRO=2, EPI=2, WG=True, LANES=16)
    for L in (4, 8, 16):
        need("tile flipped WG LANES %d" % L, entry="bwd_data", kernel="dw_fwd", K=3, LANES=L, WG=True)
    need("tile flipped slotted", entry="bwd_data", kernel="dw_fwd", slotted=True, WG=True)
    need("bn1 last chunk one quad", entry="bn1", last_chunk_quads=1)
    # stride-2 input gradient
    for K in (3, 5):
        need("s2 rpb 4 k%d" % K, kernel="s2_sums", K=K, rpb=4, rbl=33, last_rows=2, rpb_clamped=False, WG=True)
        need("s2 rpb 4 k%d no WG" % K, kernel="s2_sums", K=K, rpb=4, WG=False)
        need("s2 rpb > H = 1 k%d" % K, kernel="s2_sums", K=K, rpb=2, rpb_clamped=True, H=1)
        need("s2 plain k%d" % K, kernel="s2_plain", K=K)
        need("s2 odd H last block one row k%d" % K, kernel="s2_sums", K=K, last_rows=1, rbl=2)
    need("s2 rpb 4 > H = 3", kernel="s2_sums", rpb=4, rpb_clamped=True, H=3)
    need("s2 slotted", kernel="s2_sums", slotted=True, WG=False)
    need("s2 slotted WG", kernel="s2_sums", slotted=True, WG=True)
    need("s2 last chunk one quad", kernel="s2_sums", last_chunk_quads=1)
    # weight gradient
    for K, S in KS:
        for pro in (0, 1):
            need("wgrad <%d,%d> PRO %d" % (K, S, pro), kernel="dw_wgrad", K=K, S=S, PRO=pro)
    need("wgrad nsplit = ntiles", kernel="dw_wgrad", clamp="ntiles")
    need("wgrad nsplit < ntiles", kernel="dw_wgrad", clamp="blocks", nsplit=lambda n: n > 1)
    need("wgrad last chunk one quad", kernel="dw_wgrad", last_chunk_quads=1)
    for lw in (4, 8):
        for pro in (0, 1):
            need("wgrad rows LW %d PRO %d" % (lw, pro), kernel="dw3_wgrad_rows", LW=lw, PRO=pro)
    # one-quad last chunks and more than one block everywhere
    need("rows last chunk one quad", kernel="dw3_rows", last_chunk_quads=1, cchunks=2)
    need("tile last chunk one quad", entry="fwd", kernel="dw_fwd", last_chunk_quads=1, cchunks=2)
    assert not missing, missing
    # only the rh > 4 cases run the loop body of the rows kernels a second time: there w0..w3 and za / zb come back in rotated roles, and
    # the row the first trip's last step loads (`issue_row(oh + 5, w2)`, `issue_z(oh + 4, za)`) is consumed for the first time.  (The
    # step before it, `issue_row(oh + 4, w1)`, feeds the fourth row of the SAME trip: every block of four rows runs it.)
    rolling = sorted({c["name"] for c, m, r in recs if r["kernel"] in ("dw3_rows", "dw3_wgrad_rows") and r["rh"] > 4})
    assert rolling == sorted(["rows_r1_rh5", "rows_r1_rh6", "rows_r1_rh7", "rows_r1_rh9", "rows_r2_rh5", "rows_bwd_rh6", "rows_bwd_rh5",
                              "rows_r4_pro_rh5", "wgrad_rows_rh5"])
    # the slotted cases really are over MMD_STATS_DEPTH, and nothing else asks for slots
    for c, m, r in recs:
        slots = m[-1] if isinstance(m, tuple) else 0
        assert bool(slots) == bool(r.get("slotted")), (c["name"], m, r)
    # group mode
    for name, shape, k, s, pro, _ in R.GROUP_CASES:
        assert shape[0] == R.GROUP_N * R.GROUP_IMAGES
    assert R.route("fwd", *R.GROUP_CASES[0][1], 3, 1, out=True)["kernel"] == "dw3_rows"
    assert R.route("fwd", *R.GROUP_CASES[1][1], 5, 2, pro=True, out=True)["kernel"] == "dw_fwd"


def test_route_matches_the_geometry_the_issue_derived():
    """spot values worked out by hand from dwconv.hip"""
    r = R.route("fwd", 2, 67, 64, 144, 3, 1)                       # test_dwconv's largest rows shape: 67 * 6 / 1024 = 0 -> rh 4
    assert (r["kernel"], r["R"], r["rh"], r["rowblocks"], r["last_rows"]) == ("dw3_rows", 4, 4, 17, 3)
    r = R.route("bwd_data", 8, 128, 128, 144, 3, 1)                # the benchmarked step: cchunks 3, colblocks 2 -> rh 6
    assert (r["cchunks"], r["colblocks"], r["rh"]) == (3, 2, 6)
    assert R.route("fwd", 8, 256, 256, 64, 3, 1)["rh"] == 8
    assert R.route("fwd", 2, 256, 256, 16, 3, 1, sums=True, ws_slots=8)["kernel"] == "dw3_rows"      # test_slotted_bn_sums_match_direct
    r = R.route("bwd_data", 9, 130, 6, 256, 3, 2, bn=True)
    assert (r["rpb"], r["rbl"], r["last_rows"]) == (4, 33, 2)
    assert R.route("bwd_weight", 64, 9, 9, 2048, 3, 2)["nsplit"] == 1
