"""CPU checks of tests/mb_ref.py, the float64 references of the frozen MBConv front half (csrc/mbconv_fused.hip), the fused expand backward
(csrc/mbconv_bwd_fused.hip) and the stem kernels (mmd_stem_conv_fwd, mmd_stem_conv_bwd_weight(_bn), mmd_stem_im2col):
  1. every reference against an independently written torch composite in float64 - F.conv2d (1x1, groups = C over an explicitly zero-padded
     activated map, 3x3 / stride 2), F.silu, F.batch_norm(training = True), F.unfold - and the backward references against autograd of that
     composite, to 1e-12 relative;
  2. mb_ref.route over the case tables reaches every instantiation and every edge the issue lists (written out here);
  3. the conditions on the inputs (|shift0| of order 3, BatchNorm-1 all negative, strides, several images inside one tile);
  4. the tolerance constants K are calibrated here: the same formulas in fp32 on the CPU stay within K / 4 (K = max(8, 4 * K32))."""
import functools
import math
import os

import pytest
import torch
import torch.nn.functional as F

import mb_ref as R
from elt_ref import EPS, bn_finalize

D, S32 = torch.float64, torch.float32


def within(got, ref, A, name, rtol=1e-12):
    got, ref, A = got.detach().double(), ref.detach().double(), A.detach().double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(((got - ref).abs() <= rtol * A + 1e-300).all()), "%s: worst %.3e of A" % (name, float(((got - ref).abs() / A.clamp_min(1e-300)).max()))
    assert bool((A >= got.abs() * (1 - 1e-9)).all()), name + ": A below |value|"


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def pad_same(x, k, s):
    """explicit TF-SAME zero padding of an NCHW map: low side extra // 2, the rest on the high side"""
    H, W = x.shape[2:]
    eh, ew = max(0, (-(-H // s) - 1) * s - H + k), max(0, (-(-W // s) - 1) * s - W + k)
    return F.pad(x, (ew // 2, ew - ew // 2, eh // 2, eh - eh // 2))


# ------------------------------------------------------------------------------------------------ 1. references against torch: mbx
def mbx_torch(x, w0, sc0, sh0, wd, sc1, sh1, k, s):
    C, Cin = w0.shape
    v = lambda t: t.view(1, -1, 1, 1)
    e = F.silu(F.conv2d(nchw(x), w0.view(C, Cin, 1, 1)) * v(sc0) + v(sh0))
    c = F.conv2d(pad_same(e, k, s), wd.t().reshape(C, 1, k, k), stride=s, groups=C)
    y = F.silu(c * v(sc1) + v(sh1))
    return nhwc(y), y.mean((2, 3))


@pytest.mark.parametrize("name", [c["name"] for c in R.MBX_CASES])
def test_mbx_reference_matches_the_torch_composite(name):
    c = R.MBX[name]
    d = R._to(R.mbx_inputs(c), D, "cpu")
    ref = R.mbx_case_ref(c, R.mbx_inputs(c), D)
    y, pm = mbx_torch(d["x"], d["w0"], d["sc0"], d["sh0"], d["wd"], d["sc1"], d["sh1"], c["k"], c["s"])
    within(ref["y"][0], y, ref["y"][1], name + " y")
    within(ref["pool"][0], d["pool0"].double() / R.Q36 + pm, ref["pool"][1], name + " pool", 1e-7)          # (pool_scale is the C float 1 / (OH OW))
    assert "pool" not in R.mbx_case_ref(c, R.mbx_inputs(c), D, pool=False)
    assert ref["y"][0].shape[1:3] == R.mbx_route_of(c)["out"]


@pytest.mark.parametrize("name", [c["name"] for c in R.MBX_GROUP_CASES])
def test_mbx_grouped_reference_reads_each_nets_parameters(name):
    c = R.MBX[name]
    inp = R.mbx_inputs(c)
    d = R._to(inp, D, "cpu")
    ref = R.mbx_case_ref(c, inp, D)
    Cin, C, k, ws, bs = c["Cin"], c["Cmid"], c["k"], d["w_stride"], d["bn_stride"]
    assert ws % 4 == 0 and ws >= max(C * Cin, k * k * C)
    for b in range(c["B"]):
        gi = b // R.GROUP_IMAGES
        bn = lambda key: d[key][gi * bs:gi * bs + C]
        y, pm = mbx_torch(d["x"][b:b + 1], d["w0"][gi * ws:gi * ws + C * Cin].view(C, Cin), bn("sc0"), bn("sh0"),
                          d["wd"][gi * ws:gi * ws + k * k * C].view(k * k, C), bn("sc1"), bn("sh1"), k, c["s"])
        within(ref["y"][0][b:b + 1], y, ref["y"][1][b:b + 1], "%s image %d" % (name, b))
        within(ref["pool"][0][b:b + 1], d["pool0"][b:b + 1].double() / R.Q36 + pm, ref["pool"][1][b:b + 1], "%s image %d pool" % (name, b), 1e-7)
    assert not torch.equal(d["wd"][:k * k * C], d["wd"][ws:ws + k * k * C])


def test_mbx_input_conditions():
    c = R.MBX["shift0_3"]
    d = R._to(R.mbx_inputs(c), D, "cpu")
    assert bool((d["sh0"].abs() >= 3).all())
    halo = F.silu(d["sh0"])                                   # what a kernel that activates the padding would convolve
    assert float(halo.abs().max()) > 2.5
    c = R.MBX["bn1_negative"]
    d = R._to(R.mbx_inputs(c), D, "cpu")
    e = F.silu((d["x"] @ d["w0"].t()) * d["sc0"] + d["sh0"])
    u = R.conv(e, e.abs(), d["wd"], c["k"], c["s"])[0] * d["sc1"] + d["sh1"]
    assert bool((u < 0).all())
    pads = {(c["k"], c["s"]): set() for c in R.MBX_CASES}
    for c in R.MBX_CASES:
        pads[(c["k"], c["s"])].update(R.mbx_route_of(c)["pad"])
    assert pads[(3, 2)] >= {0, 1}                             # even and odd sizes at stride 2


# ------------------------------------------------------------------------------------------------ 1. mbw
def mbw_direct(c, d, sums):
    """the contract written out with plain ops (no helper of elt_ref / wg_ref / bd_ref)"""
    C, M = c["Cmid"], c["M"]
    m1, m2 = sums[:C] / d["count"], sums[C:] / d["count"]
    u = d["z0"] * d["scale"] + d["shift"]
    sg = torch.sigmoid(u)
    gp = d["g0"] * (sg * (1 + u * (1 - sg)))
    dz = d["scale"] * (gp - m1 - (d["z0"] - d["mean"]) * d["invstd"] * m2)
    out = {"dx": dz @ d["w"] + (d["res"] if c["res"] != "none" else 0), "dw": d["dw0"] + torch.einsum("mc,mk->ck", dz, d["x"])}
    if c["dsum"]:
        out["dgamma"], out["dbeta"] = d["dgamma0"] + sums[C:], d["dbeta0"] + sums[:C]
    if c["xs"] != "off":
        s = d["xs0"].clone()
        for m in range(0, M, R.XS_RPI):
            rows = slice(m, min(M, m + R.XS_RPI))
            gq = out["dx"][rows] * (d["xs_mul_b"][m // R.XS_RPI] if c["xs"] == "mulb" else 1.0)
            s[:c["Cin"]] += gq.sum(0)
            s[c["Cin"]:] += (gq * (d["xs_z"][rows] - d["xs_mean"]) * d["xs_invstd"]).sum(0)
        out["xs_sums"] = s
    return out


@pytest.mark.parametrize("name", [c["name"] for c in R.MBW_CASES if c["M"] <= 1001])
def test_mbw_reference_matches_the_contract_written_out(name):
    c = R.MBW[name]
    d = R._to(R.mbw_inputs(c), D, "cpu")
    sums = R.mbw_case_sums(d)
    ref, want = R.mbw_case_ref(c, d, sums), mbw_direct(c, d, sums)
    assert set(ref) == set(want)
    for k, (v, A) in ref.items():
        within(v, want[k], A, "%s %s" % (name, k), 1e-11)
    assert d["count"] != c["M"]


@pytest.mark.parametrize("Cin", sorted(R.MBW_PAIRS))
def test_mbw_reference_matches_autograd_through_the_batchnorm(Cin):
    """x -> z0 = x . w^T -> train-mode BatchNorm -> swish, the loss <out, g0> + <x, residual>: dx, dw, dgamma, dbeta against autograd (eps is
    the C float the library uses; 1e-10: the statistics' own cancellation)"""
    C, M = R.MBW_PAIRS[Cin][0], 70
    g = R.rng(71, Cin)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=D)
    x, w = rn(M, Cin).requires_grad_(True), (rn(C, Cin) / math.sqrt(Cin)).requires_grad_(True)
    gamma, beta = (torch.rand(C, generator=g, dtype=D) + 0.5).requires_grad_(True), (rn(C) * 0.2).requires_grad_(True)
    g0, res = rn(M, C), rn(M, Cin)
    z0 = x @ w.t()
    out = F.silu(F.batch_norm(z0, None, None, gamma, beta, True, 0.0, EPS))
    ((out * g0).sum() + (x * res).sum()).backward()
    zz = z0.detach()
    v, _ = bn_finalize(torch.cat([zz.sum(0), (zz * zz).sum(0)]), M, gamma.detach(), beta.detach())
    sums = R.mbw_sums(g0, zz, v["scale"], v["shift"], v["mean"], v["invstd"])
    z = torch.zeros
    ref = R.mbw_ref(g0, zz, x.detach(), w.detach(), v["scale"], v["shift"], v["mean"], v["invstd"], sums, M, z(C, Cin, dtype=D), res, z(C, dtype=D),
                    z(C, dtype=D))
    for k, want in (("dx", x.grad), ("dw", w.grad), ("dgamma", gamma.grad), ("dbeta", beta.grad)):
        within(ref[k][0], want, ref[k][1], "Cin %d %s" % (Cin, k), 1e-10)


# ------------------------------------------------------------------------------------------------ 1. stem
def stem_torch(x, w, Cin):
    Cout = w.shape[0]
    return F.conv2d(pad_same(x, 3, 2), w[:, :9 * Cin].reshape(Cout, Cin, 3, 3), stride=2)


@pytest.mark.parametrize("name", [c["name"] for c in R.STEM_FWD_CASES if c["slots"] == 0])
def test_stem_forward_reference_matches_conv2d(name):
    c = R.STEM_FWD[name]
    inp = R.stem_fwd_inputs(c)
    d = R._to(inp, D, "cpu")
    raw = nhwc(stem_torch(d["x"], d["w"], c["Cin"])).reshape(-1, c["Cout"])
    for mode in R.STEM_FWD_MODES:
        ref = R.stem_fwd_case_ref(c, mode, inp, D)
        if mode == "stats":
            within(ref["y"][0], raw, ref["y"][1], name + " raw")
            within(ref["stats"][0], d["stats0"] + torch.cat([raw.sum(0), (raw * raw).sum(0)]), ref["stats"][1], name + " stats")
        else:
            t = raw * d["osc"] + d["osh"]
            within(ref["y"][0], F.silu(t) if mode == "fold1" else t, ref["y"][1], "%s %s" % (name, mode))
    if c["Kp"] > 9 * c["Cin"]:
        assert bool((d["w"][:, 9 * c["Cin"]:] != 0).any())          # the weight's padding columns hold values: the operand's are zero


@pytest.mark.parametrize("B,Cin,H,W,Kp", R.IM2COL_CASES)
def test_im2col_reference_matches_unfold(B, Cin, H, W, Kp):
    x = torch.randn(B, Cin, H, W, generator=R.rng(72, B, Cin, H, W), dtype=D)
    col = R.stem_im2col_ref(x, Kp)
    want = F.unfold(pad_same(x, 3, 2), 3, stride=2).transpose(1, 2).reshape(-1, 9 * Cin)
    assert torch.equal(col[:, :9 * Cin], want) and bool((col[:, 9 * Cin:] == 0).all()) and col.shape[1] == Kp


@pytest.mark.parametrize("name", [c["name"] for c in R.STEM_WG_CASES if c["H"] <= 16])
def test_stem_wgrad_reference_matches_autograd(name):
    """plain: autograd of the conv with the case's dz; _bn: the operand BnBwd(g, z) written out, sent through the same autograd"""
    c = R.STEM_WG[name]
    d = R._to(R.stem_wg_inputs(c), D, "cpu")
    Cin, Cout, Kp = c["Cin"], c["Cout"], c["Kp"]
    for mode in c["modes"]:
        w = torch.zeros(Cout, Kp, dtype=D, requires_grad=True)
        y = nhwc(stem_torch(d["x"], w, Cin)).reshape(-1, Cout)
        sums = None
        up = d["dz"]
        if mode != "plain":
            act = R.stem_wg_act(mode)
            sums = R.stem_wg_case_sums(d, act)
            u = d["z"] * d["scale"] + d["shift"]
            sg = torch.sigmoid(u)
            gp = d["dz"] * (sg * (1 + u * (1 - sg))) if act else d["dz"]
            up = d["scale"] * (gp - sums[:Cout] / d["count"] - (d["z"] - d["mean"]) * d["invstd"] * sums[Cout:] / d["count"])
        (y * up).sum().backward()
        ref = R.stem_wg_case_ref(c, mode, d, sums)
        within(ref["dw"][0], d["dw0"] + w.grad, ref["dw"][1], "%s %s dw" % (name, mode), 1e-11)
        assert torch.equal(ref["dw"][0][:, 9 * Cin:], d["dw0"][:, 9 * Cin:])          # the padding columns receive exactly 0
        assert ("dgamma" in ref) == (mode in ("bn0", "bn1"))
        if "dgamma" in ref:
            within(ref["dgamma"][0], d["dgamma0"] + sums[Cout:], ref["dgamma"][1], name + " dgamma")
            within(ref["dbeta"][0], d["dbeta0"] + sums[:Cout], ref["dbeta"][1], name + " dbeta")


@pytest.mark.parametrize("act", [0, 1])
def test_stem_wgrad_bn_reference_matches_autograd_through_the_batchnorm(act):
    B, Cin, H, W, Cout = 2, 3, 5, 6, 8
    g = R.rng(73, act)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=D)
    x, w = rn(B, Cin, H, W), (rn(Cout, 28) / 5).requires_grad_(True)
    gamma, beta = (torch.rand(Cout, generator=g, dtype=D) + 0.5).requires_grad_(True), (rn(Cout) * 0.2).requires_grad_(True)
    z = nhwc(stem_torch(x, w, Cin)).reshape(-1, Cout)
    M = z.shape[0]
    out = F.batch_norm(z, None, None, gamma, beta, True, 0.0, EPS)
    out = F.silu(out) if act else out
    gy = rn(M, Cout)
    (out * gy).sum().backward()
    zz = z.detach()
    v, _ = bn_finalize(torch.cat([zz.sum(0), (zz * zz).sum(0)]), M, gamma.detach(), beta.detach())
    d = {"dz": gy, "z": zz, **v}
    sums = R.stem_wg_case_sums(d, act)
    zero = torch.zeros
    bn = {"z": zz, **v, "sums": sums, "count": M, "act": act, "mul_b": None, "rpi": 1, "dgamma0": zero(Cout, dtype=D), "dbeta0": zero(Cout, dtype=D)}
    ref = R.stem_wgrad_ref(x, gy, 28, zero(Cout, 28, dtype=D), bn)
    within(ref["dw"][0][:, :27], w.grad[:, :27], ref["dw"][1][:, :27], "dw", 1e-10)
    within(ref["dgamma"][0], gamma.grad, ref["dgamma"][1], "dgamma", 1e-10)
    within(ref["dbeta"][0], beta.grad, ref["dbeta"][1], "dbeta", 1e-10)


# ------------------------------------------------------------------------------------------------ 2. route coverage
def test_no_dispatch_override_in_the_environment():
    """MMD_MBW_TM32 / MMD_MBW_GRID change the dispatch that mb_ref.mbw_route copies (out of scope); MMD_STEM_DIRECT and MMD_STEM_WG_BLOCKS are
    followed by route"""
    assert not [k for k in os.environ if k in ("MMD_MBW_TM32", "MMD_MBW_GRID")]


def test_mbx_cases_reach_every_instantiation_and_edge():
    rs = {c["name"]: R.route("mbx", c["B"], c["H"], c["W"], c["Cin"], c["Cmid"], c["k"], c["s"]) for c in R.MBX_CASES}
    assert {r["inst"] for r in rs.values()} == {(nk, k, s) for nk in (4, 6, 8, 10, 12, 14) for k in (3, 5) for s in (1, 2)}
    edge = [c for c in R.MBX_CASES if not c["name"].startswith("lat_")]          # the edges do not lean on the lattice
    for ks in R.MBX_KS:
        assert {rs[c["name"]]["vec"] for c in edge if (c["k"], c["s"]) == ks} == {2, 4}, ks
    assert {c["Cin"] for c in edge} == set(R.MBX_CINS)
    assert {(r["inst"][1:], r["PT"], r["TPW"]) for r in rs.values()} == {((3, 1), 21, 6), ((5, 1), 25, 7), ((3, 2), 19, 5), ((5, 2), 23, 6)}
    assert all(r["partial_last"] and r["tiles_per_block"] == 1 for r in rs.values())          # `tile >= PT` is taken in every instantiation
    assert 48 in {c["Cmid"] for c in edge} and max(c["Cmid"] for c in edge) >= 144
    grids = {r["grid"] for r in rs.values()}
    assert 1 in grids and any(1 < n < 8 for n in grids) and any(n > 8 and n % 8 for n in grids) and any(n >= 8 and n % 8 == 0 for n in grids)
    # map edges: H = 1, W = 1, exact tiles at both strides, ragged multi-tile maps in both directions
    assert any(c["H"] == 1 for c in edge) and any(c["W"] == 1 for c in edge)
    exact = {(c["s"], c["k"]) for c in edge if (c["H"], c["W"]) == (16, 16) and rs[c["name"]]["ragged"] == (False, False) and rs[c["name"]]["tiles"] == 1}
    assert exact >= {(1, 3), (2, 3), (2, 5)}
    assert {(c["H"], c["W"]) for c in edge if rs[c["name"]]["tiles_hw"][0] > 1 and rs[c["name"]]["tiles_hw"][1] > 1 and all(rs[c["name"]]["ragged"])} >= {(19, 35), (33, 17)}
    assert {c["kind"] for c in edge} >= {"shift3", "negu"}
    gs = [R.mbx_route_of(c) for c in R.MBX_GROUP_CASES]
    assert {c["s"] for c in R.MBX_GROUP_CASES} == {1, 2} and {r["vec"] for r in gs} == {2, 4} and all(c["B"] == 6 for c in R.MBX_GROUP_CASES)
    for Cin, Cmid, k, s in R.MBX_REFUSED:
        assert R.route("mbx", 2, 8, 8, Cin, Cmid, k, s) is None


def test_mbw_cases_reach_every_instantiation_and_edge():
    for Cin, (C, TM, cap) in R.MBW_PAIRS.items():
        cs = [c for c in R.MBW_CASES if c["Cin"] == Cin]
        rs = [R.route("mbw", c["M"], Cin, C) for c in cs]
        assert {r["inst"] for r in rs} == {(C, Cin, TM)}
        assert {c["M"] for c in cs} == {1, TM - 1, TM, TM + 1, 1000, cap * TM + TM + 7}
        assert {r["tiles_per_block"] for r in rs} == {1, 2}
        big = [r for r in rs if r["tiles_per_block"] == 2]
        assert all(r["grid"] == cap and r["ntiles"] == cap + 2 and r["row_tail"] == 7 for r in big)
        assert {c["res"] for c in cs} == {"none", "alias", "sep"} and {c["xs"] for c in cs} == {"off", "on", "mulb"} and {c["dsum"] for c in cs} == {True, False}
        assert any(c["xs"] == "mulb" and c["M"] >= 2 * R.XS_RPI for c in cs)
    assert R.XS_RPI % 32 and 64 % R.XS_RPI and R.XS_RPI < 64          # several images meet inside one tile
    assert {r["col_mask"] for r in (R.mbw_route(100, Cin, R.MBW_PAIRS[Cin][0]) for Cin in R.MBW_PAIRS)} == {True, False}
    assert [768 * 64 + 71, 512 * 64 + 71, 256 * 64 + 71, 256 * 32 + 39] == [R.MBW_PAIRS[k][2] * R.MBW_PAIRS[k][1] + R.MBW_PAIRS[k][1] + 7 for k in (16, 24, 32, 48)]
    assert R.route("mbw", 100, 16, 144) is None and R.route("mbw", 100, 40, 240) is None
    if os.environ.get("MMD_MBW48") is None:
        assert R.mbw_supported(48, 288) == 0
    assert R.mbw_supported(16, 96) == R.mbw_supported(24, 144) == R.mbw_supported(32, 192) == 1


def test_stem_forward_cases_reach_every_instantiation_and_edge():
    direct = os.environ.get("MMD_STEM_DIRECT") is not None
    rs = {c["name"]: R.stem_fwd_route_of(c, "stats") for c in R.STEM_FWD_CASES}
    assert all(r["kernel"] == ("direct" if direct else "gemm") for r in rs.values())
    assert {c["Cin"]: c["Kp"] for c in R.STEM_FWD_CASES} == {1: 12, 2: 20, 3: 28, 8: 72, 9: 84}
    assert {c["Cout"] for c in R.STEM_FWD_CASES} == {32, 40, 48, 56, 64}
    shapes = {(c["H"], c["W"]) for c in R.STEM_FWD_CASES}
    assert (2, 2) in shapes and (1, 1) in shapes and any(h != w and h % 2 and w % 2 for h, w in shapes) and any(h != w and not h % 2 and not w % 2 for h, w in shapes)
    slotted = [n for n, r in rs.items() if r["slotted"]]
    assert len(slotted) == 1 and rs[slotted[0]]["M"] == 16641
    if not direct:
        assert {c["Kp"]: rs[c["name"]]["nkl"] for c in R.STEM_FWD_CASES} == {12: 2, 20: 3, 28: 4, 72: 1, 84: 3}
        assert {r["inst"] for r in rs.values()} == {(128, 32, n, 2) for n in (1, 2, 3, 4)}
        assert {r["row_tail"] == 0 for r in rs.values()} == {True, False} and {r["col_tail"] for r in rs.values()} == {0, 8, 16, 24}
        assert rs[slotted[0]]["ntm"] == R.STATS_DEPTH + 3 and max(r["ksteps"] for r in rs.values()) == 3
    assert R.route("stem_fwd", 2, 3, 8, 8, 28, 36) is None and R.route("stem_fwd", 2, 3, 8, 8, 24, 32) is None
    assert R.route("stem_fwd", 2, 3, 8, 8, 28, 32, scale_shift=(True, False)) is None


def test_stem_wgrad_cases_reach_every_instantiation_and_edge():
    rs = {(c["name"], m): R.stem_wg_route_of(c, m) for c in R.STEM_WG_CASES for m in c["modes"]}
    assert all(r is not None for r in rs.values())
    assert {r["inst"] for r in rs.values()} == {(cot, bn) for cot in (1, 2, 3) for bn in (False, True)}
    assert {(r["COT"], r["narrow"]) for r in rs.values()} >= {(1, True), (2, True), (2, False), (3, True), (3, False)}
    assert {c["Cin"] for c in R.STEM_WG_CASES} == {1, 3, 8} and {c["Cout"] for c in R.STEM_WG_CASES} == {4, 20, 32, 36, 48}
    assert {c["W"] for c in R.STEM_WG_CASES} == {127, 128, 255, 256} and {(r["tpr"], r["pad"][1]) for r in rs.values()} == {(1, 1), (1, 0), (2, 1), (2, 0)}
    assert min(c["H"] for c in R.STEM_WG_CASES) == 2 and {c["H"] % 2 for c in R.STEM_WG_CASES} == {0, 1}
    assert any(c["Kp"] == 80 and c["Cin"] == 1 for c in R.STEM_WG_CASES) and {r["kpad"] for r in rs.values()} >= {0, 1, 3, 71}
    modes = {m for c in R.STEM_WG_CASES for m in c["modes"]}
    assert modes == {"plain", "bn0", "bn1", "bn1n"}
    if os.environ.get("MMD_STEM_WG_BLOCKS") is None:
        assert R.stem_wg_blocks() == 1024
        assert {r["slots"] for r in rs.values()} >= set(R.STEM_WG_SLOTS) | {1024}
        assert {r["tiles_per_block"] for r in rs.values()} == {1, 2}
        assert [R.fold_iters(n) for n in (1, 15, 16, 17, 48, 49, 64, 65, 113)] == [(0, 1), (0, 1), (0, 1), (0, 2), (0, 3), (1, 3), (1, 0), (1, 1), (2, 3)]
        assert R.fold_iters(1024) == (16, 0)
    else:
        assert all(r["slots"] <= R.stem_wg_blocks() for r in rs.values())
    want = {(3, 8, 126, 28, 32): 0, (3, 8, 127, 28, 32): 1, (3, 8, 128, 28, 32): 1, (3, 8, 129, 28, 32): 0, (0, 8, 128, 28, 32): 0, (8, 8, 128, 72, 32): 1,
            (9, 8, 128, 84, 32): 0, (3, 8, 128, 84, 32): 0, (3, 8, 128, 28, 0): 0, (3, 8, 128, 28, 48): 1, (3, 8, 128, 28, 52): 0, (3, 8, 128, 28, 6): 0,
            (3, 1, 128, 28, 32): 0, (3, 2, 128, 28, 32): 1}
    assert set(want) <= set(R.STEM_WG_EDGES)
    for k, v in want.items():
        assert R.stem_wg_supported(*k) == v, k


# ------------------------------------------------------------------------------------------------ 4. calibration of K
@functools.lru_cache(maxsize=None)
def _k32():
    """K32 per family and where each family's worst sits.  One thread: the fp32 summation order of torch's CPU reductions and matmul then does
    not depend on how many cores the machine offers"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _k32_measure()
    finally:
        torch.set_num_threads(threads)


def _k32_measure():
    k32 = {f: (0.0, "") for f in R.K_BY_FAMILY}

    def take(kind, label, r32, r64):
        assert set(r32) == set(r64)
        for out in r64:
            fam = R.FAMILY[(kind, out)]
            r = R.ratio(r32[out][0], r64[out][0], r64[out][1])
            if r > k32[fam][0]:
                k32[fam] = (r, "%s %s" % (label, out))
    for c in R.MBX_CASES + R.MBX_GROUP_CASES:
        inp = R.mbx_inputs(c)
        take("mbx", c["name"], R.mbx_case_ref(c, inp, S32), R.mbx_case_ref(c, inp, D))
    for c in R.MBW_CASES:
        inp = R.mbw_inputs(c)
        d64 = R._to(inp, D, "cpu")
        sums = R.mbw_case_sums(d64)
        take("mbw", c["name"], R.mbw_case_ref(c, R._to(inp, S32, "cpu"), sums), R.mbw_case_ref(c, d64, sums))
    for c in R.STEM_FWD_CASES:
        inp = R.stem_fwd_inputs(c)
        for mode in R.STEM_FWD_MODES:
            take("stem_fwd", "%s %s" % (c["name"], mode), R.stem_fwd_case_ref(c, mode, inp, S32), R.stem_fwd_case_ref(c, mode, inp, D))
    for c in R.STEM_WG_CASES:
        inp = R.stem_wg_inputs(c)
        d64, d32 = R._to(inp, D, "cpu"), R._to(inp, S32, "cpu")
        for mode in c["modes"]:
            sums = None if mode == "plain" else R.stem_wg_case_sums(d64, R.stem_wg_act(mode))
            take("stem_wg" if mode == "plain" else "stem_wg_bn", "%s %s" % (c["name"], mode), R.stem_wg_case_ref(c, mode, d32, sums),
                 R.stem_wg_case_ref(c, mode, d64, sums))
    return k32


@pytest.mark.parametrize("family", sorted(R.K_BY_FAMILY))
def test_fp32_cpu_evaluation_is_within_a_quarter_of_K(family):
    """K = max(8, 4 * K32): the constant in mb_ref is the one this measurement gives, and the fp32 CPU run stays within K / 4"""
    k32, where = _k32()[family]
    K = R.K_BY_FAMILY[family]
    print("K32 %-10s %.3f  (K %.1f)  worst at %s" % (family, k32, K, where))
    assert k32 <= K / 4
    assert K == float(max(8, math.ceil(4 * R.K32[family]))), "K is not max(8, 4 * K32) of the stored K32"
    assert abs(R.K32[family] - k32) <= 0.05 * k32 + 0.01, "the K32 recorded in mb_ref.py is not the one measured"
