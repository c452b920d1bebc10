"""CPU checks of tests/pyr_ref.py, the float64 references of the detection heads' pyramid launches:
  1. every reference in float64 against an independently written plain evaluation per level - F.conv2d(groups = C) and its autograd, the
     autograd of swish(BatchNorm(z)) with batch statistics, a plain matmul, an index loop for the gather - to 1e-11 of A;
  2. the pyramid helper against mmd_make_pyr's arithmetic;
  3. pyr_ref.route_dw and pw_ref.route(pyr=True) over PYR_CASES reach every route and rider combination the issue names (written out here);
  4. no dispatch variable is set;
  5. the tolerance constants K are calibrated here: the fp32 models stay within K / 4, K = max(8, ceil(4 * K32)), and the K32 recorded in
     pyr_ref.py is the one measured."""
import functools
import math
import os

import pytest
import torch
import torch.nn.functional as F

import pyr_ref as R
from elt_ref import EPS, swish

D, S32 = torch.float64, torch.float32


def within(got, ref, A, name, rtol=1e-11):
    got, ref, A = got.detach().double(), ref.detach().double(), A.detach().double()
    assert got.shape == ref.shape == A.shape, (name, got.shape, ref.shape, A.shape)
    assert bool(((got - ref).abs() <= rtol * A + 1e-300).all()), "%s: worst %.3e of A" % (name, float(((got - ref).abs() / A.clamp_min(1e-300)).max()))
    assert bool((A >= got.abs() * (1 - 1e-9)).all()), name + ": A below |value|"


def nchw(t, B, H, W):
    return t.reshape(B, H, W, -1).permute(0, 3, 1, 2).contiguous()


def rows_of(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def conv_t(a, w):
    C = a.shape[1]
    return F.conv2d(a, w.t().reshape(C, 1, 3, 3), padding=1, groups=C)


def bn_train(x, gamma, beta, cdim):
    """train-mode BatchNorm written out (F.batch_norm refuses a level of one element per channel): biased variance, eps 1e-3"""
    dims = [i for i in range(x.dim()) if i != cdim]
    shape = [1] * x.dim()
    shape[cdim] = -1
    mean, var = x.mean(dims, keepdim=True), x.var(dims, unbiased=False, keepdim=True)
    return (x - mean) / torch.sqrt(var + EPS) * gamma.view(shape) + beta.view(shape)


def sl(t, o, l, ls, C):
    return t[o + l * ls:o + l * ls + C]


# ------------------------------------------------------------------------------------------------ 1. references against plain evaluations
@pytest.mark.parametrize("name", R.cases_of("dw"))
def test_depthwise_references_match_conv2d_and_its_autograd(name):
    case = R.CASE[name]
    d = R.case_inputs(case)
    P, C, ls, o = R.pyr_of(case["pyr"]), case["C"], d["ls"], d["o"]
    ref = {m: R.case_ref(case, m, d, D) for m in R.DW_MODES}
    w = d["w"].double()
    dwp = dwq = 0
    for l, (H, W) in enumerate(P.sizes):
        x, dy = nchw(R.lvl(d["x"], P, l).double(), P.B, H, W), nchw(R.lvl(d["dy"], P, l).double(), P.B, H, W)
        sc, sh = (sl(d[k].double(), o, l, ls, C).view(1, C, 1, 1) for k in ("scale", "shift"))
        within(ref["fwd_plain"]["y"][l][0], rows_of(conv_t(x, w)), ref["fwd_plain"]["y"][l][1], name + " plain")
        within(ref["fwd_given"]["y"][l][0], rows_of(conv_t(swish(x * sc + sh), w)), ref["fwd_given"]["y"][l][1], name + " given")
        bn = bn_train(x, sl(d["gamma"].double(), o, l, ls, C), sl(d["beta"].double(), o, l, ls, C), 1)
        within(ref["fwd_live"]["y"][l][0], rows_of(conv_t(swish(bn), w)), ref["fwd_live"]["y"][l][1], name + " live level %d" % l, 1e-9)
        # flip 1 and the riders: autograd of conv(f(x)) with upstream dy
        for mode, f in (("bwd_wg_plain", lambda t: t), ("bwd_wg_bn", lambda t: swish(t * sc + sh))):
            a = f(x).detach().requires_grad_(True)
            ww = w.clone().requires_grad_(True)
            conv_t(a, ww).backward(dy)
            within(ref[mode]["y"][l][0], rows_of(a.grad), ref[mode]["y"][l][1], "%s %s dx" % (name, mode))
            if mode == "bwd_wg_plain":
                dwp = dwp + ww.grad
                within(ref["bwd_plain"]["y"][l][0], rows_of(a.grad), ref["bwd_plain"]["y"][l][1], name + " flipped")
            else:
                dwq = dwq + ww.grad
                # the sums of the BatchNorm(+swish) backward that consumes the flipped launch's output: g = dx * swish'(u)
                u = (x * sc + sh).detach().requires_grad_(True)
                swish(u).backward(a.grad)
                g = rows_of(u.grad)
                xh = (R.lvl(d["x"], P, l).double() - sl(d["mean"].double(), o, l, ls, C)) * sl(d["invstd"].double(), o, l, ls, C)
                want = d["sums0"][2 * (o + l * ls):2 * (o + l * ls) + 2 * C] + torch.cat([g.sum(0), (g * xh).sum(0)])
                within(ref[mode]["bn_sums"][l][0], want, ref[mode]["bn_sums"][l][1], name + " bn_sums")
    within(ref["bwd_wg_plain"]["dw_grad"][0], d["dw0"].double() + dwp, ref["bwd_wg_plain"]["dw_grad"][1], name + " dw_grad plain")
    for m in ("bwd_wg_pro", "bwd_wg_bn"):
        within(ref[m]["dw_grad"][0], d["dw0"].double() + dwq, ref[m]["dw_grad"][1], name + " dw_grad " + m)
    assert "bn_sums" not in ref["bwd_wg_pro"] and "dw_grad" not in ref["bwd_plain"]


@pytest.mark.parametrize("name", R.cases_of("wg"))
def test_weight_gradient_reference_matches_autograd(name):
    case = R.CASE[name]
    d = R.case_inputs(case)
    P, C, ls, o = R.pyr_of(case["pyr"]), case["C"], d["ls"], d["o"]
    for mode in R.WG_MODES:
        tot = 0
        for l, (H, W) in enumerate(P.sizes):
            x, dy = nchw(R.lvl(d["x"], P, l).double(), P.B, H, W), nchw(R.lvl(d["dy"], P, l).double(), P.B, H, W)
            if mode == "pro":
                x = swish(x * sl(d["scale"].double(), o, l, ls, C).view(1, C, 1, 1) + sl(d["shift"].double(), o, l, ls, C).view(1, C, 1, 1))
            ww = d["w"].double().requires_grad_(True)
            conv_t(x, ww).backward(dy)
            tot = tot + ww.grad
        v, A = R.case_ref(case, mode, d, D)["dw"]
        within(v, d["dw0"].double() + tot, A, "%s %s" % (name, mode))


@pytest.mark.parametrize("name", [n for n in R.cases_of("pw") if R.CASE[n]["pyr"] != "big"] + R.cases_of("gpw"))
def test_gemm_references_match_matmul(name):
    case = R.CASE[name]
    d = R.case_inputs(case)
    P, K, N, ls, o = R.pyr_of(case["pyr"]), case["C"], case["N"], d["ls"], d["o"]
    ref = R.case_ref(case, False, d, D)
    for l, (H, W) in enumerate(P.sizes):
        x = R.lvl(d["x"], P, l).double()
        if case["entry"] == "gpw":
            ws, per = d["w_stride"], R.GROUP_IMAGES * H * W
            raw = torch.cat([x[g * per:(g + 1) * per] @ d["w_buf"].double()[g * ws:g * ws + N * K].view(N, K).t() + d["bias_buf"].double()[g * ws:g * ws + N]
                             for g in range(R.GROUP_N)])
            within(ref["y"][l][0], raw, ref["y"][l][1], name)
            continue
        raw = x @ d["w"].double().t() + (d["bias"].double() if case["bias"] else 0)
        within(ref["y"][l][0], torch.sigmoid(raw) if case["act"] == 2 else raw, ref["y"][l][1], name + " y")
        if case["stats"]:
            s0 = d["stats0"][2 * (o + l * ls):2 * (o + l * ls) + 2 * N]
            within(ref["sum"][l][0], s0[:N] + raw.sum(0), ref["sum"][l][1], name + " sum")
            within(ref["sumsq"][l][0], s0[N:] + (raw * raw).sum(0), ref["sumsq"][l][1], name + " sumsq")
        else:
            assert "sum" not in ref
    if case["entry"] == "pw":
        # the strided head output: every level's block lies inside an image's stride, no two elements share a position
        idx = torch.cat([R.head_index(P, l, N, d["bstride"], d["yoff"]).reshape(-1) for l in range(P.n)])
        assert idx.unique().numel() == idx.numel() == sum(P.rows) * N and int(idx.max()) < P.B * d["bstride"]


@pytest.mark.parametrize("name", R.cases_of("red"))
def test_batchnorm_backward_references_match_autograd_of_swish_bn(name):
    """y = swish(BN(z)) with batch statistics per level (written out, train mode): reduce's g and sums, then apply's dz and dgamma / dbeta from
    those sums, are autograd's; then the case's own (arbitrary) coefficients against the written-out formulas"""
    case = R.CASE[name]
    d = R.case_inputs(case)
    P, C, ls, o = R.pyr_of(case["pyr"]), case["C"], d["ls"], d["o"]
    na = o + P.n * ls
    z, gy = d["x"].double(), d["dy"].double()
    gamma, beta = d["gamma"].double(), d["beta"].double()
    coef = {k: torch.zeros(na, dtype=D) for k in ("scale", "shift", "mean", "invstd")}
    for l in range(P.n):
        v, _ = R.bn_finalize(d["stats"][2 * (o + l * ls):2 * (o + l * ls) + 2 * C], P.rows[l], sl(gamma, o, l, ls, C), sl(beta, o, l, ls, C))
        for k in coef:
            coef[k][o + l * ls:o + l * ls + C] = v[k]
    zero2 = torch.zeros(2 * na, dtype=D)
    red = R.bn_reduce_pyr(P, C, gy, z, coef["scale"][o:], coef["shift"][o:], coef["mean"][o:], coef["invstd"][o:], 1, ls, zero2[2 * o:])
    sums = torch.zeros(2 * na, dtype=D)
    for l in range(P.n):
        sums[2 * (o + l * ls):2 * (o + l * ls) + 2 * C] = red["sums"][l][0]
    zero = torch.zeros(na, dtype=D)
    app = R.bn_apply_pyr(P, C, gy, z, coef["mean"][o:], coef["invstd"][o:], gamma[o:], sums[2 * o:], ls, zero[o:], zero[o:], coef["scale"][o:],
                         coef["shift"][o:], 1)
    for l in range(P.n):
        zl = R.lvl(z, P, l).clone().requires_grad_(True)
        ga, be = sl(gamma, o, l, ls, C).clone().requires_grad_(True), sl(beta, o, l, ls, C).clone().requires_grad_(True)
        u = bn_train(zl, ga, be, 1)
        u.retain_grad()
        swish(u).backward(R.lvl(gy, P, l))
        within(red["g"][l][0], u.grad, red["g"][l][1], name + " g", 1e-9)
        within(red["sums"][l][0], torch.cat([be.grad, ga.grad]), red["sums"][l][1], name + " sums", 1e-9)
        within(app["dz"][l][0], zl.grad, app["dz"][l][1], name + " dz level %d" % l, 1e-8)
        within(app["dgamma"][l][0], ga.grad, app["dgamma"][l][1] + 1e-300, name + " dgamma", 1e-9)
        within(app["dbeta"][l][0], be.grad, app["dbeta"][l][1] + 1e-300, name + " dbeta", 1e-9)
    # the case's own coefficients and modes: written-out formulas, each level's own slices and count
    app_case = R.CASE[name.replace("red_", "app_", 1)]
    for act, _ in R.RED_MODES:
        ref = R.case_ref(case, (act, True), d, D)
        for l in range(P.n):
            zl, gl = R.lvl(z, P, l), R.lvl(gy, P, l)
            c = {k: sl(d[k].double(), o, l, ls, C) for k in ("scale", "shift", "mean", "invstd", "gamma")}
            g = gl * R.dswish(zl * c["scale"] + c["shift"]) if act else gl
            xh = (zl - c["mean"]) * c["invstd"]
            within(ref["g"][l][0], g, ref["g"][l][1], name + " g formula")
            within(ref["sums"][l][0], d["sums0"][2 * (o + l * ls):2 * (o + l * ls) + 2 * C] + torch.cat([g.sum(0), (g * xh).sum(0)]), ref["sums"][l][1], name + " sums formula")
            for grads in (True, False):
                ra = R.case_ref(app_case, (bool(act), grads), d, D)
                sm = d["sums"][2 * (o + l * ls):2 * (o + l * ls) + 2 * C]
                dz = c["gamma"] * c["invstd"] * (g - sm[:C] / P.rows[l] - xh * sm[C:] / P.rows[l])
                within(ra["dz"][l][0], dz, ra["dz"][l][1], name + " dz formula")
                assert ("dgamma" in ra) == grads
                if grads:
                    within(ra["dgamma"][l][0], sl(d["dgamma0"].double(), o, l, ls, C) + sm[C:], ra["dgamma"][l][1], name + " dgamma formula")
                    within(ra["dbeta"][l][0], sl(d["dbeta0"].double(), o, l, ls, C) + sm[:C], ra["dbeta"][l][1], name + " dbeta formula")
                    mk = R.case_ref(app_case, (bool(act), grads), d, D, model=True)          # the kernel-order form is the same number
                    within(mk["dz"][l][0], dz, ra["dz"][l][1], name + " dz kernel order")
    assert [c["name"].replace("app_", "red_", 1) for c in R.PYR_CASES if c["entry"] == "app"] == R.cases_of("red")


@pytest.mark.parametrize("name", R.cases_of("add"))
def test_add_bnsums_reference(name):
    case = R.CASE[name]
    d = R.case_inputs(case)
    P, C = R.pyr_of(case["pyr"]), case["C"]
    for with_c, _ in R.ADD_MODES:
        ref = R.case_ref(case, (with_c, False), d, D)
        for l in range(P.n):
            tot = sum(R.lvl(d[k], P, l).double() for k in (("a", "b", "c") if with_c else ("a", "b")))
            within(ref["out"][l][0], tot, ref["out"][l][1], name + " out")
            if case["zmask"] >> l & 1:
                xh = (d["z"][l].double() - d["mean"][l].double()) * d["invstd"][l].double()
                within(ref["sums"][l][0], d["sums0"][l] + torch.cat([tot.sum(0), (tot * xh).sum(0)]), ref["sums"][l][1], name + " sums")
            else:
                assert ref["sums"][l] is None


@pytest.mark.parametrize("name", R.cases_of("slice"))
def test_slice_reference_is_the_gather(name):
    case = R.CASE[name]
    d = R.case_inputs(case)
    P, N = R.pyr_of(case["pyr"]), case["N"]
    dst = R.slice_rows_pyr(P, d["src"], N, d["offs"])
    for l, (H, W) in enumerate(P.sizes):
        for b in range(P.B):
            for r in (0, H * W - 1):
                assert torch.equal(dst[P.row0[l] + b * H * W + r], d["src"][b, d["offs"][l] + r * N:d["offs"][l] + (r + 1) * N])
    assert bool((dst[~P.valid()] == 0).all())
    even = not (N & 1) and not (d["bstride"] & 1) and all(not (v & 1) for v in d["offs"])
    assert even == (N == 36 and not case["odd"])                      # the vec 2 path exactly on the all-even case


def test_grouped_depthwise_reference_reads_each_nets_parameters():
    case = R.CASE[R.cases_of("gdw")[0]]
    d = R.case_inputs(case)
    P, C, ls, o, ws, bs = R.pyr_of(case["pyr"]), case["C"], d["ls"], d["o"], d["w_stride"], d["bn_stride"]
    ref = R.case_ref(case, None, d, D)["y"]
    for l, (H, W) in enumerate(P.sizes):
        x = nchw(R.lvl(d["x"], P, l).double(), P.B, H, W)
        for b in range(P.B):
            g = b // R.GROUP_IMAGES
            sc, sh = (d[k].double()[o + g * bs + l * ls:o + g * bs + l * ls + C].view(1, C, 1, 1) for k in ("sc_buf", "sh_buf"))
            y = rows_of(conv_t(swish(x[b:b + 1] * sc + sh), d["w_buf"].double()[g * ws:g * ws + 9 * C].view(9, C)))
            within(ref[l][0][b * H * W:(b + 1) * H * W], y, ref[l][1][b * H * W:(b + 1) * H * W], "grouped dw level %d image %d" % (l, b))
    assert not torch.equal(d["w_buf"][:9 * C], d["w_buf"][ws:ws + 9 * C])


# ------------------------------------------------------------------------------------------------ 2. the pyramid helper
def test_pyramid_helper_restates_make_pyr():
    desc, row0, rows = R.pyramid(1, [(16, 8), (9, 15), (7, 5), (1, 3), (1, 1)])
    assert list(desc) == [5, 1, 16, 8, 9, 15, 7, 5, 1, 3, 1, 1]
    assert rows == [128, 135, 35, 3, 1] and row0 == [0, 128, 384, 512, 640, 768]              # 128 rows: no padding; 1 row: 127 padding rows
    desc, row0, rows = R.pyramid(2, [(7, 5)])
    assert list(desc) == [1, 2, 7, 5] and rows == [70] and row0 == [0, 128]
    assert R.pyramid(3, [(1, 43)])[1] == [0, 256] and R.pyramid(1, [(1, 129), (1, 127)])[1] == [0, 256, 384]
    for name, (B, sizes) in R.PYRAMIDS.items():
        P = R.pyr_of(name)
        assert 1 <= P.n <= R.MAX_LEV and all(r0 % 128 == 0 for r0 in P.row0) and int(P.valid().sum()) == sum(P.rows)
        assert all(0 <= P.row0[l + 1] - P.row0[l] - P.rows[l] < 128 for l in range(P.n))
    P = R.pyr_of("p5")
    assert P.row0[1] - P.rows[0] == 0 and P.row0[5] - P.row0[4] - P.rows[4] == 127 and P.rows[1] > 128 and P.rows[1] % 128


# ------------------------------------------------------------------------------------------------ 3. route coverage
def test_no_dispatch_override_in_the_environment():
    assert not [k for k in os.environ if k.startswith(R.ENV_PREFIXES)]


def test_cases_reach_every_route_and_rider_combination():
    dw = set()
    for name in R.cases_of("dw"):
        c = R.CASE[name]
        for m in R.DW_MODES:
            r = R.dw_route_of(c, m)
            dw.add((m, r["kernel"], r["riders"], c["C"] >= 64))
    want = {(m, "tile", "separate" if "wg" in m else None, wide) for m in R.DW_MODES for wide in (True, False)}
    want |= {(m, "rows", "fused" if "wg" in m else None, True) for m in R.DW_MODES if m not in ("fwd_given", "fwd_live")}
    assert dw == want, sorted(dw ^ want, key=str)
    assert {c["C"] for c in R.PYR_CASES if c["entry"] == "dw"} == set(R.WIDTHS) | {8}
    # the stand-alone weight gradient: levels with nsplit 1 and with nsplit >= 2, also as the tile route's follow-up launch
    ns = [R.wgrad_nsplit(R.pyr_of(R.CASE[n]["pyr"])) for n in R.cases_of("wg")]
    assert any(max(v) >= 2 and min(v) == 1 for v in ns)
    assert any(max(R.dw_route_of(R.CASE[n], "bwd_wg_bn")["nsplit"] or [0]) >= 2 for n in R.cases_of("dw"))
    # the GEMM: (route, bf16) with statistics, with the strided head output; every case lands where it says
    seen = set()
    for name in R.cases_of("pw"):
        c = R.CASE[name]
        P = R.pyr_of(c["pyr"])
        for bf in (False, True):
            label, rec = R.route_pw(P, c["C"], c["N"], bf, bool(c["stats"]), bool(c["strided"]))
            assert label == c["route"][bf], (name, bf, label)
            seen.add((label, bf, "stats" if c["stats"] else None))
            seen.add((label, bf, "strided" if c["strided"] else "dense"))
            if label == "rows":
                assert P.Mt >= 32768 and c["C"] // 8 in R.pw_ref.ROWS_NKK and not c["stats"]
            if label == "t128x64":
                assert rec["big_tiles"] >= 800
    for label in ("skinny", "t128x32", "t64x64", "t128x64"):
        for bf in (False, True):
            assert {(label, bf, "stats"), (label, bf, "strided"), (label, bf, "dense")} <= seen, (label, bf)
    assert {("rows", False, "strided"), ("rows", False, "dense")} <= seen and not any(s[0] == "rows" and s[1] for s in seen)
    pw = [R.CASE[n] for n in R.cases_of("pw")]
    assert {c["C"] for c in pw} >= set(R.WIDTHS) and {36, R.N32_BIG} <= {c["N"] for c in pw} and any(c["N"] <= 16 for c in pw)
    assert {c["bias"] for c in pw} == {0, 1} and {c["act"] for c in pw} == {0, 2}
    assert R.route_pw(R.pyr_of("big"), 112, R.N32_BIG, False, True, True)[1]["bn"] == 32 and R.N32_BIG > 16
    # pyramids: n = 1 and n = 5; the grouped cases: whole row tiles per group on every level, and one pyramid that breaks it
    assert {R.pyr_of(c["pyr"]).n for c in R.PYR_CASES} >= {1, 5}
    g = R.CASE[R.cases_of("gpw")[0]]
    bm = R.group_tile_rows(R.pyr_of("pg"), g["C"], g["N"])
    assert bm == 32 and all((R.GROUP_IMAGES * h * w) % bm == 0 for h, w in R.pyr_of("pg").sizes)
    assert any((R.GROUP_IMAGES * h * w) % R.group_tile_rows(R.pyr_of("pgbad"), g["C"], g["N"]) for h, w in R.pyr_of("pgbad").sizes)
    assert R.pyr_of("pg").B == R.GROUP_N * R.GROUP_IMAGES


def test_route_spot_values():
    P = R.pyr_of("prow")
    assert R.route_dw(P, 112, 1, False, True, True) == {"kernel": "rows", "riders": "fused", "bn_sums": "fused", "nsplit": None,
                                                        "blocks": [2 * 2 * 1 * 3, 2 * 2 * 1 * 2, 2 * 2 * 1 * 1, 2 * 2 * 1 * 1]}
    assert R.route_dw(P, 112, 0, True)["kernel"] == "tile" and R.route_dw(P, 8, 1, False)["kernel"] == "tile"
    assert R.route_dw(R.pyr_of("p63"), 112, 1, False, True)["nsplit"] == [2, 1] and R.wgrad_nsplit(P) == [2, 1, 1, 1]
    assert R.wgrad_nsplit(R.Pyr(1, [(64, 64), (128, 128), (256, 256)])) == [8, 16, 16]
    # pw_ref.route under a pyramid: a gate refuses the row-slab kernel, the long-K kernel refuses the pyramid
    r = R.pw_ref.route
    assert r(0, 0, 0, 43648, 112, 112, pyr=True)["family"] == "rows" and r(0, 0, 0, 43648, 112, 112, gate=True, rpi=16, pyr=True)["family"] == "tiled"
    assert r(0, 0, 0, 43648, 112, 112, gate=True, rpi=16)["family"] == "rows"
    assert r(0, 0, 0, 1050, 720, 120)["family"] == "longk" and r(0, 0, 0, 1050, 720, 120, pyr=True)["family"] == "skinny"


# ------------------------------------------------------------------------------------------------ 5. calibration of K
@functools.lru_cache(maxsize=None)
def _k32():
    """K32 per family and where each family's worst sits.  One thread: the fp32 summation order of torch's CPU reductions then does not
    depend on how many cores the machine offers"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        k32 = {f: (0.0, "") for f in R.K_BY_FAMILY}
        for case in R.PYR_CASES:
            if case["entry"] == "slice":
                continue
            inp = R.case_inputs(case)
            for mode in R.modes_of(case):
                r64, r32 = R.case_ref(case, mode, inp, D), R.case_ref(case, mode, inp, S32, model=True)
                p32 = {(k, l): p for k, l, p in R.flat_pairs(r32)}
                for k, l, (v, A) in R.flat_pairs(r64):
                    fam = R.family_of(case, mode, k)
                    if k == "g" and not mode[0]:
                        continue                                        # (act none: g_out is a copy)
                    r = R.ratio_u(p32[(k, l)][0], v, A, R.UNIT[fam])
                    if r > k32[fam][0]:
                        k32[fam] = (r, "%s %s %s level %s" % (case["name"], mode, k, l))
        return k32
    finally:
        torch.set_num_threads(threads)


@pytest.mark.parametrize("family", sorted(R.K_BY_FAMILY))
def test_fp32_model_is_within_a_quarter_of_K(family):
    k32, where = _k32()[family]
    K = R.K_BY_FAMILY[family]
    print("K32 %-14s %.3f  (K %.1f)  worst at %s" % (family, k32, K, where))
    assert k32 <= K / 4
    assert K == float(max(8, math.ceil(4 * R.K32[family]))), "K is not max(8, ceil(4 * K32))"
    assert K == 8.0 or K <= 4 * k32 * 1.25 + 1, "K is larger than max(8, 4 * K32) calls for"
    assert abs(R.K32[family] - k32) <= 0.05 * k32 + 0.01, "the K32 recorded in pyr_ref.py is not the one measured"
