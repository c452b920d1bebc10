"""CPU checks of tests/node_ref.py, the float64 references of the BiFPN node kernels (csrc/bifpn.hip):
  1. every reference against an independently written torch composite in float64 - F.interpolate(nearest), F.max_pool2d over an explicitly
     zero-padded map, F.conv2d(groups = C), F.conv2d 1x1, F.batch_norm(training = True) - and the backward against autograd of that
     composite, to 1e-12 relative, on every case of NODE_CASES;
  2. node_ref.route over NODE_CASES reaches every instantiation the dispatch macros can launch (the list is written out here);
  3. the conditions on the inputs: exact ties where the pooled operand is plain fp32, a separated arg-max in EVERY window where it is lazy;
  4. the tolerance constants K are calibrated here: the same formulas in fp32 on the CPU stay within K / 4 (K = max(8, 4 * K32))."""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

import node_ref as R
from elt_ref import EPS

D, S32 = torch.float64, torch.float32
BWD = ("bwd_full", "bwd_dw")


def within(got, ref, A, name, rtol=1e-12):
    got, ref, A = got.detach().double(), ref.detach().double(), A.detach().double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(((got - ref).abs() <= rtol * A + 1e-300).all()), "%s: worst %.3e of A" % (name, float(((got - ref).abs() / A.clamp_min(1e-300)).max()))
    assert bool((A >= got.abs() * (1 - 1e-9)).all()), name + ": A below |value|"


# ------------------------------------------------------------------------------------------------ the composite
def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def maxpool_torch(x):
    """F.max_pool2d(3, 2) over the map padded with explicit zeros the TF-SAME way (odd sizes: one on each side; even: high side only)"""
    PH, PW = x.shape[2:]
    OH, OW = (PH + 1) // 2, (PW + 1) // 2
    eh, ew = max(0, (OH - 1) * 2 + 3 - PH), max(0, (OW - 1) * 2 + 3 - PW)
    return F.max_pool2d(F.pad(x, (ew // 2, ew - ew // 2, eh // 2, eh - eh // 2)), 3, 2)


def composite(vals, mode, theta, w_dw, w_pw, bias):
    """vals: slot -> NCHW operand value.  -> (operands at the node's size, s, f, zd, z)"""
    r = F.relu(theta)
    w = r / (r.sum() + R.FUSE_EPS)
    ops = [vals[0]] + ([vals[1]] if mode & 1 else []) + ([F.interpolate(vals[2], scale_factor=2, mode="nearest")] if mode & 2 else []) + \
          ([maxpool_torch(vals[3])] if mode & 4 else [])
    s = sum(wi * o for wi, o in zip(w, ops))
    f = s * torch.sigmoid(s)
    C = f.shape[1]
    zd = F.conv2d(F.pad(f, (1, 1, 1, 1)), w_dw.t().reshape(C, 1, 3, 3), groups=C)
    z = F.conv2d(zd, w_pw.reshape(C, C, 1, 1), bias)
    return ops, s, f, zd, z


def operand_vals(case, d, grad=False):
    """the operands of a case as the node sees them (a lazy one through its BatchNorm), NCHW float64"""
    vals = {}
    for i in R.op_indices(case["mode"]):
        x = nchw(d[R.SLOT_KEY[i]].double())
        if case["lazy"] >> i & 1:
            lz = d["lz%d" % i]
            if R.lazy_form(case) == "live":
                x = F.batch_norm(x, None, None, lz["gamma"].double(), lz["beta"].double(), True, 0.0, EPS)
            else:
                x = x * lz["scale"].double().view(1, -1, 1, 1) + lz["shift"].double().view(1, -1, 1, 1)
        vals[i] = x.detach().requires_grad_(grad)
    return vals


def dd(d, *keys):
    return [d[k].double() if d.get(k) is not None else None for k in keys]


# ------------------------------------------------------------------------------------------------ 1. references against the composite
@pytest.mark.parametrize("name", R.cases_of("fwd", "eval", "dw", "lazy"))
def test_forward_references_match_the_composite(name):
    case = R.CASE[name]
    d = R.case_inputs(case)
    ref = R.case_ref(case, d, D)
    theta, w_dw, w_pw, bias, scale, shift = dd(d, "theta", "w_dw", "w_pw", "bias", "scale", "shift")
    _, _, f, zd, z = composite(operand_vals(case, d), case["mode"], theta, w_dw, w_pw, bias)
    want = {"f": nhwc(f), "zd": nhwc(zd), "z": nhwc(z), "y": nhwc(z) * scale + shift,
            "stats": d["stats0"] + torch.cat([z.sum((0, 2, 3)), (z * z).sum((0, 2, 3))])}
    for k, (v, A) in ref.items():
        within(v, want[k], A, "%s %s" % (name, k))
    if case["entry"] == "lazy" or case["entry"] == "fwd":
        assert bool((ref["stats"][1] >= d["stats0"].abs() + torch.cat([z.abs().sum((0, 2, 3)), (z * z).sum((0, 2, 3))]) * (1 - 1e-12)).all())


@pytest.mark.parametrize("name", R.cases_of("group"))
def test_grouped_reference_reads_each_nets_parameters(name):
    case = R.CASE[name]
    B, H, W, C = case["shape"]
    d = R.case_inputs(case)
    ref = R.case_ref(case, d, D)
    n, ws, bs = R.nops(case["mode"]), d["w_stride"], d["bn_stride"]
    for b in range(B):
        g = b // R.GROUP_IMAGES
        cut = lambda key, st, shape: d[key + "_buf"].double()[g * st:g * st + torch.Size(shape).numel()].view(shape)
        vals = {i: nchw(d[R.SLOT_KEY[i]][b:b + 1].double()) for i in R.op_indices(case["mode"])}
        _, _, f, zd, z = composite(vals, case["mode"], cut("theta", ws, (n,)), cut("w_dw", ws, (9, C)), cut("w_pw", ws, (C, C)), cut("bias", ws, (C,)))
        y = nhwc(z) * cut("scale", bs, (C,)) + cut("shift", bs, (C,))
        for k, want in (("y", y), ("f", nhwc(f)), ("zd", nhwc(zd))):
            within(ref[k][0][b:b + 1], want, ref[k][1][b:b + 1], "%s image %d %s" % (name, b, k))
    assert not torch.equal(d["w_dw_buf"][:9 * C], d["w_dw_buf"][ws:ws + 9 * C])


@pytest.mark.parametrize("name", R.cases_of("maxpool"))
def test_pool_reference_matches_max_pool2d_over_the_zero_padded_map(name):
    case = R.CASE[name]
    d = R.case_inputs(case)
    v, A = R.case_ref(case, d, D)["pool"]
    assert torch.equal(v, nhwc(maxpool_torch(nchw(d["src"].double()))))
    assert v.shape[1:3] == ((case["shape"][1] + 1) // 2, (case["shape"][2] + 1) // 2) and bool((A >= v.abs()).all())
    assert bool((v[0, 0, :, 0] == 0).all()) and bool((v[0, :, 0, 0] <= 0).all())      # the all-negative channel: the padding zero wins at the border


def test_pool_geometry_and_first_maximum():
    """odd sizes pad on both sides, even ones on the high side only; the arg-max is the FIRST maximum in row-major order, -1 for a padding zero"""
    assert [R.same_pad_lo(n, 3, 2) for n in (1, 2, 5, 7, 9, 16)] == [(1, 1), (1, 0), (3, 1), (4, 1), (5, 1), (8, 0)]
    p = torch.tensor([[1., 5, 5, 2], [5, 0, 1, -1], [3, -2, -3, -4], [-1, -2, -3, -1]], dtype=D).view(1, 4, 4, 1)
    v, arg = R.pool_arg(p)
    assert v.view(2, 2).tolist() == [[5.0, 5.0], [3.0, 0.0]]
    assert arg.view(2, 2).tolist() == [[1, 0], [0, -1]]          # (window (1, 1): the in-image -1s lose to the padding zero)
    z = torch.zeros(1, 2, 2, 1, dtype=D)
    assert R.pool_arg(z)[1].item() == 0                            # an in-image zero scanned before the padding keeps the gradient
    (dp, _), _ = R.pool_scatter(torch.ones(1, 2, 2, 1, dtype=D), torch.ones(1, 2, 2, 1, dtype=D), arg, 4, 4, torch.zeros(1, 4, 4, 1, dtype=D))
    assert dp.view(4, 4).tolist() == [[0, 1, 1, 0], [0, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0]]


@pytest.mark.parametrize("name", R.cases_of(*BWD))
def test_backward_references_match_autograd_of_the_composite(name):
    """the case's own inputs: the upstream gradient of the depthwise output (given, or the BatchNorm backward formula times w_pw) is sent
    through autograd of the composite; every output of every (acc, own) variant against it"""
    case = R.CASE[name]
    B, H, W, C = case["shape"]
    mode, full = case["mode"], case["entry"] == "bwd_full"
    d = R.case_inputs(case)
    theta = d["theta"].double().requires_grad_(True)
    w_dw = d["w_dw"].double().requires_grad_(True)
    vals = operand_vals(case, d, grad=True)
    ops, s, f, zd, _ = composite(vals, mode, theta, w_dw, d["w_pw"].double(), None)
    s.retain_grad()
    if full:
        g, z, sc, mu, istd = dd(d, "g", "z", "bn_scale", "bn_mean", "bn_invstd")
        m1, m2 = d["bn_sums"][:C] / d["count"], d["bn_sums"][C:] / d["count"]
        dz = sc * (g - m1 - (z - mu) * istd * m2)
        dzd = dz @ d["w_pw"].double()
    else:
        dzd = d["dzd"].double()
    zd.backward(nchw(dzd))
    init = {k: v.double() for k, v in d["init"].items()}
    n = R.nops(mode)
    for acc, own in R.BWD_VARIANTS:
        ref = R.case_ref(case, d, D, variant=(acc, own))
        want = {"wdot": init["wdot"][:n] + torch.stack([(s.grad * o).sum() for o in ops]), "dw_grad": init["dw_grad"] + w_dw.grad,
                "dtheta": None}
        if not full:
            want["dx"] = nhwc(s.grad)
        else:
            want.update(dz=dz, dgamma=init["dgamma"] + d["bn_sums"][C:], dbeta=init["dbeta"] + d["bn_sums"][:C])
        for i in R.op_indices(mode):
            gk, sk = R.GRAD_KEY[i], R.SUMS_KEY[i]
            mine = nhwc(vals[i].grad)
            if i == 3:
                if not full:
                    continue
                tot = init[gk] + mine
            else:
                tot = init[gk] * acc + mine
            want[gk] = tot
            if full:
                b = d["bn%d" % i]
                zz = (d[R.SLOT_KEY[i]] if b["z"] is None else b["z"]).double()
                xh = (zz - b["mean"].double()) * b["invstd"].double()
                gs = mine if (i == 3 or own >> i & 1) else tot
                want[sk] = b["sums0"] + torch.cat([gs.sum((0, 1, 2)), (gs * xh).sum((0, 1, 2))])
        assert set(ref) == set(want), (sorted(ref), sorted(want))
        for k, (v, A) in ref.items():
            if want[k] is not None:
                within(v, want[k], A, "%s acc %d own %d %s" % (name, acc, own, k))
        # d theta through the wdot contract: the wdot this launch adds, handed to theta_bwd, is autograd's d theta
        dth, _ = R.theta_bwd(theta.detach(), ref["wdot"][0] - init["wdot"][:n], torch.zeros(n, dtype=D))
        within(dth, theta.grad, ref["wdot"][1].sum() / (theta.detach().clamp_min(0).sum() + 1e-4) * torch.ones(n, dtype=D), name + " d theta")


@pytest.mark.parametrize("mode,H,W,C", [(5, 6, 10, 16), (2, 4, 6, 8), (4, 2, 2, 8), (3, 4, 4, 8), (6, 4, 4, 8), (1, 3, 5, 8)])
def test_whole_node_backward_matches_autograd_through_every_batchnorm(mode, H, W, C):
    """the node's own train-mode BatchNorm and the operands' (every operand lazy) as F.batch_norm(training=True): dz, dgamma / dbeta and the
    operand BatchNorm sums (= [dbeta_k, dgamma_k] of operand k's BatchNorm) against autograd"""
    B = 3
    g_ = R.rng(51, mode, H, W, C)
    rn = lambda *sh: torch.randn(*sh, generator=g_, dtype=D)
    shapes = {0: (B, H, W, C), 1: (B, H, W, C), 2: (B, H // 2, W // 2, C), 3: (B, 2 * H, 2 * W, C)}
    idx = R.op_indices(mode)
    raw = {i: rn(*shapes[i]) * 1.5 + 0.3 for i in idx}
    ga = {i: (rn(C) * 0.8).requires_grad_(True) for i in idx}
    be = {i: (rn(C) * 0.3).requires_grad_(True) for i in idx}
    vals = {i: F.batch_norm(nchw(raw[i]), None, None, ga[i], be[i], True, 0.0, EPS) for i in idx}
    for v in vals.values():
        v.retain_grad()
    theta = torch.tensor(R.THETA3[:len(idx)], dtype=D).requires_grad_(True)
    w_dw, w_pw, bias = (rn(9, C) / 3).requires_grad_(True), rn(C, C) / C ** 0.5, rn(C) * 0.1
    gamma, beta = (torch.rand(C, generator=g_, dtype=D) + 0.5).requires_grad_(True), (rn(C) * 0.1).requires_grad_(True)
    ops, s, f, zd, z = composite(vals, mode, theta, w_dw, w_pw, bias)
    z.retain_grad()
    y = F.batch_norm(z, None, None, gamma, beta, True, 0.0, EPS)
    gy = rn(*y.shape)
    y.backward(gy)
    M = B * H * W
    st = lambda t: torch.cat([t.sum((0, 1, 2)), (t * t).sum((0, 1, 2))])
    zr = nhwc(z.detach())
    c, _ = R.bn_finalize(st(zr), M, gamma.detach(), beta.detach())
    coef, bn, d = {}, {}, {}
    for i in idx:
        ci, _ = R.bn_finalize(st(raw[i]), raw[i].numel() // C, ga[i].detach(), be[i].detach())
        coef[i] = (ci["scale"], ci["shift"], None)
        bn[i] = (raw[i], ci["mean"], ci["invstd"], torch.zeros(2 * C, dtype=D))
        d[R.SLOT_KEY[i]] = raw[i]
    init = {"wdot": torch.zeros(4, dtype=D), "dw_grad": torch.zeros(9, C, dtype=D), "dpl": torch.zeros(shapes[3], dtype=D),
            "dgamma": torch.zeros(C, dtype=D), "dbeta": torch.zeros(C, dtype=D)}
    o = R.node_bwd_full(d, mode, theta.detach(), w_dw.detach(), init, 0, nhwc(gy), zr, c["scale"], c["mean"], c["invstd"],
                        torch.cat([beta.grad, gamma.grad]), M, w_pw, coef, bn, 0)
    within(o["dz"][0], nhwc(z.grad), o["dz"][1], "dz", 1e-11)
    within(o["dgamma"][0], gamma.grad, o["dgamma"][1], "dgamma")
    within(o["dbeta"][0], beta.grad, o["dbeta"][1], "dbeta")
    within(o["dw_grad"][0], w_dw.grad, o["dw_grad"][1], "dw_grad", 1e-11)
    for i in idx:
        within(o[R.GRAD_KEY[i]][0], nhwc(vals[i].grad), o[R.GRAD_KEY[i]][1], "gradient of operand %d" % i, 1e-11)
        within(o[R.SUMS_KEY[i]][0], torch.cat([be[i].grad, ga[i].grad]), o[R.SUMS_KEY[i]][1], "sums of operand %d" % i, 1e-11)
    dth, A = R.theta_bwd(theta.detach(), o["wdot"][0], torch.zeros(len(idx), dtype=D))
    within(dth, theta.grad, A + o["wdot"][1].sum(), "d theta", 1e-11)


def test_fuse_weights_edges():
    w = R.fuse_weights(torch.tensor([-1.0, 0.9, 0.0], dtype=D))
    assert w[0] == 0 and w[2] == 0 and w[1] == 0.9 / (0.9 + R.FUSE_EPS)
    th = torch.tensor([0.7, -0.5, 0.0], dtype=D)
    dth, _ = R.theta_bwd(th, torch.ones(3, dtype=D), torch.zeros(3, dtype=D))
    assert dth[1] == 0 and dth[2] == 0 and dth[0] != 0              # relu'(0) = 0: an entry at exactly 0 is inactive


# ------------------------------------------------------------------------------------------------ 2. route coverage
def test_no_dispatch_override_in_the_environment():
    """MMD_NODE_NOPARK_MIN, MMD_NODE_CW16_BELOW, MMD_POOL_LDS_MIN, MMD_NO_POOL_LDS change the dispatch that node_ref.route copies"""
    assert not [k for k in os.environ if k.startswith(("MMD_NODE_", "MMD_POOL_LDS", "MMD_NO_POOL_LDS"))]


def _routes():
    ev, tr, dw, bw = set(), set(), set(), set()
    for c in R.NODE_CASES:
        B, H, W, C = c["shape"]
        e, m = c["entry"], c["mode"]
        if e in ("fwd", "eval", "group"):
            ev.add(R.route("eval", B, H, W, C, m))
        if e in ("fwd", "lazy"):
            tr.add(R.route("train", B, H, W, C, m, lazy=c["lazy"]))
        if e in ("dw", "group"):
            dw.add(R.route("dw", B, H, W, C, m))
        if e == "bwd_full":
            bw.update(r for _, r in R.bwd_forms(c))
        if e == "bwd_dw":
            bw.add(R.route("bwd_dw", B, H, W, C, m))
    return ev, tr, dw, bw


def test_cases_reach_every_instantiation():
    ev, tr, dw, bw = _routes()
    assert ev == {("eval", m, C, True) for C in (64, 112, 160, 224) for m in (1, 2, 4, 5)} | {("eval", 2, 112, False)}
    assert tr == {("train", m, C, C <= 160) for C in (64, 112, 160, 224) for m in (1, 2, 4, 5)}
    assert dw == {("dw", 1), ("dw", 2)}
    T, Fa = True, False
    gemm = {(5, 0, 64, Fa), (5, 0, 64, T), (2, 0, 64, Fa), (4, 0, 64, Fa), (4, 0, 64, T),                                            # generic K: C = 64, 160
            (5, 7, 64, Fa), (5, 7, 64, T), (5, 7, 16, Fa), (2, 7, 64, Fa), (2, 7, 16, Fa), (4, 7, 64, Fa), (4, 7, 64, T), (4, 7, 16, Fa),      # C = 112
            (5, 14, 64, Fa), (5, 14, 16, Fa), (2, 14, 64, Fa), (2, 14, 16, Fa), (4, 14, 64, Fa), (4, 14, 16, Fa)}                    # C = 224: no room for the fine tile
    generic = {(1, 0, 64, Fa), (3, 0, 64, Fa), (6, 0, 64, Fa)}
    assert bw == {("bwd", m, True, nk, cw, pl) for m, nk, cw, pl in gemm} | {("bwd", m, False, nk, cw, pl) for m, nk, cw, pl in generic}
    # lazy forward cases exist for every width that allows them, and the train route of C = 224 does not
    assert {R.CASE[n]["shape"][3] for n in R.cases_of("lazy")} == {64, 112, 160}


def test_route_spot_values():
    assert R.route("eval", 256, 10, 10, 112, 2) == ("eval", 2, 112, False) and R.route("eval", 255, 10, 10, 112, 2) == ("eval", 2, 112, True)
    assert R.route("eval", 1024, 2, 2, 112, 2) == ("eval", 2, 112, False) and R.route("eval", 1023, 2, 2, 112, 2) == ("eval", 2, 112, True)
    assert R.route("eval", 1024, 2, 2, 64, 2)[3] and R.route("eval", 1024, 2, 2, 112, 5)[3]          # only (in, up) at C = 112 has the kernel
    assert R.route("eval", 2, 8, 8, 112, 3) is None and R.route("eval", 2, 8, 8, 48, 2) is None and R.route("eval", 2, 7, 8, 112, 2) is None
    assert R.route("train", 2, 8, 8, 224, 2, lazy=1) is None and R.route("train", 2, 8, 8, 224, 2) == ("train", 2, 224, False)
    assert R.route("bwd_dw", 2, 6, 10, 48, 7) is None               # four operands: fuse_fill refuses, the MODE 7 instantiation is unreachable
    assert R.route("bwd_full", 8, 64, 64, 112, 5, dpl=True) == ("bwd", 5, True, 7, 64, True)         # the benchmarked level: default form
    assert R.route("bwd_full", 8, 4, 4, 112, 4, dpl=True) == ("bwd", 4, True, 7, 16, False)


# ------------------------------------------------------------------------------------------------ 3. conditions on the inputs
def test_lazy_pooled_operands_have_a_separated_argmax_in_every_window():
    names = [c["name"] for c in R.NODE_CASES if c["lazy"] & 8]
    assert len(names) >= 15 and any(R.CASE[n]["entry"] == "bwd_full" for n in names)
    for n in names:
        gap = R.pool_gap(R.CASE[n], R.case_inputs(R.CASE[n]))          # the minimum over every window of the case: none is excluded
        assert gap > R.GAP, (n, gap)


def test_plain_pooled_operands_hold_exact_ties_and_theta_is_fp32():
    for c in R.NODE_CASES:
        d = R.case_inputs(c)
        if "theta" in d:
            assert d["theta"].dtype == S32
        if c["mode"] & 4 and not c["lazy"] & 8 and c["pool"] == "mixed":
            p = d["pl"]
            assert torch.equal(p[:, 1::2, :, 1::4], p[:, 0::2, :, 1::4]) and bool((p[:, -1, :, 2::4] == 0).all())
            taps, inside, _ = R.pool_taps(p.double())
            v = torch.where(inside[:, None, :, :, None], taps, torch.zeros_like(taps))
            top = v.topk(2, dim=0)[0]
            assert int((top[0] == top[1]).sum()) > 0, c["name"]


def test_lazy_padding_cases_are_what_they_say():
    for m in (4, 5):
        for kind in ("padlose", "padwin"):
            c = R.CASE["lazy_%s_m%d" % (kind, m)]
            d = R.case_inputs(c)
            sc, sh, _ = R.lazy_coef(R._to(d["lz3"], D, "cpu"), D, "live")
            t = d["pl"].double() * sc + sh
            arg = R.pool_arg(t)[1]
            if kind == "padlose":
                assert bool((d["pl"] < 0).all()) and bool((t > 0).all()) and bool((arg >= 0).all())
            else:
                assert bool((t < 0).all()) and bool((arg[:, -1] == -1).all()) and bool((arg[:, :, -1] == -1).all()) and bool((arg[:, :-1, :-1] >= 0).all())


# ------------------------------------------------------------------------------------------------ 4. calibration of K
@functools.lru_cache(maxsize=None)
def _k32():
    """K32 per family and where each family's worst sits.  One thread: the fp32 summation order of torch's CPU reductions and matmul then
    does not depend on how many cores the machine offers"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _k32_measure()
    finally:
        torch.set_num_threads(threads)


def _k32_measure():
    k32 = {f: (0.0, "") for f in R.K_BY_FAMILY}
    for case in R.NODE_CASES:
        inp = R.case_inputs(case)
        for v in (R.BWD_VARIANTS if case["entry"] in BWD else [None]):
            r64, r32 = R.case_ref(case, inp, D, variant=v), R.case_ref(case, inp, S32, variant=v)
            for out in r64:
                fam = R.FAMILY[out]
                r = R.ratio(r32[out][0], r64[out][0], r64[out][1])
                if r > k32[fam][0]:
                    k32[fam] = (r, "%s %s %s" % (case["name"], v, out))
    return k32


@pytest.mark.parametrize("family", sorted(R.K_BY_FAMILY))
def test_fp32_cpu_evaluation_is_within_a_quarter_of_K(family):
    """K = max(8, 4 * K32): the constant in node_ref is the one this measurement gives, and the fp32 CPU run stays within K / 4"""
    k32, where = _k32()[family]
    K = R.K_BY_FAMILY[family]
    print("K32 %-10s %.3f  (K %.1f)  worst at %s" % (family, k32, K, where))
    assert k32 <= K / 4
    assert K == 8.0 or K <= 4 * k32 * 1.25 + 1, "K is larger than max(8, 4 * K32) calls for"
    assert abs(R.K32[family] - k32) <= 0.05 * k32 + 0.01, "the K32 recorded in node_ref.py is not the one measured"
