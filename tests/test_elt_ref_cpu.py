"""CPU checks of tests/elt_ref.py, the float64 references of the row-streaming kernels (csrc/elt.hip):
  1. the references agree with torch autograd in float64 (F.batch_norm in training mode + swish with the per-image modifiers; the
     squeeze-excite block of test_gpu_kernels.test_se_path in double) to rtol 1e-12 per element;
  2. the tolerance constants K of elt_ref are calibrated here: the same formulas evaluated in fp32 torch on the CPU, on the very cases
     the GPU tests run, stay within K / 4 of the float64 reference in units of 2^-24 * A (K = max(8, 4 * K32))."""
import pytest
import torch
import torch.nn.functional as F

import elt_ref as R

D, S32 = torch.float64, torch.float32


def rel_close(got, ref, name, rtol=1e-12):
    got, ref = got.detach().double(), ref.detach().double()
    assert got.shape == ref.shape, name
    bad = (got - ref).abs() > rtol * ref.abs()
    assert not bool(bad.any()), "%s: %d elements off, worst rel %.3e" % (name, int(bad.sum()), float(((got - ref).abs() / ref.abs().clamp_min(1e-300)).max()))


# ------------------------------------------------------------------------------------------------ 1. the references are right
@pytest.mark.parametrize("M,C,B,act", [(500, 48, 2, 1), (63, 20, 3, 0), (15, 68, 5, 1)])
def test_bn_references_match_float64_autograd(M, C, B, act):
    g = R.rng(11, M, C)
    rpi = M // B
    z = (R.randn(g, M, C).double() * 2 + 0.5).requires_grad_(True)
    gamma = (R.rand(g, C).double() + 0.5).requires_grad_(True)
    beta = (R.randn(g, C).double() * 0.1).requires_grad_(True)
    rm, rv = R.randn(g, C).double() * 0.1, R.rand(g, C).double() + 0.5
    rm2, rv2 = rm.clone(), rv.clone()
    y = F.batch_norm(z, rm2, rv2, gamma, beta, True, R.MOMENTUM, R.EPS)
    a = R.swish(y) if act else y
    mul_bc, add_bc, mul_b = R.rand(g, B, C).double(), R.randn(g, B, C).double() * 0.1, R.rand(g, B).double()
    gin = R.randn(g, M, C).double()
    geff = gin * mul_bc.repeat_interleave(rpi, 0) * mul_b.repeat_interleave(rpi).view(-1, 1) + add_bc.repeat_interleave(rpi, 0)
    a.backward(geff)
    zd = z.detach()
    stats = torch.cat([zd.sum(0), (zd * zd).sum(0)])
    v, _ = R.bn_finalize(stats, M, gamma.detach(), beta.detach(), rm, rv)
    rel_close(v["rmean"], rm2, "running mean"); rel_close(v["rvar"], rv2, "running var")
    rel_close(v["mean"], zd.mean(0), "mean")
    ya, _ = R.affine_act(zd, v["scale"], v["shift"], act)
    # y = z*scale+shift cancels where z is close to the mean: per element relative to |z*scale| + |shift|, the magnitude the reference reports
    _, Ay = R.affine_act(zd, v["scale"], v["shift"], 0)
    assert bool(((ya - a.detach()).abs() <= 1e-12 * Ay).all())
    gg, Ag, sums, As = R.bn_bwd_reduce(gin, zd, v["scale"], v["shift"], v["mean"], v["invstd"], act, mul_bc, mul_b, add_bc, rpi,
                                       torch.zeros(2 * C, dtype=D))
    assert bool((Ag >= gg.abs() * (1 - 1e-12)).all()) and bool((As >= sums.abs() * (1 - 1e-12)).all())
    rel_close(sums[:C], beta.grad, "sum g = dbeta"); rel_close(sums[C:], gamma.grad, "sum g*xhat = dgamma")
    pre = torch.ones(C, dtype=D) * 0.75
    out = R.bn_bwd_apply(gg, Ag, zd, v["mean"], v["invstd"], gamma.detach(), sums, M, pre, -pre)
    dz, Adz = out["dz"]
    # dz is a difference of three terms of size A: the agreement is 1e-12 of that size per element
    assert bool(((dz - z.grad).abs() <= 1e-12 * Adz).all()), float(((dz - z.grad).abs() / Adz).max())
    # (dgamma0 + sum - dgamma0 rounds at the size of the accumulated value: 1e-12 of the magnitude the reference reports for it)
    assert bool(((out["dgamma"][0] - pre - gamma.grad).abs() <= 1e-12 * out["dgamma"][1]).all())
    assert bool(((out["dbeta"][0] + pre - beta.grad).abs() <= 1e-12 * out["dbeta"][1]).all())
    # count > 1 guard and eval-mode fold
    v1, _ = R.bn_finalize(torch.cat([zd[0], zd[0] ** 2]), 1, gamma.detach(), beta.detach(), rm, rv)
    assert bool((v1["rvar"] <= (1 - R.MOMENTUM) * rv + 1e-12).all()) and bool(torch.isfinite(v1["rvar"]).all())
    f, _ = R.bn_fold(gamma.detach(), beta.detach(), rm, rv)
    ye = F.batch_norm(zd, rm, rv, gamma.detach(), beta.detach(), False, 0.0, R.EPS)
    assert bool(((zd * f["scale"] + f["shift"] - ye).abs() <= 1e-12 * ((zd * f["scale"]).abs() + f["shift"].abs())).all())


def test_finalize_all_is_finalize_per_layer():
    case = R.finalize_all_case()
    v, m, nbt = R.finalize_all_ref(case, D)
    assert nbt.tolist() == [4, 8, 1]
    off = 0
    for n, C in zip(R.ALL_COUNTS, R.ALL_WIDTHS):
        sl = slice(off, off + C)
        if n == 0:
            for k in ("scale", "shift", "mean", "invstd"):
                assert torch.equal(v[k][sl], case["prev"][k][sl].double())
            assert torch.equal(v["rmean"][sl], case["rmean"][sl].double()) and torch.equal(v["rvar"][sl], case["rvar"][sl].double())
        else:
            one, _ = R.bn_finalize(case["stats"][2 * off:2 * off + 2 * C], n, case["gamma"][sl].double(), case["beta"][sl].double(),
                                      case["rmean"][sl].double(), case["rvar"][sl].double())
            for k in one:
                assert torch.equal(v[k][sl], one[k]), k
        off += C


@pytest.mark.parametrize("C,S", [(144, 6), (20, 3)])
def test_se_references_match_float64_autograd(C, S):
    g = R.rng(12, C, S)
    B, HW = 3, 64
    z = R.randn(g, B * HW, C).double().requires_grad_(True)
    sc, sh = R.rand(g, C).double() + 0.5, R.randn(g, C).double() * 0.1
    wr = (R.randn(g, S, C).double() / 12).requires_grad_(True); br = R.randn(g, S).double().requires_grad_(True)
    we = (R.randn(g, C, S).double() / 3).requires_grad_(True); be = R.randn(g, C).double().requires_grad_(True)
    a = R.swish(z * sc + sh).view(B, HW, C)
    pooled = a.mean(1); pooled.retain_grad()
    hpre = pooled @ wr.t() + br; hpre.retain_grad()
    h = R.swish(hpre); h.retain_grad()
    pre = h @ we.t() + be; pre.retain_grad()
    gate = torch.sigmoid(pre); gate.retain_grad()
    out = a * gate.unsqueeze(1)
    gout = R.randn(g, B, HW, C).double()
    out.backward(gout)
    zd, g1 = z.detach(), gout.reshape(B * HW, C)
    wet = we.detach().t().contiguous()
    zero = torch.zeros(B, C, dtype=D)
    p, Ap = R.chan_pool(zd, sc, sh, 1, None, zero, 1.0 / HW, B, HW)
    rel_close(p, pooled, "pool"); assert bool((Ap >= p.abs() * (1 - 1e-12)).all())
    f = R.se_fwd(p, wr.detach(), br.detach(), wet, be.detach())
    rel_close(f["hpre"][0], hpre, "hpre"); rel_close(f["gate"][0], gate, "gate")
    dgate, _ = R.chan_pool(zd, sc, sh, 1, g1, zero, 1.0, B, HW)
    rel_close(dgate, gate.grad, "dgate")
    mu, istd = R.randn(g, C).double() * 0.2, R.rand(g, C).double() + 0.5
    pool5, A5 = R.chan_pool_bwd(zd, sc, sh, mu, istd, g1, torch.zeros(5, B, C, dtype=D), B, HW)
    assert bool((A5 >= pool5.abs() * (1 - 1e-12)).all())
    rel_close(pool5[0], dgate, "plane 0 = dgate")
    b = R.se_bwd(dgate, f["gate"][0], f["hpre"][0], wr.detach(), wet, 1.0 / HW, pool5, torch.zeros(2 * C, dtype=D))
    # (gradients are sums of signed terms: 1e-12 of the magnitude the reference reports, per element)
    for k, ref in (("dpe", pre.grad), ("dh", h.grad), ("dpr", hpre.grad), ("dpooled", pooled.grad / HW)):
        assert bool(((b[k][0] - ref).abs() <= 1e-12 * b[k][1]).all()), k
        assert bool((b[k][1] >= b[k][0].abs() * (1 - 1e-12)).all()), k
    w = R.se_wgrad(b["dpe"][0], b["dpr"][0], f["hpre"][0], p, [torch.ones(S, C, dtype=D), torch.ones(S, dtype=D),
                                                               torch.ones(S, C, dtype=D), torch.ones(C, dtype=D)])
    for k, ref in (("dwr", wr.grad), ("dbr", br.grad), ("dwe", we.grad.t()), ("dbe", be.grad)):
        assert bool(((w[k][0] - 1 - ref).abs() <= 1e-12 * w[k][1]).all()), k
    # dz through SE: the BN-1 upstream gradient g = (gout*gate + dpooled) * swish'(u), as bn_bwd_reduce forms it with mul_bc / add_bc
    gg, Ag, sums, As = R.bn_bwd_reduce(g1, zd, sc, sh, mu, istd, 1, f["gate"][0], None, b["dpooled"][0], HW, torch.zeros(2 * C, dtype=D))
    # (gout*gate + dpooled cancels in places: 1e-12 of the magnitude the reference reports for g, per element)
    assert bool(((gg * sc - z.grad).abs() <= 1e-12 * Ag * sc).all())
    # ... and its sums equal the identity over the five pooled planes
    ident = torch.cat([(f["gate"][0] * pool5[1] + b["dpooled"][0] * pool5[3]).sum(0), (f["gate"][0] * pool5[2] + b["dpooled"][0] * pool5[4]).sum(0)])
    assert bool(((ident - sums).abs() <= 1e-12 * As).all())
    assert bool(((b["bn_sums"][0] - sums).abs() <= 1e-12 * As).all())


def test_dispatch_rule_reaches_every_branch():
    """the cases the GPU tests run reach the branches the issue lists (the rule is restated in elt_ref from elt.hip's dispatch)"""
    assert [R.rows_per_block(M, C) for M, C in R.ELT_SHAPES] == [64, 64, 64, 64, 128, 256]
    assert [R.rows_per_block(M, C, True) for M, C, _, _, _ in R.REDUCE_CASES] == [64, 64, 64, 128, 256, 256]
    assert R.cdiv(33000, 256) > 128                      # MMD_STATS_DEPTH: the slotted path
    assert [R.pool_nsplit(*s) for s in R.POOL_SHAPES] == [1, 1, 2, 16, 4, 1]
    assert all(B * rpi == M for M, _, B, rpi, _ in R.REDUCE_CASES)


# ------------------------------------------------------------------------------------------------ 2. calibration of K
def _k32_affine():
    k = 0.0
    for M, C in R.ELT_SHAPES:
        case = R.affine_case(M, C)
        for mode in R.affine_modes(M, C):
            ref, A = R.affine_ref(case, mode, D)
            k = max(k, R.ratio(R.affine_ref(case, mode, S32)[0], ref, A))
    return k


def _k32_pool():
    k = 0.0
    for shp in R.POOL_SHAPES:
        case = R.pool_case(*shp)
        for mode in R.pool_modes(*shp):
            ref, A = R.pool_ref(case, mode, D)
            k = max(k, R.ratio(R.pool_ref(case, mode, S32)[0], ref, A))
    return k


def _k32_pool_bwd():
    k = 0.0
    for shp in R.POOL_SHAPES:
        case = R.pool_case(*shp)
        ref, A = R.pool_bwd_ref(case, D)
        k = max(k, R.ratio(R.pool_bwd_ref(case, S32)[0], ref, A))
    return k


def _k32_finalize():
    k = 0.0
    for C in R.FINALIZE_WIDTHS:
        for kind in R.FINALIZE_KINDS:
            case = R.finalize_case(C, kind)
            v, m = R.finalize_ref(case, kind, D)
            v32 = R.finalize_ref(case, kind, S32)[0]
            k = max([k] + [R.ratio(v32[n], v[n], m[n]) for n in v])
        f, fm = R.fold_ref(R.fold_case(C), D)
        f32 = R.fold_ref(R.fold_case(C), S32)[0]
        k = max([k] + [R.ratio(f32[n], f[n], fm[n]) for n in f])
    case = R.finalize_all_case()
    v, m, _ = R.finalize_all_ref(case, D)
    v32 = R.finalize_all_ref(case, S32)[0]
    return max([k] + [R.ratio(v32[n], v[n], m[n]) for n in v])


def _k32_reduce():
    k = 0.0
    for M, C, B, rpi, _ in R.REDUCE_CASES:
        case = R.reduce_case(M, C, B, rpi)
        for mode in R.reduce_modes(M, C):
            g, Ag, s, As = R.reduce_ref(case, mode, D)
            g32, _, s32, _ = R.reduce_ref(case, mode, S32)
            k = max(k, R.ratio(g32, g, Ag), R.ratio(s32, s, As))
    return k


def _k32_apply():
    k = 0.0
    for M, C in R.ELT_SHAPES:
        case = R.apply_case(M, C)
        for mode in R.apply_modes(M, C):
            ref, r32 = R.apply_ref(case, mode, D), R.apply_ref(case, mode, S32)
            k = max([k] + [R.ratio(r32[n][0], ref[n][0], ref[n][1]) for n in ref])
    return k


def _k32_colsum():
    k = 0.0
    for M, C in R.COLSUM_SHAPES:
        a, o = R.colsum_case(M, C)
        ref, A = R.colsum(a.double(), o.double())
        k = max(k, R.ratio(R.colsum(a, o)[0], ref, A))
    return k


def _k32_se():
    k = 0.0
    for shp in R.SE_SHAPES:
        case = R.se_case(*shp)
        f, f32 = R.se_fwd_ref(case, D), R.se_fwd_ref(case, S32)
        b, b32 = R.se_bwd_ref(case, D), R.se_bwd_ref(case, S32)
        dpe, dpr = b["dpe"][0].float(), b["dpr"][0].float()
        w, w32 = (R.se_wgrad_ref(dpe, dpr, case["hpre"], case["pooled"], case["g0"], dt) for dt in (D, S32))
        for ref, got in ((f, f32), (b, b32), (w, w32)):
            k = max([k] + [R.ratio(got[n][0], ref[n][0], ref[n][1]) for n in ref])
    return k


FAMILIES = {"affine": _k32_affine, "pool": _k32_pool, "pool_bwd": _k32_pool_bwd, "finalize": _k32_finalize, "reduce": _k32_reduce,
            "apply": _k32_apply, "colsum": _k32_colsum, "se": _k32_se}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_fp32_cpu_evaluation_is_within_a_quarter_of_K(family):
    """K = max(8, 4 * K32): the constant in elt_ref is the one this measurement gives, and the fp32 CPU run stays within K / 4"""
    k32 = FAMILIES[family]()
    K = R.K_BY_FAMILY[family]
    print("K32 %-9s %.3f  (K %.1f)" % (family, k32, K))
    assert k32 <= K / 4
    assert K == 8.0 or K <= 4 * k32 * 1.25 + 1, "K is larger than max(8, 4 * K32) calls for"
