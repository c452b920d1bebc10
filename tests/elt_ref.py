"""Helper (not a test): float64 restatement of the row-streaming kernels of csrc/elt.hip, written from the formulas in the comments
of elt.hip and common.h (not from the kernels' loops), plus the inputs and the case lists that test_elt_ref_cpu.py and
test_gpu_elt_float64.py share.

Every reference computes in the dtype of its tensor arguments: called with float64 tensors it is the reference, called with the
same values as float32 it is the "plain fp32" evaluation that calibrates the tolerances (test_elt_ref_cpu.py).  Besides the value
each reference returns, per output element, the magnitude A of what was summed to make it:
  * a reduction: A = sum |term| (+ |initial value| where the kernel accumulates with +=)
  * an elementwise result: the largest absolute intermediate.  For f(u) with u = z*scale+shift that is |f(u)| + |f'(u)| * A_u,
    A_u = |z*scale| + |shift|: the rounding of u reaches the result through f', also where f(u) itself is small.
Errors are judged per element in units of U * A, U = 2^-24 (half an fp32 ulp of a value of size A):
    |got - ref64| <= K * U * A + tiny.
The K of each family is max(8, 4 * K32), K32 the largest error of the fp32 CPU evaluation in the same unit over the family's
cases (profiles/elt_float64_notes.md lists the measured K32).  The factor 4 is for what the CPU run does not have: another
summation tree (16 row groups, shuffles, LDS, atomics) and the device's exp / reciprocal intrinsics.  No constant comes from a
GPU run of the kernels."""
import math

import torch

U = 2.0 ** -24
TINY = 2.0 ** -126                   # smallest normal fp32: a result flushed to zero is not an error
SENTINEL = -7.25e33                  # guard rows behind every output

# K per family = max(8, 4 * K32); K32 measured by test_elt_ref_cpu.py (which asserts K32 <= K / 4)
K_AFFINE = 15.0
K_POOL = 23.0
K_POOL_BWD = 17.0
K_FINALIZE = 14.0
K_REDUCE = 27.0
K_APPLY = 32.0
K_COLSUM = 8.0
K_SE = 13.0
K_BY_FAMILY = {"affine": K_AFFINE, "pool": K_POOL, "pool_bwd": K_POOL_BWD, "finalize": K_FINALIZE, "reduce": K_REDUCE,
               "apply": K_APPLY, "colsum": K_COLSUM, "se": K_SE}

# eps and momentum as the kernels receive them (C floats)
EPS, MOMENTUM = float(torch.tensor(1e-3, dtype=torch.float32)), float(torch.tensor(0.01, dtype=torch.float32))


def cdiv(a, b):
    return -(-a // b)


def rows_per_block(M, C, reduces=False):
    """Which branch a case reaches: a COPY of elt_rows_per_block() in elt.hip (pool_nsplit: of the `ns` lines of chan_pool_impl and
    mmd_chan_pool_bwd).  Nothing checks the copy against the kernels' host code: keep it in step by hand when the dispatch changes."""
    blocks = cdiv(C, 64) * cdiv(M, 256)
    rpb = 256 if blocks >= 1024 else (128 if blocks >= 256 else 64)
    while reduces and rpb < 256 and cdiv(M, rpb) > 64:
        rpb *= 2
    return rpb


def pool_nsplit(B, rpi, C):
    return max(1, min(cdiv(1024, cdiv(C, 64) * B), cdiv(rpi, 64)))


# ------------------------------------------------------------------------------------------------ activations
def sigmoid(u):
    return torch.sigmoid(u)


def swish(u):
    return u * torch.sigmoid(u)


def dswish(u):
    s = torch.sigmoid(u)
    return s * (1 + u * (1 - s))


def d2swish(u):
    s = torch.sigmoid(u)
    return s * (1 - s) * (2 + u * (1 - 2 * s))


def act_fwd(u, Au, act):
    """a = act(u) and its magnitude"""
    if act == 0:
        return u, Au
    s = torch.sigmoid(u)
    if act == 1:
        return u * s, (u * s).abs() + dswish(u).abs() * Au
    return s, s + s * (1 - s) * Au


def dswish_mag(u, Au):
    """magnitude of swish'(u) = s*(1 + u*(1-s)): the two terms of the bracket by absolute value, and the rounding of u through swish''"""
    s = torch.sigmoid(u)
    return s * (1 + u.abs() * (1 - s)) + d2swish(u).abs() * Au


def _img(M, rpi):
    return torch.arange(M) // rpi


# ------------------------------------------------------------------------------------------------ elementwise
def affine_act(z, scale, shift, act, rowscale=None, rpi=1, res=None, A_shift=None):
    """y = act(z*scale+shift) * rowscale[row // rpi] + res.  A_shift: magnitude of the shift where it is itself a difference (live BN)"""
    if scale is None:
        u, Au = z, z.abs()
    else:
        u = z * scale + shift
        Au = (z * scale).abs() + (shift.abs() if A_shift is None else A_shift)
    a, A = act_fwd(u, Au, act)
    if rowscale is not None:
        rs = rowscale[_img(z.shape[0], rpi)].unsqueeze(1)
        a, A = a * rs, A * rs.abs()
    if res is not None:
        a, A = a + res, A + res.abs()
    return a, A


def chan_pool(z, scale, shift, act, g, out0, out_scale, B, rpi):
    """out[b,c] = out0[b,c] + out_scale * sum_rows (g ? g*a : a), a = act(z*scale+shift)"""
    u = z if scale is None else z * scale + shift
    a = swish(u) if act == 1 else u
    t = a if g is None else g * a
    C = z.shape[1]
    s = t.view(B, rpi, C).sum(1) * out_scale
    A = t.abs().view(B, rpi, C).sum(1) * abs(out_scale) + out0.abs()
    return out0 + s, A


def chan_pool_bwd(z, scale, shift, mean, invstd, g1, out0, B, rpi):
    """the five planes [5, B, C] of the SE backward pool: sum g1*a, sum g1*s', sum g1*s'*xhat, sum s', sum s'*xhat (+= out0)"""
    C = z.shape[1]
    u = z * scale + shift
    sp = dswish(u)
    xh = (z - mean) * invstd
    terms = [g1 * swish(u), g1 * sp, g1 * sp * xh, sp, sp * xh]
    out = torch.stack([t.view(B, rpi, C).sum(1) for t in terms]) + out0
    A = torch.stack([t.abs().view(B, rpi, C).sum(1) for t in terms]) + out0.abs()
    return out, A


def colsum(a, out0):
    return out0 + a.sum(0), out0.abs() + a.abs().sum(0)


# ------------------------------------------------------------------------------------------------ BatchNorm forward coefficients
def bn_finalize(stats, count, gamma, beta, rmean=None, rvar=None, momentum=MOMENTUM, eps=EPS):
    """stats: float64 [2C] = [sum z, sum z^2] (the same numbers the kernel receives).  Mean and variance are formed in float64, as the
    kernel's comment promises; everything after takes the dtype of gamma.  Returns (vals, mags)."""
    C = gamma.numel()
    dt = gamma.dtype
    n = float(count)
    mean64 = stats[:C] / n
    ex2 = stats[C:] / n
    var64 = (ex2 - mean64 * mean64).clamp_min(0.0)
    mean, var = mean64.to(dt), var64.to(dt)
    invstd = 1 / torch.sqrt(var + eps)
    scale = gamma * invstd
    shift = beta - mean * scale
    vals = {"scale": scale, "shift": shift, "mean": mean, "invstd": invstd}
    mags = {"scale": scale.abs(), "shift": beta.abs() + (mean * scale).abs(), "mean": mean.abs(), "invstd": invstd.abs()}
    if rmean is not None:
        unb = var * (n / (n - 1.0)) if n > 1 else var
        vals["rmean"] = (1 - momentum) * rmean + momentum * mean
        vals["rvar"] = (1 - momentum) * rvar + momentum * unb
        mags["rmean"] = ((1 - momentum) * rmean).abs() + (momentum * mean).abs()
        mags["rvar"] = ((1 - momentum) * rvar).abs() + (momentum * unb).abs()
    return vals, mags


def bn_finalize_all(stats_flat, counts, widths, gamma, beta, rmean, rvar, prev, nbt, momentum=MOMENTUM, eps=EPS):
    """Every layer of a net at once.  stats_flat: [2*C_l per layer] concatenated; counts: rows per layer (0 = idle this step: all six
    outputs keep `prev` / the running stats); num_batches_tracked += 1 for every layer."""
    vals = {k: prev[k].clone() for k in ("scale", "shift", "mean", "invstd")}
    vals["rmean"], vals["rvar"] = rmean.clone(), rvar.clone()
    mags = {k: v.abs() for k, v in vals.items()}
    off = 0
    for n, C in zip(counts, widths):
        sl = slice(off, off + C)
        if n > 0:
            v, m = bn_finalize(stats_flat[2 * off:2 * off + 2 * C], n, gamma[sl], beta[sl], rmean[sl], rvar[sl], momentum, eps)
            for k in vals:
                vals[k][sl], mags[k][sl] = v[k], m[k]
        off += C
    return vals, mags, nbt + 1


def bn_fold(gamma, beta, rmean, rvar, eps=EPS):
    scale = gamma / torch.sqrt(rvar + eps)
    shift = beta - rmean * scale
    return {"scale": scale, "shift": shift}, {"scale": scale.abs(), "shift": beta.abs() + (rmean * scale).abs()}


# ------------------------------------------------------------------------------------------------ BatchNorm backward
def bn_bwd_g(g_in, z, scale, shift, act, mul_bc, mul_b, add_bc, rpi):
    """g = (g_in * mul_bc[img] * mul_b[img] + add_bc[img]) * act'(z*scale+shift) and its magnitude"""
    img = _img(z.shape[0], rpi)
    g = g_in
    if mul_bc is not None:
        g = g * mul_bc[img]
    if mul_b is not None:
        g = g * mul_b[img].unsqueeze(1)
    A = g.abs()
    if add_bc is not None:
        g, A = g + add_bc[img], A + add_bc[img].abs()
    if act == 1:
        u = z * scale + shift
        g, A = g * dswish(u), A * dswish_mag(u, (z * scale).abs() + shift.abs())
    return g, A


def bn_bwd_reduce(g_in, z, scale, shift, mean, invstd, act, mul_bc, mul_b, add_bc, rpi, sums0):
    """-> g [M, C] with its magnitude, sums [2C] = sums0 + [sum g, sum g*xhat] with A = |sums0| + [sum |g|, sum |g*xhat|]"""
    g, Ag = bn_bwd_g(g_in, z, scale, shift, act, mul_bc, mul_b, add_bc, rpi)
    gx = g * ((z - mean) * invstd)
    sums = sums0 + torch.cat([g.sum(0), gx.sum(0)]).to(sums0.dtype)
    A = sums0.abs() + torch.cat([g.abs().sum(0), gx.abs().sum(0)]).to(sums0.dtype)
    return g, Ag, sums, A


def bn_bwd_apply(g, Ag, z, mean, invstd, gamma, sums, count, dgamma0=None, dbeta0=None, k=None):
    """dz = gamma*invstd*(g - m1 - xhat*m2), m = sums / count (sums: the float64 numbers the kernel receives); dgamma += sum g*xhat,
    dbeta += sum g.  k: the factor gamma*invstd itself where the kernel is handed that (the GEMM operand forms receive `scale`)"""
    C = z.shape[1]
    dt = z.dtype
    m1, m2 = (sums[:C] / float(count)).to(dt), (sums[C:] / float(count)).to(dt)
    xh = (z - mean) * invstd
    k = gamma * invstd if k is None else k
    dz = k * (g - m1 - xh * m2)
    A = k.abs() * (Ag + m1.abs() + (xh * m2).abs())
    out = {"dz": (dz, A)}
    if dgamma0 is not None:
        out["dgamma"] = (dgamma0 + sums[C:].to(dt), dgamma0.abs() + sums[C:].abs().to(dt))
        out["dbeta"] = (dbeta0 + sums[:C].to(dt), dbeta0.abs() + sums[:C].abs().to(dt))
    return out


# ------------------------------------------------------------------------------------------------ squeeze-excite FCs
def se_fwd(pooled, wr, br, wet, be):
    """wr [S, C], br [S], wet [S, C] (the expand weight transposed), be [C] -> hpre [B, S], gate [B, C] and magnitudes"""
    hpre = pooled @ wr.t() + br
    A_h = pooled.abs() @ wr.abs().t() + br.abs()
    h = swish(hpre)
    pre = h @ wet + be
    A_pre = (h.abs() + dswish(hpre).abs() * A_h) @ wet.abs() + be.abs()
    gate = torch.sigmoid(pre)
    return {"hpre": (hpre, A_h), "gate": (gate, gate + gate * (1 - gate) * A_pre)}


def se_bwd(dgate, gate, hpre, wr, wet, dpool_scale, pool5=None, bn_sums0=None):
    """dpe = dgate*gate*(1-gate); dh = dpe @ wet^T; dpr = dh*swish'(hpre); dpooled = dpool_scale * dpr @ wr;
    BN-1 sums += [sum_b gate*pool5[1] + dpooled*pool5[3], sum_b gate*pool5[2] + dpooled*pool5[4]]"""
    dpe = dgate * gate * (1 - gate)
    dh = dpe @ wet.t()
    A_dh = dpe.abs() @ wet.abs().t()
    s = torch.sigmoid(hpre)
    dpr = dh * dswish(hpre)
    A_dpr = A_dh * (s * (1 + hpre.abs() * (1 - s)))
    dpooled = (dpr @ wr) * dpool_scale
    A_dp = (A_dpr @ wr.abs()) * abs(dpool_scale)
    out = {"dpe": (dpe, dpe.abs()), "dh": (dh, A_dh), "dpr": (dpr, A_dpr), "dpooled": (dpooled, A_dp)}
    if pool5 is not None:
        s1 = (gate * pool5[1] + dpooled * pool5[3]).sum(0)
        s2 = (gate * pool5[2] + dpooled * pool5[4]).sum(0)
        A1 = ((gate * pool5[1]).abs() + A_dp * pool5[3].abs()).sum(0)
        A2 = ((gate * pool5[2]).abs() + A_dp * pool5[4].abs()).sum(0)
        out["bn_sums"] = (bn_sums0 + torch.cat([s1, s2]).to(bn_sums0.dtype), bn_sums0.abs() + torch.cat([A1, A2]).to(bn_sums0.dtype))
    return out


def se_wgrad(dpe, dpr, hpre, pooled, g0):
    """g0 = (dwr [S,C], dbr [S], dwe [S,C] transposed layout, dbe [C]) before the call; all four accumulate"""
    h = swish(hpre)
    dwr0, dbr0, dwe0, dbe0 = g0
    return {"dwr": (dwr0 + dpr.t() @ pooled, dwr0.abs() + dpr.abs().t() @ pooled.abs()),
            "dbr": (dbr0 + dpr.sum(0), dbr0.abs() + dpr.abs().sum(0)),
            "dwe": (dwe0 + h.t() @ dpe, dwe0.abs() + h.abs().t() @ dpe.abs()),
            "dbe": (dbe0 + dpe.sum(0), dbe0.abs() + dpe.abs().sum(0))}


# ------------------------------------------------------------------------------------------------ error unit
def ratio(got, ref, A):
    """max_i |got_i - ref_i| / (U * A_i + TINY): the error in the unit the K constants are stated in"""
    got, ref, A = got.detach().double().cpu(), ref.detach().double().cpu(), A.detach().double().cpu()
    assert got.shape == ref.shape == A.shape, (got.shape, ref.shape, A.shape)
    assert bool(torch.isfinite(got).all()), "non-finite output"
    err = (got - ref).abs()
    return float((err / (U * A + TINY)).max()) if got.numel() else 0.0


# ------------------------------------------------------------------------------------------------ shared inputs and cases
def f32(x):
    """a host scalar as the kernel receives it (a C float)"""
    return float(torch.tensor(x, dtype=torch.float32))


def rng(*seed):
    g = torch.Generator()
    g.manual_seed(sum(int(s) * p for s, p in zip(seed, (1, 1009, 100003, 10007, 101, 13))) % (2 ** 31))
    return g


def randn(g, *shape):
    return torch.randn(*shape, generator=g)


def rand(g, *shape):
    return torch.rand(*shape, generator=g)


def bn_inputs(g, M, C):
    """z [M, C] fp32 with its float64 raw sums, gamma, beta, and the fp32 (scale, shift, mean, invstd) the finalize formulas give.
    Below 32 rows the sums are not those of z alone (see below), so the consumers with live coefficients at M = 1 and M = 15 never see
    degenerate statistics: var = 0 and count == 1 are covered by the finalize cases (finalize_case, finalize_all_case) only."""
    z = randn(g, M, C) * 1.7 + 0.3
    gamma, beta = rand(g, C) + 0.5, randn(g, C) * 0.2
    # the batch statistics of a handful of rows are degenerate (one row: var = 0 and u = beta exactly, behind a scale of gamma / sqrt(eps)):
    # below 32 rows the sums are those of a 64-row batch that z is the head of
    zs = z if M >= 32 else torch.cat([z, randn(g, 64 - M, C) * 1.7 + 0.3])
    stats = torch.cat([zs.double().sum(0), (zs.double() ** 2).sum(0)])
    v, _ = bn_finalize(stats, zs.shape[0], gamma.double(), beta.double())
    coef = {k: t.float() for k, t in v.items()}
    coef["stats_count"] = zs.shape[0]
    return z, gamma, beta, stats, coef


ELT_SHAPES = [(1, 4), (15, 68), (77, 36), (257, 64), (4091, 1028), (4091, 4036)]


def affine_modes(M, C):
    """(act, coef in {null, given, live}, rowscale, res, in_place) per shape: every combination on the small shapes, a covering few on
    the two large ones"""
    if M * C > 4_000_000:
        return [(1, "given", True, True, False)]
    if M * C > 1_000_000:
        return [(2, "live", True, True, True), (0, "null", False, False, False), (1, "given", True, True, False)]
    modes = [(a, c, r, r, False) for a in (0, 1, 2) for c in ("null", "given", "live") for r in (False, True)]
    return modes + [(1, "given", True, False, True), (2, "live", False, True, True), (0, "null", True, True, True)]


def affine_rpi(M):
    return max(1, M // 7)            # 4091 // 7 = 584: divides neither 64, 128 nor 256, and leaves a ragged last image of 3 rows


def affine_case(M, C):
    g = rng(1, M, C)
    z, gamma, beta, stats, coef = bn_inputs(g, M, C)
    rpi = affine_rpi(M)
    return {"z": z, "gamma": gamma, "beta": beta, "stats": stats, "scale": coef["scale"], "shift": coef["shift"],
            "stats_count": coef["stats_count"], "rowscale": rand(g, cdiv(M, rpi)) * 1.5 - 0.25, "rpi": rpi, "res": randn(g, M, C)}


def affine_ref(case, mode, dt):
    """reference of one mode in dtype dt -> (y, A).  Live coefficients come from the finalize reference in dt; A then carries the
    shift's own magnitude |beta| + |mean*scale|."""
    act, coef, rs, res, _ = mode
    c = lambda t: t.to(dt)
    sc = sh = ash = None
    if coef == "given":
        sc, sh = c(case["scale"]), c(case["shift"])
    elif coef == "live":
        v, m = bn_finalize(case["stats"], case["stats_count"], c(case["gamma"]), c(case["beta"]))
        sc, sh, ash = v["scale"], v["shift"], m["shift"]
    return affine_act(c(case["z"]), sc, sh, act, c(case["rowscale"]) if rs else None, case["rpi"], c(case["res"]) if res else None, ash)


REDUCE_CASES = [(1, 4, 1, 1, 0), (15, 68, 3, 5, 0), (500, 48, 2, 250, 0), (4097, 20, 17, 241, 0), (16385, 20, 5, 3277, 0),
                (33000, 8, 4, 8250, 8)]       # (M, C, B, rpi, ws_slots)
REDUCE_MODS = [(), ("mul_bc",), ("mul_b",), ("add_bc",), ("mul_bc", "mul_b", "add_bc")]


def reduce_modes(M, C):
    """(act, modifiers, g_out given).  All twenty on the small shapes; the long ones take the covering four."""
    if M > 1000:
        return [(1, REDUCE_MODS[4], True), (0, REDUCE_MODS[0], False), (1, REDUCE_MODS[1], False), (0, REDUCE_MODS[4], True)]
    return [(a, m, o) for a in (0, 1) for m in REDUCE_MODS for o in (False, True)]


def reduce_case(M, C, B, rpi):
    g = rng(2, M, C)
    z, gamma, beta, stats, coef = bn_inputs(g, M, C)
    return {"z": z, "gamma": gamma, "g_in": randn(g, M, C), "mul_bc": rand(g, B, C) + 0.1, "mul_b": rand(g, B) + 0.2,
            "add_bc": randn(g, B, C) * 0.1, "rpi": rpi, "sums0": randn(g, 2 * C).double() * 3, "dgamma0": randn(g, C), "dbeta0": randn(g, C),
            **coef}


def reduce_ref(case, mode, dt):
    act, mods, _ = mode
    c = lambda t: t.to(dt)
    m = {k: (c(case[k]) if k in mods else None) for k in ("mul_bc", "mul_b", "add_bc")}
    return bn_bwd_reduce(c(case["g_in"]), c(case["z"]), c(case["scale"]), c(case["shift"]), c(case["mean"]), c(case["invstd"]), act,
                         m["mul_bc"], m["mul_b"], m["add_bc"], case["rpi"], case["sums0"])


def apply_modes(M, C):
    """(recompute g with act 1 and all three modifiers, dgamma / dbeta given)"""
    if M * C > 4_000_000:
        return [(True, True)]
    return [(False, True), (True, True), (False, False), (True, False)]


def apply_case(M, C):
    rpi = affine_rpi(M)                           # a ragged last image: the per-image tables have cdiv(M, rpi) rows
    case = reduce_case(M, C, cdiv(M, rpi), rpi)
    case["count"] = 2 * M + 1                     # count != M
    g = rng(3, M, C)
    case["sums"] = torch.cat([randn(g, C).double() * math.sqrt(M), randn(g, C).double() * math.sqrt(M)])
    return case


def apply_ref(case, mode, dt):
    recompute, grads = mode
    c = lambda t: t.to(dt)
    if recompute:
        g, Ag = bn_bwd_g(c(case["g_in"]), c(case["z"]), c(case["scale"]), c(case["shift"]), 1, c(case["mul_bc"]), c(case["mul_b"]),
                         c(case["add_bc"]), case["rpi"])
    else:
        g = c(case["g_in"]); Ag = g.abs()
    return bn_bwd_apply(g, Ag, c(case["z"]), c(case["mean"]), c(case["invstd"]), c(case["gamma"]), case["sums"], case["count"],
                        c(case["dgamma0"]) if grads else None, c(case["dbeta0"]) if grads else None)


POOL_SHAPES = [(1, 1, 4), (3, 17, 68), (2, 65, 36), (1, 1000, 20), (5, 200, 1028), (16, 130, 4100)]       # (B, rpi, C)


def pool_modes(B, rpi, C):
    """(g given, act, coef, out_scale = 1 / rpi)"""
    if B * rpi * C > 500_000:
        return [(False, 1, "given", True), (True, 1, "live", False), (True, 0, "null", False), (False, 0, "live", True)]
    return [(g, a, c, s) for g in (False, True) for a in (0, 1) for c in ("null", "given", "live") for s in (False, True)]


def pool_case(B, rpi, C):
    g = rng(4, B, rpi, C)
    M = B * rpi
    z, gamma, beta, stats, coef = bn_inputs(g, M, C)
    return {"z": z, "gamma": gamma, "beta": beta, "stats": stats, "g": randn(g, M, C), "out0": randn(g, B, C),
            "out5": randn(g, 5, B, C), "B": B, "rpi": rpi, **coef}


def pool_ref(case, mode, dt):
    gg, act, coef, inv = mode
    c = lambda t: t.to(dt)
    sc = sh = None
    if coef == "given":
        sc, sh = c(case["scale"]), c(case["shift"])
    elif coef == "live":
        v, _ = bn_finalize(case["stats"], case["stats_count"], c(case["gamma"]), c(case["beta"]))
        sc, sh = v["scale"], v["shift"]
    osc = f32(1.0 / case["rpi"]) if inv else 1.0
    return chan_pool(c(case["z"]), sc, sh, act, c(case["g"]) if gg else None, c(case["out0"]), osc, case["B"], case["rpi"])


def pool_bwd_ref(case, dt):
    c = lambda t: t.to(dt)
    return chan_pool_bwd(c(case["z"]), c(case["scale"]), c(case["shift"]), c(case["mean"]), c(case["invstd"]), c(case["g"]),
                         c(case["out5"]), case["B"], case["rpi"])


COLSUM_SHAPES = [(M, C) for M in (1, 255, 256, 257, 700) for C in (4, 36, 68, 132)]


def colsum_case(M, C):
    g = rng(5, M, C)
    return randn(g, M, C), randn(g, C) * 2


FINALIZE_WIDTHS = [4, 68, 260]
FINALIZE_KINDS = ["plain", "count1", "no_running", "no_mean_out"]


def finalize_case(C, kind):
    """stats built by hand so that channel 0 is constant (var exactly 0), channel 1 constant with sum z^2 a hair low (var < 0),
    channel 2 has |mean| = 1e3 and std = 1e-2; the rest come from data."""
    g = rng(6, C)
    n = 1 if kind == "count1" else 301
    z = (randn(g, n, C) * 1.7 + 0.3).double()
    z[:, 0] = 0.5
    z[:, 1] = -1.25
    if C > 2 and n > 1:
        z[:, 2] = -1e3 + 1e-2 * torch.randn(n, generator=g).double()
    stats = torch.cat([z.sum(0), (z * z).sum(0)])
    stats[C + 1] = stats[C + 1] * (1 - 1e-12)
    return {"stats": stats, "count": n, "gamma": rand(g, C) + 0.5, "beta": randn(g, C) * 0.2, "rmean": randn(g, C) * 0.1,
            "rvar": rand(g, C) + 0.5}


def finalize_ref(case, kind, dt):
    run = kind != "no_running"
    return bn_finalize(case["stats"], case["count"], case["gamma"].to(dt), case["beta"].to(dt), case["rmean"].to(dt) if run else None,
                       case["rvar"].to(dt) if run else None)


ALL_WIDTHS, ALL_COUNTS = [4, 68, 20], [300, 0, 1]         # three layers: active, idle, active with count == 1


def finalize_all_case():
    g = rng(7)
    tot = sum(ALL_WIDTHS)
    parts = []
    for C, n in zip(ALL_WIDTHS, ALL_COUNTS):
        z = (randn(g, max(n, 2), C) * 1.7 + 0.3).double()[:max(n, 1)]
        parts.append(torch.cat([z.sum(0), (z * z).sum(0)]))
    return {"stats": torch.cat(parts), "gamma": rand(g, tot) + 0.5, "beta": randn(g, tot) * 0.2, "rmean": randn(g, tot) * 0.1,
            "rvar": rand(g, tot) + 0.5, "prev": {k: randn(g, tot) for k in ("scale", "shift", "mean", "invstd")},
            "nbt": torch.tensor([3, 7, 0], dtype=torch.int64)}


def finalize_all_ref(case, dt):
    return bn_finalize_all(case["stats"], ALL_COUNTS, ALL_WIDTHS, case["gamma"].to(dt), case["beta"].to(dt), case["rmean"].to(dt),
                           case["rvar"].to(dt), {k: v.to(dt) for k, v in case["prev"].items()}, case["nbt"])


def fold_case(C):
    g = rng(8, C)
    rv = rand(g, C) + 0.3
    rv[0], rv[1] = 0.0, 1e-6
    return {"gamma": rand(g, C) + 0.5, "beta": randn(g, C), "rmean": randn(g, C), "rvar": rv}


def fold_ref(case, dt):
    return bn_fold(*(case[k].to(dt) for k in ("gamma", "beta", "rmean", "rvar")))


SE_SHAPES = [(1, 4, 1), (5, 16, 4), (3, 252, 5), (3, 260, 6), (2, 1028, 43), (2, 64, 256), (2, 3072, 128)]       # (B, C, S)
SE_AUX = (20, 3)                      # the second table entry of the batched weight-gradient launch: another (C, S), same B
SE_HW = 49


def se_case(B, C, S):
    """weights scaled as test_se_path scales them; pooled / dgate / pool5 as fp32 data.  hpre and gate handed to the backward are the
    float64 forward rounded to fp32, as a forward kernel would have left them."""
    g = rng(9, B, C, S)
    # the pool in float64 with bits below fp32 (the float64 average pool of 7 rows of swish): the Q36 integers are built from it
    pooled64, _ = chan_pool((randn(g, B * 7, C) * 1.5 + 0.5).double(), None, None, 1, None, torch.zeros(B, C, dtype=torch.float64), 1.0 / 7, B, 7)
    case = {"pooled64": pooled64, "pooled": pooled64.float(), "wr": randn(g, S, C) / math.sqrt(C), "br": randn(g, S),
            "wet": randn(g, S, C) / math.sqrt(S), "be": randn(g, C), "dgate": randn(g, B, C) * 3, "pool5": randn(g, 5, B, C) * 4,
            "bn_sums0": randn(g, 2 * C).double() * 5, "scale": f32(1.0 / SE_HW),
            "g0": [randn(g, S, C), randn(g, S), randn(g, S, C), randn(g, C)]}
    f = se_fwd(case["pooled"].double(), case["wr"].double(), case["br"].double(), case["wet"].double(), case["be"].double())
    case["hpre"], case["gate"] = f["hpre"][0].float(), f["gate"][0].float()
    Ca, Sa = SE_AUX
    case["aux"] = {"dpe": randn(g, B, Ca), "dpr": randn(g, B, Sa), "hpre": randn(g, B, Sa), "pooled": randn(g, B, Ca),
                   "g0": [randn(g, Sa, Ca), randn(g, Sa), randn(g, Sa, Ca), randn(g, Ca)]}
    return case


def se_fwd_ref(case, dt, pooled=None):
    c = lambda t: t.to(dt)
    return se_fwd(c(case["pooled"] if pooled is None else pooled), c(case["wr"]), c(case["br"]), c(case["wet"]), c(case["be"]))


def se_bwd_ref(case, dt, with_sums=True):
    c = lambda t: t.to(dt)
    return se_bwd(c(case["dgate"]), c(case["gate"]), c(case["hpre"]), c(case["wr"]), c(case["wet"]), case["scale"],
                  c(case["pool5"]) if with_sums else None, case["bn_sums0"] if with_sums else None)


def se_wgrad_ref(dpe, dpr, hpre, pooled, g0, dt):
    c = lambda t: t.to(dt)
    return se_wgrad(c(dpe), c(dpr), c(hpre), c(pooled), [c(t) for t in g0])
