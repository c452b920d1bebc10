"""Helper (not a test): float64 restatement of the BiFPN node kernels of csrc/bifpn.hip - mmd_bifpn_fuse_fwd, mmd_bifpn_node_dw_fwd,
mmd_bifpn_node_fwd_fused (+ grouped nets), mmd_bifpn_node_fwd_fused_train(_lz), mmd_maxpool_same_fwd, mmd_bifpn_node_dw_bwd,
mmd_bifpn_node_bwd_full_form, mmd_bifpn_theta_bwd - written from the formulas in the comments of bifpn.hip and the contracts of its entry
points, not from the kernels' loops; a copy of the host dispatch (route); and the one case table (NODE_CASES) that test_node_ref_cpu.py and
test_gpu_node_float64.py share.

Conventions are those of elt_ref.py and dw_ref.py.  Every reference computes in the dtype (and on the device) of its tensor arguments:
float64 is the oracle, float32 the "plain fp32" evaluation that calibrates K.  Tensors are NHWC, depthwise taps tap-major [9, C], the 1x1
weight [C out, C in].  Operand sets are bit masks: bit 0 = in1, bit 1 = up, bit 2 = pool.  Every reference returns (value, A), A_i the
magnitude of what was summed into element i:
  * fused activation: swish(sum w_i op_i) with A_s = sum w_i A_op_i carried through elt_ref.act_fwd; a lazy operand z*sc+sh has
    A = |z*sc| + A_sh (A_sh = |beta| + |mean*scale| where the coefficients come from live sums); the pooled operand's A is the max of |taps|
  * depthwise / 1x1 products: sum |w| * A_input (+ |bias|), the folded BatchNorm A_z * |scale| + |shift|
  * forward BatchNorm sums: |initial| + sum |term| + sum over the 8x8 blocks of |block partial| (the kernel adds each block's partial,
    formed with fp32 LDS atomics, to the double sums: one more fp32 rounding of that partial)
  * gradients: the magnitude of the upstream gradient carried through every product (|w| * A_g, A_df * elt_ref.dswish_mag, ...);
    reductions of such products (wdot, depthwise weight gradient, operand BatchNorm sums): |initial| + sum A_factor * |other factor|
Errors are judged per element: |got - ref64| <= K * 2^-24 * A + tiny, K = max(8, 4 * K32) per family, K32 the largest error of the fp32
CPU evaluation over every case of NODE_CASES in the same unit (test_node_ref_cpu.py measures it and asserts K32 <= K / 4).  No constant
comes from a GPU run of the kernels.

The node's BatchNorm backward is elt_ref.bn_bwd_apply (the formula bd_ref.bd_fwd wraps), its 1x1 input gradient a plain matmul."""
import functools
import math

import torch

from elt_ref import (swish, dswish, dswish_mag, act_fwd, ratio, rng, SENTINEL, f32, bn_finalize, bn_bwd_apply, cdiv, U, TINY)      # noqa: F401
from dw_ref import conv, conv_bwd_data, conv_bwd_weight, same_pad_lo, _padded, _win, _to                                          # noqa: F401

FUSE_EPS = f32(1e-4)                 # FUSE_EPS (bifpn.hip), the C float the kernels add
WIDTHS = (64, 112, 160, 224)         # mmd_bifpn_node_fused_supported
NOPARK_MIN = 1024                    # MMD_NODE_NOPARK_MIN unset
CW16_BELOW = 128                     # MMD_NODE_CW16_BELOW unset
POOL_LDS_MIN = 128                   # MMD_POOL_LDS_MIN unset
GAP = 2.0 ** -18                     # arg-max gap of a lazy pooled operand (see pool_gap)

# K per family = max(8, 4 * K32).  K32 as test_node_ref_cpu.py measures it (fp32 CPU evaluation of these references on every case):
K32 = {"fuse": 2.611, "dw": 2.924, "eval": 1.635, "z": 1.384, "sums": 4.375, "pool": 0.0, "opgrad": 3.861, "scatter": 1.247, "wdot": 0.025, "dtheta": 1.271, "wgrad": 2.109, "dz": 2.729, "dgamma": 1.697, "opsums": 0.762}
K_BY_FAMILY = {"fuse": 11.0, "dw": 12.0, "eval": 8.0, "z": 8.0, "sums": 18.0, "pool": 8.0, "opgrad": 16.0, "scatter": 8.0, "wdot": 8.0, "dtheta": 8.0, "wgrad": 9.0, "dz": 11.0, "dgamma": 8.0, "opsums": 8.0}


def nops(mode):
    return 1 + bin(mode).count("1")


def op_indices(mode):
    """operand slots (0 in0, 1 in1, 2 up, 3 pool) present in an operand set, in the order the fusion weights are assigned"""
    return [0] + [i + 1 for i in range(3) if mode >> i & 1]


# ------------------------------------------------------------------------------------------------ references: forward
def fuse_weights(theta):
    """w = relu(theta) / (sum relu(theta) + 1e-4), in the order of the non-null operands (in0, in1, up, pool)"""
    r = theta.clamp_min(0)
    return r / (r.sum() + FUSE_EPS)


def up2(u):
    """nearest x2: out[b, h, w] = u[b, h // 2, w // 2]"""
    return u.repeat_interleave(2, 1).repeat_interleave(2, 2)


def pool_taps(p):
    """the nine taps [9, B, OH, OW, C] of the 3x3 / stride-2 windows of p under TF-SAME ZERO padding, the mask [9, OH, OW] of the taps
    that lie inside the image, and the geometry (OH, OW, pad_t, pad_l)"""
    pp, OH, OW, pt, pl = _padded(p, 3, 2)
    ins = _padded(torch.ones_like(p[:1, :, :, :1]), 3, 2)[0]
    ij = [(i, j) for i in range(3) for j in range(3)]
    taps = torch.stack([pp[:, _win(i, OH, 2), _win(j, OW, 2)] for i, j in ij])
    inside = torch.stack([ins[0, _win(i, OH, 2), _win(j, OW, 2), 0] for i, j in ij]) > 0
    return taps, inside, (OH, OW, pt, pl)


def pool_arg(p):
    """-> (max, arg): arg = tap index 3i + j of the FIRST maximum in row-major order, -1 where a padding zero is that first maximum"""
    taps, inside, _ = pool_taps(p)
    best = torch.full_like(taps[0], -math.inf)
    arg = torch.full(taps[0].shape, -1, dtype=torch.int64, device=p.device)
    for t in range(9):
        upd = taps[t] > best
        best = torch.where(upd, taps[t], best)
        code = torch.where(inside[t], t, -1)[None, :, :, None].expand_as(arg)
        arg = torch.where(upd, code, arg)
    return best, arg


def pool_same(p, Ap=None):
    """3x3 / stride 2 max under TF-SAME padding, the zero padding taking part in the max.  A: the max of |taps|"""
    A = pool_taps(p.abs() if Ap is None else Ap)[0].max(0)[0]
    return pool_arg(p)[0], A


def lazy_coef(lz, dt, form):
    """(scale, shift, A_shift) of a lazy operand.  form "live": from the float64 batch sums, as the forward reads them (bn_live_coef =
    the finalize formulas, eps 1e-3); "final": the finalized fp32 (scale, shift) the backward is handed"""
    if form == "final":
        return lz["scale"].to(dt), lz["shift"].to(dt), None
    v, m = bn_finalize(lz["stats"], lz["count"], lz["gamma"].to(dt), lz["beta"].to(dt))
    return v["scale"], v["shift"], m["shift"]


def operands(d, mode, coef=None):
    """[(slot, value, A)] of the operand set at the node's resolution.  coef[slot] = (scale, shift, A_shift): the operand is given RAW and
    transformed while read; the pooled one inside the image only - the padding of the TRANSFORMED map is zero"""
    def tr(i, x):
        if coef and coef.get(i) is not None:
            sc, sh, ash = coef[i]
            return x * sc + sh, (x * sc).abs() + (sh.abs() if ash is None else ash)
        return x, x.abs()
    ops = [(0,) + tr(0, d["in0"])]
    if mode & 1:
        ops.append((1,) + tr(1, d["in1"]))
    if mode & 2:
        v, A = tr(2, d["up"])
        ops.append((2, up2(v), up2(A)))
    if mode & 4:
        v, A = tr(3, d["pl"])
        ops.append((3,) + pool_same(v, A))
    return ops


def fused(ops, theta):
    """f = swish(sum w_i op_i) -> (f, A_f, s, A_s)"""
    w = fuse_weights(theta)
    s = sum(w[k] * v for k, (_, v, _) in enumerate(ops))
    As = sum(w[k] * A for k, (_, _, A) in enumerate(ops))
    f, Af = act_fwd(s, As, 1)
    return f, Af, s, As


def sep_conv(f, Af, w_dw, w_pw, bias):
    """zd = dw3x3(f), z = zd . w_pw^T + bias"""
    zd, Azd = conv(f, Af, w_dw, 3, 1)
    z, Az = zd @ w_pw.t(), Azd @ w_pw.abs().t()
    if bias is not None:
        z, Az = z + bias, Az + bias.abs()
    return zd, Azd, z, Az


def node_dw(d, mode, theta, w_dw, coef=None):
    """mmd_bifpn_fuse_fwd / mmd_bifpn_node_dw_fwd -> {"f", "zd"}"""
    f, Af, _, _ = fused(operands(d, mode, coef), theta)
    return {"f": (f, Af), "zd": conv(f, Af, w_dw, 3, 1)}


def node_eval(d, mode, theta, w_dw, w_pw, bias, scale, shift):
    """mmd_bifpn_node_fwd_fused: y = ((dw3x3(fused) . w_pw^T) + bias) * scale + shift"""
    f, Af, _, _ = fused(operands(d, mode), theta)
    _, _, z, Az = sep_conv(f, Af, w_dw, w_pw, bias)
    return {"y": (z * scale + shift, Az * scale.abs() + shift.abs())}


def node_train(d, mode, theta, w_dw, w_pw, bias, stats0, coef=None):
    """mmd_bifpn_node_fwd_fused_train(_lz): z (raw, + bias), zd, stats = stats0 + [sum z, sum z^2] over the z of this dtype"""
    f, Af, _, _ = fused(operands(d, mode, coef), theta)
    zd, Azd, z, Az = sep_conv(f, Af, w_dw, w_pw, bias)
    B, H, W, C = z.shape
    zp = torch.nn.functional.pad(z, (0, 0, 0, cdiv(W, 8) * 8 - W, 0, cdiv(H, 8) * 8 - H)).view(B, cdiv(H, 8), 8, cdiv(W, 8), 8, C)
    part = torch.cat([zp.sum((2, 4)).abs().sum((0, 1, 2)), (zp * zp).sum((0, 1, 2, 3, 4))])
    dd = (0, 1, 2)
    st = stats0 + torch.cat([z.sum(dd), (z * z).sum(dd)]).to(stats0.dtype)
    Ast = stats0.abs() + (torch.cat([z.abs().sum(dd), (z * z).sum(dd)]) + part).to(stats0.dtype)
    return {"z": (z, Az), "zd": (zd, Azd), "stats": (st, Ast)}


def grouped(fn, d, n, images, keys, w_stride, bn_stride, sizes):
    """Grouped frozen nets: image b reads the parameters of net b // images; net g's theta / w_dw / w_pw / bias lie g * w_stride floats
    behind net 0's, its scale / shift g * bn_stride floats (fuse_dw_fwd_kernel: `a.theta += gw; wdw += gw`; bifpn_node_fused_kernel:
    `wdw += gw; wpw += gw; bias += gw; scale += gb; shift += gb; fuse_weights(a.theta + gw)`).  fn(operands of the net's images,
    {parameter: the net's view}) -> {out: (value, A)}; the images' results concatenated"""
    outs = []
    for g in range(n):
        sl = slice(g * images, (g + 1) * images)
        par = {}
        for k in keys:
            st = bn_stride if k in ("scale", "shift") else w_stride
            par[k] = d[k + "_buf"][g * st:g * st + math.prod(sizes[k])].view(sizes[k])
        outs.append(fn({k: d[k][sl] for k in ("in0", "in1", "up", "pl") if k in d}, par))
    return {k: (torch.cat([o[k][0] for o in outs]), torch.cat([o[k][1] for o in outs])) for k in outs[0]}


# ------------------------------------------------------------------------------------------------ references: backward
def pool_scatter(g, Ag, arg, PH, PW, init):
    """dpl = init + the scatter of g to the arg-max element of every window (dropped where arg = -1: a padding zero won)"""
    B, OH, OW, C = g.shape
    pt, pl = same_pad_lo(PH, 3, 2)[1], same_pad_lo(PW, 3, 2)[1]
    HP, WP = max((OH - 1) * 2 + 3, pt + PH), max((OW - 1) * 2 + 3, pl + PW)
    buf, A = g.new_zeros(B, HP, WP, C), g.new_zeros(B, HP, WP, C)
    for t in range(9):
        i, j = divmod(t, 3)
        m = arg == t
        buf[:, _win(i, OH, 2), _win(j, OW, 2)] += torch.where(m, g, torch.zeros_like(g))
        A[:, _win(i, OH, 2), _win(j, OW, 2)] += torch.where(m, Ag, torch.zeros_like(g))
    share, Ash = buf[:, pt:pt + PH, pl:pl + PW], A[:, pt:pt + PH, pl:pl + PW]
    return (init + share, init.abs() + Ash), (share, Ash)


def op_sums(gs, Ags, z, mean, invstd, sums0):
    """sums0 + [sum g, sum g * xhat], xhat = (z - mean) * invstd (common.h BnSumDst)"""
    xh = (z - mean) * invstd
    dd = (0, 1, 2)
    return (sums0 + torch.cat([gs.sum(dd), (gs * xh).sum(dd)]).to(sums0.dtype),
            sums0.abs() + torch.cat([Ags.sum(dd), (Ags * xh.abs()).sum(dd)]).to(sums0.dtype))


def fuse_bwd(d, mode, theta, w_dw, dzd, Adzd, init, acc, coef=None, bn=None, own=0, scatter=True):
    """The fusion + depthwise backward every node backward launch shares.  dzd: gradient w.r.t. the depthwise output.
        df = dwconv^T(dzd, w_dw),  dx = df * swish'(s),  s = sum w_i op_i
        d op_i = w_i * dx for the same-size operands, w_up * (2x2 block sums) for the up operand, w_pool * dx scattered to the FIRST maximum
        of each window for the pooled one (dropped where a padding zero wins);  gradients (+)= the running ones where acc
        wdot_i += <dx, op_i>;  dw_grad[t] += sum_q f[q + tap t] * dzd[q]
        operand BatchNorm sums bn[slot] = (z, mean, invstd, sums0): += [sum g, sum g xhat] of the completed gradient (own bit: of this
        launch's share); the pooled operand's: always of this launch's share
    init: the outputs' contents before the call -> {"dx", "d0", "d1", "dup", "dpl", "wdot", "dw_grad", "s0", "s1", "su", "sp"}"""
    ops = operands(d, mode, coef)
    w = fuse_weights(theta)
    f, Af, s, As = fused(ops, theta)
    B, H, W, C = s.shape
    df, Adf = conv_bwd_data(dzd, Adzd, w_dw, H, W, 3, 1)
    gx, Agx = df * dswish(s), Adf * dswish_mag(s, As)
    out = {"dx": (gx, Agx)}
    n = len(ops)
    wd0 = init["wdot"][:n]
    out["wdot"] = (wd0 + torch.stack([(gx * v).sum() for _, v, _ in ops]), wd0.abs() + torch.stack([(Agx * v.abs()).sum() for _, v, _ in ops]))
    out["dw_grad"] = (conv_bwd_weight(f, dzd, 3, 1, init["dw_grad"])[0], conv_bwd_weight(f.abs(), Adzd, 3, 1, init["dw_grad"].abs())[0])
    names = {0: ("d0", "s0", 1), 1: ("d1", "s1", 2), 2: ("dup", "su", 4)}
    for k, (slot, _, _) in enumerate(ops):
        if slot == 3:
            if not scatter:
                continue
            raw = d["pl"] if not (coef and coef.get(3) is not None) else d["pl"] * coef[3][0] + coef[3][1]
            arg = pool_arg(raw)[1]
            out["dpl"], (share, Ash) = pool_scatter(w[k] * gx, w[k] * Agx, arg, 2 * H, 2 * W, init["dpl"])
            if bn and bn.get(3):
                out["sp"] = op_sums(share, Ash, *bn[3])
            continue
        gname, sname, bit = names[slot]
        mine, Am = w[k] * gx, w[k] * Agx
        if slot == 2:
            mine, Am = (t.view(B, H // 2, 2, W // 2, 2, C).sum((2, 4)) for t in (mine, Am))
        tot, At = (init[gname] + mine, init[gname].abs() + Am) if acc else (mine, Am)
        out[gname] = (tot, At)
        if bn and bn.get(slot):
            out[sname] = op_sums(*((mine, Am) if own & bit else (tot, At)), *bn[slot])
    return out


def node_bwd_full(d, mode, theta, w_dw, init, acc, g, z, bn_scale, bn_mean, bn_invstd, bn_sums, count, w_pw, coef=None, bn=None, own=0):
    """mmd_bifpn_node_bwd_full: dz = scale * (g - m1 - xhat * m2), [m1, m2] = bn_sums / count; dgamma += sums[C:], dbeta += sums[:C];
    dzd = dz . w_pw (the kernel is handed w_pw transposed), then fuse_bwd"""
    C = g.shape[-1]
    o = bn_bwd_apply(g.reshape(-1, C), g.reshape(-1, C).abs(), z.reshape(-1, C), bn_mean, bn_invstd, None, bn_sums, count,
                     init["dgamma"], init["dbeta"], k=bn_scale)
    dz, Adz = (t.view(g.shape) for t in o["dz"])
    out = fuse_bwd(d, mode, theta, w_dw, dz @ w_pw, Adz @ w_pw.abs(), init, acc, coef, bn, own)
    del out["dx"]
    out.update(dz=(dz, Adz), dgamma=o["dgamma"], dbeta=o["dbeta"])
    return out


def theta_bwd(theta, wdot, dtheta0):
    """d theta_k += [theta_k > 0] * sum_i wdot_i * (delta_ik * S - r_i) / S^2,  S = sum r + eps (above fuse_theta_bwd_kernel)"""
    r = theta.clamp_min(0)
    S = r.sum() + FUSE_EPS
    n = theta.numel()
    eye = torch.eye(n, dtype=theta.dtype, device=theta.device)
    J = (eye * S - r.view(n, 1)) / (S * S)                       # J[i, k]
    on = (theta > 0).to(theta.dtype)
    return dtheta0 + on * (wdot[:n].view(n, 1) * J).sum(0), dtheta0.abs() + on * (wdot[:n].abs().view(n, 1) * (eye * S + r.view(n, 1)) / (S * S)).sum(0)


# ------------------------------------------------------------------------------------------------ the dispatch, copied
def route(entry, B, H, W, C, mode, lazy=0, dpl=False, small_below=-1, pool_lds=-1):
    """Which kernel instantiation a call reaches: a COPY of the host dispatch of bifpn.hip (MMD_NODE_FWD_C, MMD_NODE_FWD_TC,
    mmd_bifpn_node_dw_fwd, node_dw_bwd_impl) with no MMD_NODE_* / MMD_POOL_LDS_* / MMD_NO_POOL_LDS variable set.  Nothing checks the copy
    against the host code: keep it in step by hand when the dispatch changes.  None: the host refuses the call.
      "eval"     -> ("eval", MODE, FC, PK)         PK False = the no-park kernel
      "train"    -> ("train", MODE, FC, lazy allowed)
      "dw"       -> ("dw", 64-channel chunks)
      "bwd_full" -> ("bwd", MODE, True, NK, CW, pool_lds)    small_below / pool_lds: the NodeForm arguments (< 0: default)
      "bwd_dw"   -> ("bwd", MODE, False, 0, 64, pool_lds)"""
    n = nops(mode)
    if n < 2 or n > 3 or C <= 0 or (C & 3) or ((mode & 2) and ((H & 1) or (W & 1))):
        return None
    th, tw = cdiv(H, 8), cdiv(W, 8)
    if entry == "dw":
        return ("dw", cdiv(C, 64))
    if entry in ("eval", "train"):
        if C not in WIDTHS or (mode & 3) == 3 or mode not in (1, 2, 4, 5):
            return None
        if entry == "eval":
            return ("eval", mode, C, not (mode == 2 and C == 112 and B * th * tw >= NOPARK_MIN))
        if lazy and C > 160:
            return None
        return ("train", mode, C, C <= 160)
    full = entry == "bwd_full"
    if full and ((C & 15) or C > 224 or mode not in (2, 5, 4)):
        return None
    cc = cdiv(C, 64)
    below = small_below if small_below >= 0 else CW16_BELOW
    cw16 = full and C in (112, 224) and B * th * tw * cc < below
    if cw16:
        cc = cdiv(C, 16)
    grid = B * th * tw * cc
    on = pool_lds if pool_lds >= 0 else 1
    fine, gemm = 17 * 17 * 64 * 4, (100 * (C + 8) + 4 * C) * 4
    plds = bool(on and not cw16 and dpl and (grid >= POOL_LDS_MIN or pool_lds == 1) and
                ((gemm + fine + 30 * 1024) if full else (fine + 40 * 1024)) <= 160 * 1024)
    nk = {112: 7, 224: 14}.get(C, 0) if full else 0
    return ("bwd", mode, full, nk, 16 if cw16 else 64, plds)


FORMS = [(0, 0), (0, 1), (1 << 30, 0), (1 << 30, 1)]          # (small_below, pool_lds) of mmd_bifpn_node_bwd_full_form


def bwd_forms(case):
    """the (small_below, pool_lds) arguments that reach distinct kernels for a bwd_full case -> [((small_below, pool_lds), route)]"""
    B, H, W, C = case["shape"]
    seen, out = set(), []
    for sb, pl in FORMS:
        r = route("bwd_full", B, H, W, C, case["mode"], dpl=bool(case["mode"] & 4), small_below=sb, pool_lds=pl)
        if r not in seen:
            seen.add(r)
            out.append(((sb, pl), r))
    return out


# ------------------------------------------------------------------------------------------------ cases
THETA3 = [0.7, 1.3, 0.4]


def _c(name, entry, mode, shape, why, theta=None, pool="mixed", lazy=0, lzkind=None):
    return {"name": name, "entry": entry, "mode": mode, "shape": shape, "theta": theta, "pool": pool, "lazy": lazy, "lzkind": lzkind, "why": why}


def _cases():
    cs = []
    # ---- whole-node forward (eval and train form), every width
    for C in WIDTHS:
        for m in (2, 5, 4, 1):
            cs.append(_c("fwd_m%d_8x8_c%d" % (m, C), "fwd", m, (2, 8, 8, C), "operand set %d on one full tile" % m))
        cs.append(_c("fwd_m5_6x10_c%d" % C, "fwd", 5, (2, 6, 10, C), "ragged map: partial tiles in both directions"))
        cs.append(_c("fwd_m2_6x10_c%d" % C, "fwd", 2, (2, 6, 10, C), "ragged map, up operand"))
        cs.append(_c("fwd_m2_2x2_c%d" % C, "fwd", 2, (2, 2, 2, C), "map smaller than a tile"))
        cs.append(_c("fwd_m4_2x2_c%d" % C, "fwd", 4, (2, 2, 2, C), "map smaller than a tile, pooled operand"))
        cs.append(_c("fwd_m5_16x12_c%d" % C, "fwd", 5, (2, 16, 12, C), "several tiles: interior halos cross tiles"))
        cs.append(_c("fwd_m1_16x12_c%d" % C, "fwd", 1, (2, 16, 12, C), "several tiles, operand set 1"))
    # ---- fusion + depthwise launch, the unfused fusion
    for C in (48, 64, 112):
        for m in (2, 5, 4, 1):
            cs.append(_c("dw_m%d_6x10_c%d" % (m, C), "dw", m, (2, 6, 10, C), "%d channel chunk(s)%s" % (cdiv(C, 64), ", ragged" if C % 64 else "")))
    cs.append(_c("dw_m5_16x12_c112", "dw", 5, (2, 16, 12, 112), "several tiles"))
    # ---- the no-park kernel, by launch size
    cs.append(_c("nopark_b256_10x10", "eval", 2, (256, 10, 10, 112), "1024 blocks of ragged 2 x 2 tiles: no-park"))
    cs.append(_c("park_b255_10x10", "eval", 2, (255, 10, 10, 112), "1020 blocks: parked"))
    cs.append(_c("nopark_b1024_2x2", "eval", 2, (1024, 2, 2, 112), "1024 blocks of one partial tile: no-park"))
    cs.append(_c("park_b1023_2x2", "eval", 2, (1023, 2, 2, 112), "1023 blocks: parked"))
    # ---- theta edges
    for m, ths in ((5, {"neg": [0.7, -0.5, 0.4], "zero": [0.7, 0.0, 0.4], "one": [-1.0, 0.9, 0.0], "unequal": [1e-3, 5.0, 1.0]}),
                   (2, {"neg": [0.7, -0.5], "zero": [0.0, 1.3], "one": [-1.0, 0.9], "unequal": [1e-3, 5.0]})):
        for k, th in ths.items():
            cs.append(_c("theta_%s_m%d" % (k, m), "fwd", m, (2, 8, 8, 112), "theta %s" % th, theta=th))
    # ---- pool edges
    for m in (4, 5):
        cs.append(_c("poolneg_m%d" % m, "fwd", m, (2, 6, 10, 112), "pooled operand all negative: border windows take the padding zero", pool="neg"))
        cs.append(_c("poolpos_m%d" % m, "fwd", m, (2, 6, 10, 112), "pooled operand all positive", pool="pos"))
    # ---- grouped frozen nets
    for m in (2, 5):
        for C in (112, 64):
            cs.append(_c("group_m%d_c%d" % (m, C), "group", m, (GROUP_N * GROUP_IMAGES, 6, 10, C), "3 nets x 2 images"))
    # ---- lazy forward
    for C in (64, 112, 160):
        for m, masks in ((2, (0b0001, 0b0100, 0b0101)), (5, (0b0001, 0b0010, 0b1000, 0b1011)), (4, (0b0001, 0b1000, 0b1001))):
            for lz in masks:
                cs.append(_c("lazy_m%d_l%d_c%d" % (m, lz, C), "lazy", m, (2, 6, 10, C), "lazy mask %s" % bin(lz), lazy=lz))
    for m in (4, 5):
        cs.append(_c("lazy_padlose_m%d" % m, "lazy", m, (2, 6, 10, 112), "negative pooled source, large positive beta: in-image values exceed the padding zero",
                     lazy=0b1000, lzkind="padlose", pool="neg"))
        cs.append(_c("lazy_padwin_m%d" % m, "lazy", m, (2, 6, 10, 112), "large negative beta: the padding zero wins every border window",
                     lazy=0b1000, lzkind="padwin"))
    # ---- the stand-alone pool
    for PH, PW in ((7, 5), (1, 1), (2, 2), (9, 16)):
        for C in (4, 112):
            cs.append(_c("maxpool_%dx%d_c%d" % (PH, PW, C), "maxpool", 0, (2, PH, PW, C), "pad_lo %s" % ((same_pad_lo(PH, 3, 2)[1], same_pad_lo(PW, 3, 2)[1]),)))
    # ---- whole-node backward
    cs.append(_c("bf_m5_6x10_c64", "bwd_full", 5, (2, 6, 10, 64), "generic-K GEMM form, ragged map, pooled scatter"))
    cs.append(_c("bf_m2_6x10_c160", "bwd_full", 2, (2, 6, 10, 160), "generic-K GEMM form, C = 160, up operand on a ragged map"))
    cs.append(_c("bf_m4_2x2_c160", "bwd_full", 4, (2, 2, 2, 160), "generic-K GEMM form, map smaller than a tile"))
    cs.append(_c("bf_m4_2x2_c64", "bwd_full", 4, (2, 2, 2, 64), "generic-K GEMM form with the LDS fine tile"))
    cs.append(_c("bf_m5_8x8_c112_inactive", "bwd_full", 5, (2, 8, 8, 112), "an inactive theta entry", theta=[0.7, -0.5, 0.4]))
    cs.append(_c("bf_m5_8x8_c112_lazy", "bwd_full", 5, (2, 8, 8, 112), "lazy operands on every operand", lazy=0b1011))
    cs.append(_c("bf_m2_8x8_c64_lazy", "bwd_full", 2, (2, 8, 8, 64), "lazy operands on every operand", lazy=0b0101))
    cs.append(_c("bf_m2_4x4_c112", "bwd_full", 2, (2, 4, 4, 112), "NK 7, up operand"))
    cs.append(_c("bf_m4_2x2_c112", "bwd_full", 4, (2, 2, 2, 112), "NK 7, (in, pool)"))
    cs.append(_c("bf_m5_4x4_c224", "bwd_full", 5, (2, 4, 4, 224), "NK 14"))
    cs.append(_c("bf_m2_4x4_c224", "bwd_full", 2, (2, 4, 4, 224), "NK 14, up operand"))
    cs.append(_c("bf_m4_2x2_c224", "bwd_full", 4, (2, 2, 2, 224), "NK 14, (in, pool)"))
    # ---- generic operand sets of the two-launch backward
    for m in (1, 3, 6):
        for C in (48, 112):
            cs.append(_c("bd_m%d_c%d" % (m, C), "bwd_dw", m, (2, 6, 10, C), "generic operand set %d" % m))
    return cs


GROUP_N, GROUP_IMAGES = 3, 2
NODE_CASES = _cases()
CASE = {c["name"]: c for c in NODE_CASES}
assert len(CASE) == len(NODE_CASES)


def cases_of(*entries):
    return [c["name"] for c in NODE_CASES if c["entry"] in entries]


FAMILY = {"f": "fuse", "zd": "dw", "y": "eval", "z": "z", "stats": "sums", "pool": "pool", "dx": "opgrad", "d0": "opgrad", "d1": "opgrad",
          "dup": "opgrad", "dpl": "scatter", "wdot": "wdot", "dtheta": "dtheta", "dw_grad": "wgrad", "dz": "dz", "dgamma": "dgamma",
          "dbeta": "dgamma", "s0": "opsums", "s1": "opsums", "su": "opsums", "sp": "opsums"}
SLOT_KEY = {0: "in0", 1: "in1", 2: "up", 3: "pl"}
GRAD_KEY = {0: "d0", 1: "d1", 2: "dup", 3: "dpl"}
SUMS_KEY = {0: "s0", 1: "s1", 2: "su", 3: "sp"}


# ------------------------------------------------------------------------------------------------ inputs
def _gen(case, seed):
    B, H, W, C = case["shape"]
    mode, e = case["mode"], case["entry"]
    g = rng(41, B, H, W, C, mode * 64 + seed + 1000 * (sum(map(ord, case["name"])) % 97))
    rn = lambda *sh: torch.randn(*sh, generator=g)
    ru = lambda *sh: torch.rand(*sh, generator=g)
    if e == "maxpool":
        src = rn(B, H, W, C) - 0.5
        src[0, :, :, 0] = -src[0, :, :, 0].abs() - 0.1                   # a channel where every border window takes the padding zero
        return {"src": src}
    lazy = case["lazy"]
    d = {"in0": rn(B, H, W, C)}
    if mode & 1:
        d["in1"] = rn(B, H, W, C) * 1.2 + 0.1
    if mode & 2:
        d["up"] = rn(B, H // 2, W // 2, C)
    if mode & 4:
        p = rn(B, 2 * H, 2 * W, C) - 0.5
        if case["pool"] == "neg":
            p = -p.abs() - 0.05
        elif case["pool"] == "pos":
            p = p.abs() + 0.05
        elif not lazy & 8:
            # deliberate exact ties (a plain fp32 operand: the arg-max is exact in both precisions, the FIRST maximum takes the gradient):
            # rows 2oh and 2oh + 1 equal in every fourth channel; exact zeros on the last row / column that tie with the padding
            p[:, 1::2, :, 1::4] = p[:, 0::2, :, 1::4]
            p[:, -1, :, 2::4] = 0.0
            p[:, :, -1, 2::4] = 0.0
        d["pl"] = p
    for i in range(4):
        if lazy >> i & 1:
            x = d[SLOT_KEY[i]] * 1.7 + (0.0 if case["lzkind"] == "padlose" else 0.4)      # (padlose: the raw pooled source stays negative)
            d[SLOT_KEY[i]] = x
            rows = x.reshape(-1, C).double()
            stats = torch.cat([rows.sum(0), (rows * rows).sum(0)])
            gamma, beta = rn(C) * 0.8, rn(C) * 0.3                       # gamma of either sign: the max is taken AFTER the transform
            if case["lzkind"]:
                gamma = ru(C) * 0.5 + 0.25
                beta = (ru(C) + 1.0) * (4.0 if case["lzkind"] == "padlose" else -4.0)
            v, _ = bn_finalize(stats, rows.shape[0], gamma.double(), beta.double())
            d["lz%d" % i] = {"stats": stats, "gamma": gamma, "beta": beta, "count": rows.shape[0], "scale": v["scale"].float(),
                             "shift": v["shift"].float(), "mean": v["mean"].float(), "invstd": v["invstd"].float()}
    n = nops(mode)
    d["theta"] = torch.tensor(case["theta"] or THETA3[:n], dtype=torch.float32)
    if e == "group":
        ws, bs = C * C + 36, C + 20                                      # larger than any parameter block: a kernel that ignores them reads filler
        d["w_stride"], d["bn_stride"] = ws, bs
        d["theta_buf"] = ru(GROUP_N * ws) * 2 - 0.5
        d["w_dw_buf"], d["w_pw_buf"], d["bias_buf"] = rn(GROUP_N * ws) / 3, rn(GROUP_N * ws) / math.sqrt(C), rn(GROUP_N * ws) * 0.1
        d["scale_buf"], d["shift_buf"] = ru(GROUP_N * bs) + 0.5, rn(GROUP_N * bs) * 0.2
        return d
    d["w_dw"], d["w_pw"], d["bias"] = rn(9, C) / 3, rn(C, C) / math.sqrt(C), rn(C) * 0.1
    d["scale"], d["shift"] = ru(C) + 0.5, rn(C) * 0.2
    d["stats0"] = rn(2 * C).double() * 3
    if e in ("bwd_full", "bwd_dw"):
        M = B * H * W
        d["init"] = {"wdot": rn(4), "dw_grad": rn(9, C), "d0": rn(B, H, W, C) * 0.3, "dgamma": rn(C), "dbeta": rn(C)}
        if mode & 1:
            d["init"]["d1"] = rn(B, H, W, C) * 0.3
        if mode & 2:
            d["init"]["dup"] = rn(B, H // 2, W // 2, C) * 0.3
        if mode & 4:
            d["init"]["dpl"] = rn(B, 2 * H, 2 * W, C) * 0.3
        d["dtheta0"], d["wdot_in"] = rn(n), rn(n) * math.sqrt(M)          # mmd_bifpn_theta_bwd: its own inputs (the wdot contract)
        if e == "bwd_dw":
            d["dzd"] = rn(B, H, W, C)
        else:
            d["g"], d["z"] = rn(B, H, W, C), rn(B, H, W, C) * 1.2 + 0.1
            d["bn_scale"], d["bn_mean"], d["bn_invstd"] = ru(C) + 0.5, rn(C) * 0.2, ru(C) + 0.5
            d["bn_sums"], d["count"] = rn(2 * C).double() * math.sqrt(M), 2 * M + 1
            # BatchNorm inputs / statistics of the operands whose gradient the launch completes; a lazy operand IS its BatchNorm's input
            for i in op_indices(mode):
                x = d[SLOT_KEY[i]]
                if lazy >> i & 1:
                    d["bn%d" % i] = {"z": None, "mean": d["lz%d" % i]["mean"], "invstd": d["lz%d" % i]["invstd"]}
                else:
                    d["bn%d" % i] = {"z": torch.randn(x.shape, generator=g), "mean": rn(C) * 0.2, "invstd": ru(C) + 0.5}
                d["bn%d" % i]["sums0"] = rn(2 * C).double() * 3
    return d


def lazy_form(case):
    return "final" if case["entry"] in ("bwd_full", "bwd_dw") else "live"


def pool_gap(case, d):
    """The condition on a lazy pooled operand: in float64, the smallest distance between a window's best and second-best candidates (all
    padding taps = one candidate 0 of magnitude 0) in units of the larger |z*sc| + |sh| of the two.  The fp32 transform can flip a nearer
    tie, and with it the discrete arg-max the scattered gradient follows; None: no lazy pooled operand"""
    if not case["lazy"] & 8:
        return None
    sc, sh, _ = lazy_coef(_to(d["lz3"], torch.float64, "cpu"), torch.float64, lazy_form(case))
    x = d["pl"].double()
    taps, inside, _ = pool_taps(x * sc + sh)
    mags, _, _ = pool_taps((x * sc).abs() + sh.abs())
    ins = inside[:, None, :, :, None]
    first_pad = (~inside) & ((~inside).cumsum(0) == 1)
    drop = ((~inside) & ~first_pad)[:, None, :, :, None]
    v = torch.where(drop, torch.full_like(taps, -math.inf), torch.where(ins, taps, torch.zeros_like(taps)))
    m = torch.where(ins, mags, torch.zeros_like(mags))
    top, idx = v.topk(2, dim=0)
    mm = m.gather(0, idx).max(0)[0]
    return float(((top[0] - top[1]) / mm.clamp_min(1e-300)).min())


@functools.lru_cache(maxsize=None)
def _inputs(name):
    case = CASE[name]
    for seed in range(32):                                               # seeds are tried on the CPU until the arg-max condition holds
        d = _gen(case, seed)
        gap = pool_gap(case, d)
        if gap is None or gap > GAP:
            return d
    raise AssertionError("no seed gives %s a separated arg-max" % name)


def case_inputs(case):
    """fp32 (float64 for raw sums) CPU tensors of one case, the same for the CPU calibration and the GPU test; cached - do not modify"""
    return _inputs(case["name"])


def _coef(case, d, dt):
    return {i: lazy_coef(d["lz%d" % i], dt, lazy_form(case)) for i in range(4) if case["lazy"] >> i & 1} or None


def _bn_of(case, d):
    bn = {}
    for i in op_indices(case["mode"]):
        b = d["bn%d" % i]
        bn[i] = (d[SLOT_KEY[i]] if b["z"] is None else b["z"], b["mean"], b["invstd"], b["sums0"])
    return bn


def case_ref(case, inp, dt, dev="cpu", variant=None):
    """reference of one case in dtype dt -> {output name: (value, A)}.  variant: (acc, own) of the backward entries"""
    d = _to(inp, dt, dev)
    e, mode = case["entry"], case["mode"]
    B, H, W, C = case["shape"]
    if e == "maxpool":
        return {"pool": pool_same(d["src"])}
    if e == "dw":
        return node_dw(d, mode, d["theta"], d["w_dw"])
    if e == "eval":
        return node_eval(d, mode, d["theta"], d["w_dw"], d["w_pw"], d["bias"], d["scale"], d["shift"])
    if e == "fwd":
        out = node_eval(d, mode, d["theta"], d["w_dw"], d["w_pw"], d["bias"], d["scale"], d["shift"])
        out.update(node_train(d, mode, d["theta"], d["w_dw"], d["w_pw"], d["bias"], d["stats0"]))
        return out
    if e == "lazy":
        return node_train(d, mode, d["theta"], d["w_dw"], d["w_pw"], d["bias"], d["stats0"], _coef(case, d, dt))
    if e == "group":
        n = nops(mode)
        sizes = {"theta": (n,), "w_dw": (9, C), "w_pw": (C, C), "bias": (C,), "scale": (C,), "shift": (C,)}
        a = grouped(lambda o, p: node_eval(o, mode, p["theta"], p["w_dw"], p["w_pw"], p["bias"], p["scale"], p["shift"]), d, GROUP_N,
                    GROUP_IMAGES, list(sizes), d["w_stride"], d["bn_stride"], sizes)
        b = grouped(lambda o, p: node_dw(o, mode, p["theta"], p["w_dw"]), d, GROUP_N, GROUP_IMAGES, ["theta", "w_dw"], d["w_stride"],
                    d["bn_stride"], sizes)
        return {"y": a["y"], "f": b["f"], "zd": b["zd"]}
    acc, own = variant
    if e == "bwd_dw":
        out = fuse_bwd(d, mode, d["theta"], d["w_dw"], d["dzd"], d["dzd"].abs(), d["init"], acc, scatter=False)
    else:
        out = node_bwd_full(d, mode, d["theta"], d["w_dw"], d["init"], acc, d["g"], d["z"], d["bn_scale"], d["bn_mean"], d["bn_invstd"],
                            d["bn_sums"], d["count"], d["w_pw"], _coef(case, d, dt), _bn_of(case, d), own)
    out["dtheta"] = theta_bwd(d["theta"], d["wdot_in"], d["dtheta0"])
    return out


BWD_VARIANTS = [(0, 0), (1, 0), (1, 7)]          # (acc, own): overwrite; accumulate, sums of the total; accumulate, sums of this launch's share
