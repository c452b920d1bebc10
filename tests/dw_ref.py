"""Helper (not a test): float64 restatement of the four depthwise entry points of csrc/dwconv.hip - mmd_dwconv_fwd, mmd_dwconv_bwd_data,
mmd_dwconv_bwd_data_bn1, mmd_dwconv_bwd_weight - written from the formulas in the comments of dwconv.hip (DwArgs, the entry points'
contracts), not from the kernels' loops; a copy of the host dispatch (route); and the one case table (DW_CASES) that test_dw_ref_cpu.py
and test_gpu_dw_float64.py share.

Conventions are those of elt_ref.py.  Every reference computes in the dtype (and on the device) of its tensor arguments: float64 is the
oracle, float32 the "plain fp32" evaluation that calibrates K.  Tensors are NHWC, taps are tap-major [k*k, C].  The convolution is k*k
shifted multiply-adds under TF-SAME padding (same_pad_lo: extra = max(0, (ceil(n/s)-1)*s - n + k), low side extra // 2, so even sizes
at stride 2 pad asymmetrically).  Every reference returns (value, A), A_i the magnitude of what was summed into element i:
  * conv output / input gradient: sum_taps |w| * A_a, A_a the magnitude of the transformed input (its own rounding carried through, as
    elt_ref.affine_act does); a folded epilogue act(y*scale+shift) carries A_y on through elt_ref.act_fwd
  * BatchNorm sums, `bz` sums, weight gradients: sum |term| + |initial value| (the kernels accumulate)
  * squeeze-excite pool: sum |t| * pool_scale + |initial| + nblocks * 2^-36 (each block adds round(2^36 * partial mean); nblocks from route)
Errors are judged per element: |got - ref64| <= K * 2^-24 * A + tiny, K = max(8, 4 * K32) per family, K32 the largest error of the fp32
CPU evaluation over every (case, mode) of DW_CASES in the same unit (test_dw_ref_cpu.py measures it and asserts K32 <= K / 4).  No
constant comes from a GPU run of the kernels."""
import math

import torch
import torch.nn.functional as F

from elt_ref import swish, dswish, dswish_mag, act_fwd, ratio, rng, SENTINEL, f32, bn_finalize, cdiv, U, TINY      # noqa: F401

STATS_DEPTH = 128                    # MMD_STATS_DEPTH (common.h)
Q36 = 2.0 ** 36                      # MMD_POOL_Q

# K per family = max(8, 4 * K32).  K32 as test_dw_ref_cpu.py measures it (fp32 CPU evaluation of these references on every case):
K32 = {"conv": 4.725, "sums": 7.438, "bzsums": 2.218, "wgrad": 3.593, "pool": 4.098, "bn1_dx": 3.959, "bn1_dgamma": 1.734}
K_BY_FAMILY = {"conv": 19.0, "sums": 30.0, "bzsums": 9.0, "wgrad": 15.0, "pool": 17.0, "bn1_dx": 16.0, "bn1_dgamma": 8.0}


# ------------------------------------------------------------------------------------------------ geometry
def same_pad_lo(n, k, s):
    """-> (output size, low-side padding)"""
    o = cdiv(n, s)
    return o, max(0, (o - 1) * s - n + k) // 2


def _padded(a, k, s):
    """a [B, H, W, C] zero-padded to [(OH-1)*s + k, (OW-1)*s + k]; -> (padded, OH, OW, pad_t, pad_l)"""
    H, W = a.shape[1], a.shape[2]
    (OH, pt), (OW, pl) = same_pad_lo(H, k, s), same_pad_lo(W, k, s)
    HP, WP = (OH - 1) * s + k, (OW - 1) * s + k
    return F.pad(a, (0, 0, pl, WP - pl - W, pt, HP - pt - H)), OH, OW, pt, pl


def _win(i, n, s):
    return slice(i, i + (n - 1) * s + 1, s)


# ------------------------------------------------------------------------------------------------ references
def conv(a, Aa, w, k, s):
    """y[b,oh,ow,c] = sum_{i,j} w[i*k+j, c] * a[b, oh*s+i-pad_t, ow*s+j-pad_l, c]"""
    ap, OH, OW, _, _ = _padded(a, k, s)
    Ap = _padded(Aa, k, s)[0]
    y = A = 0
    for i in range(k):
        for j in range(k):
            y = y + ap[:, _win(i, OH, s), _win(j, OW, s)] * w[i * k + j]
            A = A + Ap[:, _win(i, OH, s), _win(j, OW, s)] * w[i * k + j].abs()
    return y, A


def conv_bwd_data(dy, Ady, w, H, W, k, s):
    """dx[b,ih,iw,c] = sum over (oh, i), (ow, j) with oh*s+i-pad_t == ih, ow*s+j-pad_l == iw of dy[b,oh,ow,c] * w[i*k+j, c]"""
    B, OH, OW, C = dy.shape
    (oh_, pt), (ow_, pl) = same_pad_lo(H, k, s), same_pad_lo(W, k, s)
    assert (oh_, ow_) == (OH, OW)
    HP, WP = max((OH - 1) * s + k, pt + H), max((OW - 1) * s + k, pl + W)
    dx, A = dy.new_zeros(B, HP, WP, C), dy.new_zeros(B, HP, WP, C)
    for i in range(k):
        for j in range(k):
            dx[:, _win(i, OH, s), _win(j, OW, s)] += dy * w[i * k + j]
            A[:, _win(i, OH, s), _win(j, OW, s)] += Ady * w[i * k + j].abs()
    return dx[:, pt:pt + H, pl:pl + W].contiguous(), A[:, pt:pt + H, pl:pl + W].contiguous()


def conv_bwd_weight(a, dy, k, s, dw0):
    """dw[i*k+j, c] = dw0 + sum_{b,oh,ow} dy[b,oh,ow,c] * a[b, oh*s+i-pad_t, ow*s+j-pad_l, c]"""
    ap, OH, OW, _, _ = _padded(a, k, s)
    rows, mags = [], []
    for i in range(k):
        for j in range(k):
            t = ap[:, _win(i, OH, s), _win(j, OW, s)] * dy
            rows.append(t.sum((0, 1, 2)))
            mags.append(t.abs().sum((0, 1, 2)))
    return dw0 + torch.stack(rows), dw0.abs() + torch.stack(mags)


def producer(x, sc, sh, A_sh, act):
    """a = act(x*sc+sh) (sc None: a = act(x)) and its magnitude"""
    if sc is None:
        return act_fwd(x, x.abs(), act)
    return act_fwd(x * sc + sh, (x * sc).abs() + (sh.abs() if A_sh is None else A_sh), act)


def bz_sums(dx, z, bsc, bsh, bmu, bis, sums0):
    """sums0 + [sum g, sum g*xhat], g = dx * swish'(z*bsc+bsh), xhat = (z-bmu)*bis"""
    g = dx * dswish(z * bsc + bsh)
    gx = g * ((z - bmu) * bis)
    d = (0, 1, 2)
    return (sums0 + torch.cat([g.sum(d), gx.sum(d)]).to(sums0.dtype),
            sums0.abs() + torch.cat([g.abs().sum(d), gx.abs().sum(d)]).to(sums0.dtype))


def dw_fwd(x, w, k, s, sc=None, sh=None, A_sh=None, in_act=0, osc=None, osh=None, out_act=0, stats0=None, pool0=None, nblocks=0):
    """mmd_dwconv_fwd: y = epi(dwconv_same(pro(x), w)); stats += [sum y, sum y^2] of the RAW conv output; pool += mean_hw of the stored y.
    pool0: float64 [B, C] = the Q36 integers / 2^36.  -> {"y", "stats", "pool"} of (value, A)"""
    a, Aa = producer(x, sc, sh, A_sh, in_act)
    y, Ay = conv(a, Aa, w, k, s)
    out = {}
    d = (0, 1, 2)
    if stats0 is not None:
        out["stats"] = (stats0 + torch.cat([y.sum(d), (y * y).sum(d)]).to(stats0.dtype),
                        stats0.abs() + torch.cat([y.abs().sum(d), (y * y).sum(d)]).to(stats0.dtype))
    t, At = y, Ay
    if osc is not None:
        t, At = y * osc + osh, Ay * osc.abs() + osh.abs()
    t, At = act_fwd(t, At, out_act)
    out["y"] = (t, At)
    if pool0 is not None:
        ps = f32(1.0 / (y.shape[1] * y.shape[2]))
        out["pool"] = (pool0 + (t.sum((1, 2)) * ps).to(pool0.dtype), pool0.abs() + (t.abs().sum((1, 2)) * ps).to(pool0.dtype) + nblocks / Q36)
    return out


def dw_bwd_data(dy, w, H, W, k, s, bn=None, sums0=None, dw0=None):
    """mmd_dwconv_bwd_data.  bn = (bn_z, scale, shift, mean, invstd): bn_sums += the `bz` sums of dx; dw0 given: dw_grad += the weight
    gradient of the forward conv whose input was a0 = swish(bn_z*scale+shift).  -> {"dx", "bn_sums", "dw_grad"}"""
    dx, A = conv_bwd_data(dy, dy.abs(), w, H, W, k, s)
    out = {"dx": (dx, A)}
    if bn is not None:
        out["bn_sums"] = bz_sums(dx, *bn, sums0)
        if dw0 is not None:
            out["dw_grad"] = conv_bwd_weight(swish(bn[0] * bn[1] + bn[2]), dy, k, s, dw0)
    return out


def dw_bwd_data_bn1(g1, z1, w, k, q_scale, q_shift, q_mean, q_invstd, q_sums, q_count, gate, add, bn, sums0, dw0, dgamma0=None, dbeta0=None):
    """mmd_dwconv_bwd_data_bn1 (stride 1): the conv's dY is the BatchNorm-1 (+swish, squeeze-excite) backward of DwArgs,
        dz1 = scale*(g' - m1 - xhat*m2),  g' = (g1*gate[img,c] + add[img,c]) * swish'(z1*scale+shift),  xhat = (z1-mean)*invstd,
        [m1, m2] = q_sums / q_count   (q_sums: the float64 numbers the kernel receives; m1, m2 take the tensors' dtype)
    then dx, bn_sums and dw_grad as dw_bwd_data(dz1, ..., bn, dw_grad).  q_dgamma / q_dbeta ACCUMULATE (a plain, non-atomic +=):
    q_dgamma[c] += (float) q_sums[C + c], q_dbeta[c] += (float) q_sums[c], written once per channel by the blocks of image 0's first tile
    (b == 0, th == 0, tw == 0: one block per 64-channel chunk).  -> {"dx", "bn_sums", "dw_grad", "q_dgamma", "q_dbeta"}"""
    B, H, W, C = g1.shape
    dt = g1.dtype
    m1, m2 = (q_sums[:C] / float(q_count)).to(dt), (q_sums[C:] / float(q_count)).to(dt)
    u = z1 * q_scale + q_shift
    gt, ad = gate.view(B, 1, 1, C), add.view(B, 1, 1, C)
    gp = (g1 * gt + ad) * dswish(u)
    Agp = ((g1 * gt).abs() + ad.abs()) * dswish_mag(u, (z1 * q_scale).abs() + q_shift.abs())
    xh = (z1 - q_mean) * q_invstd
    dz = q_scale * (gp - m1 - xh * m2)
    Adz = q_scale.abs() * (Agp + m1.abs() + (xh * m2).abs())
    dx, A = conv_bwd_data(dz, Adz, w, H, W, k, 1)
    out = {"dx": (dx, A), "bn_sums": bz_sums(dx, *bn, sums0), "dw_grad": conv_bwd_weight(swish(bn[0] * bn[1] + bn[2]), dz, k, 1, dw0)}
    if dgamma0 is not None:
        out["q_dgamma"] = (dgamma0 + q_sums[C:].to(dt), dgamma0.abs() + q_sums[C:].abs().to(dt))
        out["q_dbeta"] = (dbeta0 + q_sums[:C].to(dt), dbeta0.abs() + q_sums[:C].abs().to(dt))
    return out


def dw_bwd_weight(x, dy, k, s, dw0, sc=None, sh=None, in_act=0):
    """mmd_dwconv_bwd_weight: dw += sum dy * pro(x)[shifted]"""
    return conv_bwd_weight(producer(x, sc, sh, None, in_act)[0], dy, k, s, dw0)


# ------------------------------------------------------------------------------------------------ the dispatch, copied
def _rows_geom(B, H, W, C, LW, R):
    cch, colblocks = cdiv(C, 4 * LW), cdiv(W, (256 // LW) * R)
    per_row = B * cch * colblocks
    rh = min(max(H * per_row // 1024, 4), H)
    rowblocks = cdiv(H, rh)
    return {"R": R, "LW": LW, "cchunks": cch, "colblocks": colblocks, "rh": rh, "rowblocks": rowblocks, "last_rows": H - (rowblocks - 1) * rh,
            "blocks": per_row * rowblocks, "last_chunk_quads": (C - (cch - 1) * 4 * LW) // 4}


def _rows(B, H, W, C, pro, stats, out, bz, ws_slots):
    """dw3_rows_launch / dw3_rows_go; None: left to the tile kernel"""
    if stats and out:
        return None
    lw = 4 if C <= 16 else (8 if C <= 32 else 16)
    strips = 256 // lw
    if pro and C > 64 and (C & 63):
        return None
    if W >= 4 * strips:
        R = 4
    elif pro or lw != 16:
        return None
    elif W >= 32:
        R = 2
    elif W >= 16:
        R = 1
    else:
        return None
    r = _rows_geom(B, H, W, C, lw, R)
    r.update(kernel="dw3_rows", PRO=int(pro), EPI=2 if bz else (1 if stats else (3 if out else 0)), WG=False,
             slotted=bool(stats and ws_slots >= 2 and r["blocks"] // r["cchunks"] > STATS_DEPTH), pool_blocks=r["rowblocks"] * r["colblocks"])
    return r


def _tile(B, OH, OW, C, K, S, LANES, pro, stats, out, bz, dwg, bn1, ws_slots):
    """dw_fwd_launch<K, S, LANES>"""
    TH = 8 if S == 1 else 4
    tiles, cch = cdiv(OH, TH) * cdiv(OW, 8), cdiv(C, 4 * LANES)
    epi = 4 if (stats and out) else (2 if bz else (1 if stats else (3 if out else 0)))
    PRO, WG = int(pro), False
    if bn1:
        assert S == 1 and LANES >= 8 and dwg and epi == 2 and not pro
        PRO, WG = 2, True
    elif dwg:
        assert S == 1 and epi == 2 and not pro
        WG = True
    return {"kernel": "dw_fwd", "K": K, "S": S, "LANES": LANES, "PRO": PRO, "EPI": epi, "WG": WG, "tiles": tiles, "cchunks": cch,
            "blocks": B * tiles * cch, "slotted": bool(stats and ws_slots >= 2 and B * tiles > STATS_DEPTH), "pool_blocks": tiles,
            "last_chunk_quads": (C - (cch - 1) * 4 * LANES) // 4}


def _lanes31(C):
    return 4 if C <= 16 else (8 if C <= 32 else 16)


def route(entry, B, H, W, C, k, s, pro=False, sums=False, out=False, bn=False, dwg=False, ws_slots=0):
    """Which kernel instantiation and geometry a call reaches: a COPY of the host dispatch of dwconv.hip (dw3_rows_launch / dw3_rows_go,
    dw_fwd_launch_31 / _51, dw_fwd_launch, the stride-2 branch of mmd_dwconv_bwd_data, dw3_wgrad_rows_launch / _go, dw_wgrad_launch), with
    no MMD_DW_* variable set.  Nothing checks the copy against the host code: keep it in step by hand when the dispatch changes.
    entry: "fwd" (pro / sums / out = folded epilogue, activation or pool), "bwd_data" (bn = bn_sums given, dwg = dw_grad given), "bn1",
    "bwd_weight" (pro)."""
    OH, OW = same_pad_lo(H, k, s)[0], same_pad_lo(W, k, s)[0]
    if entry == "fwd":
        r = _rows(B, H, W, C, pro, sums, out, False, ws_slots) if (k, s) == (3, 1) else None
        return r or _tile(B, OH, OW, C, k, s, _lanes31(C) if (k, s) == (3, 1) else 16, pro, sums, out, False, False, False, ws_slots)
    if entry == "bn1":
        return _tile(B, H, W, C, k, 1, 16, False, True, False, True, True, True, ws_slots)
    if entry == "bwd_data" and s == 1:
        r = _rows(B, H, W, C, False, bn, False, bn, ws_slots) if (k == 3 and not dwg) else None
        return r or _tile(B, H, W, C, k, 1, _lanes31(C) if k == 3 else 16, False, bn, False, bn, dwg, False, ws_slots)
    if entry == "bwd_data":
        if not bn:
            return {"kernel": "s2_plain", "K": k, "blocks": cdiv(B * H * W * (C // 4), 256)}
        cch = cdiv(C, 64)
        rpb = max(cdiv(B * H * cch, 2048), 2)
        rpb += rpb & 1
        clamped = rpb > H
        if clamped:
            rpb = H + (H & 1)
        rbl = cdiv(H, rpb)
        return {"kernel": "s2_sums", "K": k, "WG": bool(dwg), "rpb": rpb, "rbl": rbl, "rpb_clamped": clamped, "last_rows": H - (rbl - 1) * rpb,
                "cchunks": cch, "blocks": B * rbl * cch, "slotted": bool(ws_slots > 1 and B * rbl > STATS_DEPTH),
                "last_chunk_quads": (C - (cch - 1) * 64) // 4}
    assert entry == "bwd_weight"
    if (k, s) == (3, 1) and C <= 32 and W >= 256:
        r = _rows_geom(B, H, W, C, 8 if C > 16 else 4, 4)
        r.update(kernel="dw3_wgrad_rows", PRO=int(pro))
        return r
    TH = 8 if s == 1 else 4
    ntiles, cch = cdiv(OH, TH) * cdiv(OW, 8), cdiv(C, 64)
    want = cdiv(2048, B * cch)
    return {"kernel": "dw_wgrad", "K": k, "S": s, "PRO": int(pro), "ntiles": ntiles, "nsplit": max(1, min(want, ntiles)),
            "clamp": "ntiles" if want > ntiles else ("exact" if want == ntiles else "blocks"), "cchunks": cch,
            "last_chunk_quads": (C - (cch - 1) * 64) // 4}


# ------------------------------------------------------------------------------------------------ cases
# forward modes: (pro, epi, ws_slots).  pro: none | given (scale, shift, swish) | live (in_stats, swish) | act (swish only) | affine (scale,
# shift, no activation).  epi: "0" raw | "1" sums | "3" out_scale + swish + pool | "3a" swish only, no pool | "4" sums + out_scale + swish + pool
def _m(pros, epis, slots=0):
    return [(p, e, slots) for p in pros for e in epis]


PEL = _m(("none", "given", "live"), ("0", "1", "3", "4"))            # the PRO x EPI lattice
PEL_X = PEL + [("act", "3a", 0), ("affine", "1", 0)]
BWD_S1 = [("plain", 0), ("bn", 0), ("bnwg", 0)]
BWD_S2 = [("bn", 0), ("bnwg", 0)]


def _c(name, entry, shape, k, s, modes, why):
    return {"name": name, "entry": entry, "shape": shape, "k": k, "s": s, "modes": modes, "why": why}


DW_CASES = [
    # ---- rows kernel, rh > 4: the rolling window rolls
    _c("rows_r1_rh5", "fwd", (4, 81, 16, 1024), 3, 1, [("none", "0", 0)], "dw3_rows<1,16> PRO 0 EPI 0, rh 5, last row block 1 row"),
    _c("rows_r1_rh6", "fwd", (4, 100, 16, 1024), 3, 1, [("none", "1", 0)], "dw3_rows<1,16> EPI 1, rh 6"),
    _c("rows_r1_rh7", "fwd", (4, 115, 16, 1024), 3, 1, [("none", "3", 0)], "dw3_rows<1,16> EPI 3 (out_scale, swish, pool), rh 7"),
    _c("rows_r1_rh9", "fwd", (4, 150, 16, 1024), 3, 1, [("none", "1", 0)], "dw3_rows<1,16> EPI 1, rh 9: a third loop iteration"),
    _c("rows_r2_rh5", "fwd", (4, 83, 32, 1020), 3, 1, [("none", "1", 0), ("none", "3", 0)], "dw3_rows<2,16>, rh 5, ragged last chunk"),
    _c("rows_bwd_rh6", "bwd_data", (4, 100, 16, 1024), 3, 1, [("bn", 0)], "dw3_rows<1,16> flipped, EPI 2, rh 6: the za / zb rotation"),
    _c("rows_bwd_rh5", "bwd_data", (4, 81, 16, 1024), 3, 1, [("plain", 0)], "dw3_rows<1,16> flipped, EPI 0, rh 5"),
    _c("rows_r4_pro_rh5", "fwd", (4, 88, 64, 960), 3, 1, [("given", "1", 0), ("live", "1", 0)], "dw3_rows<4,16> PRO 1 EPI 1, rh 5, given and live"),
    _c("wgrad_rows_rh5", "bwd_weight", (8, 641, 256, 16), 3, 1, [True], "dw3_wgrad_rows<4,4> PRO, rh 5, last row block 1 row"),
    # ---- rows kernel, maps lower than 4 rows (rh == H) and the W / C thresholds
    _c("rows_h1", "fwd", (2, 1, 16, 64), 3, 1, _m(("none",), ("0", "1", "3")), "dw3_rows<1,16> rh = H = 1"),
    _c("rows_h2", "fwd", (2, 2, 16, 64), 3, 1, _m(("none",), ("0", "1", "3")), "dw3_rows<1,16> rh = H = 2"),
    _c("rows_h3", "fwd", (2, 3, 16, 64), 3, 1, _m(("none",), ("0", "1", "3")), "dw3_rows<1,16> rh = H = 3"),
    _c("rows_h3_r4", "fwd", (2, 3, 70, 80), 3, 1, _m(("none",), ("0", "1", "3", "3a")), "dw3_rows<4,16> rh = H = 3, two column blocks, ragged chunk"),
    _c("rows_h2_pro", "fwd", (2, 2, 70, 64), 3, 1, _m(("given", "live", "act", "affine"), ("0", "1", "3")), "dw3_rows<4,16> PRO 1, rh = H = 2"),
    _c("w15", "fwd", (2, 5, 15, 68), 3, 1, _m(("none",), ("0", "1", "3")), "W 15 < 16: tile LANES 16"),
    _c("w16", "fwd", (2, 5, 16, 68), 3, 1, _m(("none",), ("0", "1", "3")), "W 16: dw3_rows<1,16>, last chunk one quad, second row block of 1 row"),
    _c("w31", "fwd", (2, 5, 31, 68), 3, 1, _m(("none",), ("0", "1", "3")), "W 31: dw3_rows<1,16>, two column blocks"),
    _c("w32", "fwd", (2, 5, 32, 68), 3, 1, _m(("none",), ("0", "1", "3")), "W 32: dw3_rows<2,16>, last chunk one quad"),
    _c("w63", "fwd", (2, 5, 63, 68), 3, 1, _m(("none",), ("0", "1", "3")), "W 63: dw3_rows<2,16>, two column blocks"),
    _c("w64", "fwd", (2, 5, 64, 68), 3, 1, _m(("none",), ("0", "1", "3")), "W 64: dw3_rows<4,16>, last chunk one quad"),
    _c("w63_pro", "fwd", (2, 5, 63, 64), 3, 1, _m(("given",), ("0", "1", "3")), "W 63 with a producer: tile"),
    _c("w127_c24", "fwd", (2, 5, 127, 24), 3, 1, _m(("none", "given"), ("0", "1", "3")), "C 24, W 127 < 128: tile LANES 8"),
    _c("w128_c24", "fwd", (2, 5, 128, 24), 3, 1, _m(("none", "given"), ("0", "1", "3")), "C 24, W 128: dw3_rows<4,8>"),
    _c("w255_c12", "fwd", (2, 5, 255, 12), 3, 1, _m(("none", "given"), ("0", "1", "3")), "C 12, W 255 < 256: tile LANES 4"),
    _c("w256_c12", "fwd", (2, 5, 256, 12), 3, 1, _m(("none", "given"), ("0", "1", "3")), "C 12, W 256: dw3_rows<4,4>"),
    _c("c144_pro", "fwd", (2, 6, 64, 144), 3, 1, _m(("given", "live"), ("0", "1", "3")), "producer and C = 144: tile"),
    _c("c128_pro", "fwd", (2, 6, 64, 128), 3, 1, _m(("given", "live"), ("0", "1", "3")), "producer and C = 128: dw3_rows<4,16> PRO 1"),
    _c("lw8_ragged", "fwd", (2, 9, 131, 24), 3, 1, _m(("none", "given", "live"), ("0", "1", "3")), "dw3_rows<4,8>, W no multiple of the column block"),
    _c("lw4_ragged", "fwd", (2, 6, 259, 12), 3, 1, _m(("none", "given", "live"), ("0", "1", "3")), "dw3_rows<4,4>, W no multiple of the column block"),
    # ---- tile kernel: PRO x EPI
    _c("t31_c12", "fwd", (2, 13, 9, 12), 3, 1, PEL_X, "dw_fwd<3,1,4>: the lattice"),
    _c("t31_c28", "fwd", (2, 13, 9, 28), 3, 1, PEL_X, "dw_fwd<3,1,8>: the lattice"),
    _c("t31_c68", "fwd", (2, 13, 9, 68), 3, 1, PEL_X, "dw_fwd<3,1,16>: the lattice, last chunk one quad"),
    _c("t31_1x1_c12", "fwd", (2, 1, 1, 12), 3, 1, PEL, "dw_fwd<3,1,4> on a 1x1 map"),
    _c("t31_1x1_c28", "fwd", (2, 1, 1, 28), 3, 1, PEL, "dw_fwd<3,1,8> on a 1x1 map"),
    _c("t31_1x1_c68", "fwd", (2, 1, 1, 68), 3, 1, PEL, "dw_fwd<3,1,16> on a 1x1 map"),
    _c("t31_c144_pro", "fwd", (2, 24, 70, 144), 3, 1, _m(("given", "live"), ("0", "1", "3")), "dw_fwd<3,1,16> PRO 1 where the rows kernel refuses C = 144"),
    _c("t31_epi4", "fwd", (2, 18, 40, 64), 3, 1, _m(("none", "given", "live"), ("4",)), "sums + folded epilogue: EPI 4, tile only"),
    _c("t51", "fwd", (2, 16, 16, 144), 5, 1, PEL_X, "dw_fwd<5,1,16>: the lattice"),
    _c("t51_h1", "fwd", (2, 1, 7, 20), 5, 1, PEL, "dw_fwd<5,1,16>, one row"),
    _c("t32", "fwd", (2, 16, 16, 96), 3, 2, PEL_X, "dw_fwd<3,2>: even sizes (asymmetric padding)"),
    _c("t32_odd", "fwd", (2, 9, 7, 16), 3, 2, PEL, "dw_fwd<3,2>: odd sizes"),
    _c("t32_1x1", "fwd", (2, 1, 1, 4), 3, 2, PEL, "dw_fwd<3,2> on a 1x1 map"),
    _c("t52", "fwd", (2, 17, 12, 48), 5, 2, PEL_X, "dw_fwd<5,2>: odd H, even W"),
    _c("t52_big", "fwd", (2, 32, 32, 240), 5, 2, PEL, "dw_fwd<5,2>: four chunks, 32 tiles"),
    _c("t51_slotted", "fwd", (2, 72, 72, 20), 5, 1, [("none", "1", 8), ("given", "1", 8), ("live", "4", 8)], "dw_fwd<5,1,16>: 2 x 81 tiles > 128, slotted sums"),
    # ---- stride-1 input gradient, tile kernel (EPI 2, WG) and small rows forms
    _c("b31_c12", "bwd_data", (2, 13, 9, 12), 3, 1, BWD_S1, "dw_fwd<3,1,4> flipped: EPI 0 / 2 / 2 + WG"),
    _c("b31_c28", "bwd_data", (2, 13, 9, 28), 3, 1, BWD_S1, "dw_fwd<3,1,8> flipped"),
    _c("b31_c68", "bwd_data", (2, 13, 9, 68), 3, 1, BWD_S1, "dw_fwd<3,1,16> flipped"),
    _c("b31_1x1", "bwd_data", (2, 1, 1, 68), 3, 1, BWD_S1, "dw_fwd<3,1,16> flipped on a 1x1 map"),
    _c("b31_c144", "bwd_data", (2, 24, 70, 144), 3, 1, BWD_S1, "rows<4,16> EPI 0 / 2 without dw_grad, tile WG with it"),
    _c("b51", "bwd_data", (2, 16, 16, 144), 5, 1, BWD_S1, "dw_fwd<5,1,16> flipped"),
    _c("b51_h1", "bwd_data", (2, 1, 7, 20), 5, 1, BWD_S1, "dw_fwd<5,1,16> flipped, one row"),
    _c("b51_slotted", "bwd_data", (2, 72, 72, 20), 5, 1, [("bn", 8), ("bnwg", 8)], "dw_fwd<5,1,16> flipped, slotted `bz` sums"),
    # ---- stride-2 input gradient
    _c("s2_rpb4_k3", "bwd_data", (9, 130, 6, 256), 3, 2, BWD_S2, "s2_sums<3>: rpb 4, rbl 33, last block 2 rows"),
    _c("s2_rpb4_k5", "bwd_data", (9, 130, 6, 256), 5, 2, BWD_S2, "s2_sums<5>: rpb 4"),
    _c("s2_h1_k3", "bwd_data", (2, 1, 9, 20), 3, 2, BWD_S2, "s2_sums<3>: rpb 2 > H = 1"),
    _c("s2_h1_k5", "bwd_data", (2, 1, 9, 20), 5, 2, BWD_S2, "s2_sums<5>: rpb 2 > H = 1"),
    _c("s2_h3_k3", "bwd_data", (2, 3, 5, 68), 3, 2, BWD_S2, "s2_sums<3>: odd H and W, last block one row, last chunk one quad"),
    _c("s2_h3_k5", "bwd_data", (2, 3, 5, 68), 5, 2, BWD_S2, "s2_sums<5>: odd H and W"),
    _c("s2_h3_clamp", "bwd_data", (64, 3, 5, 1348), 5, 2, BWD_S2, "s2_sums<5>: rpb 4 > H = 3, clamped to H + 1"),
    _c("s2_slotted", "bwd_data", (2, 262, 5, 16), 5, 2, [("bn", 8), ("bnwg", 8)], "s2_sums<5>: B * rbl = 262 > 128, slotted"),
    _c("s2_even_k3", "bwd_data", (2, 16, 16, 96), 3, 2, [("plain", 0)] + BWD_S2, "even H and W"),
    _c("s2_odd_k3", "bwd_data", (2, 9, 7, 16), 3, 2, [("plain", 0)] + BWD_S2, "odd H and W"),
    _c("s2_k5", "bwd_data", (2, 17, 12, 48), 5, 2, [("plain", 0)] + BWD_S2, "odd H, even W; the plain gather"),
    _c("s2_plain_k3", "bwd_data", (2, 17, 12, 48), 3, 2, [("plain", 0)], "the plain gather, k 3"),
    _c("s2_1x1_k3", "bwd_data", (2, 1, 1, 4), 3, 2, [("plain", 0)] + BWD_S2, "1x1 map"),
    _c("s2_1x1_k5", "bwd_data", (2, 1, 1, 4), 5, 2, [("plain", 0)] + BWD_S2, "1x1 map"),
    # ---- BatchNorm-1 backward in the prologue
    _c("bn1_k3_c64", "bn1", (2, 9, 7, 64), 3, 1, [True, False], "dw_fwd<3,1,16,2,2,WG>"),
    _c("bn1_k5_c64", "bn1", (2, 9, 7, 64), 5, 1, [True, False], "dw_fwd<5,1,16,2,2,WG>"),
    _c("bn1_k3_c144", "bn1", (2, 16, 12, 144), 3, 1, [True, False], "three chunks, ragged"),
    _c("bn1_k5_c144", "bn1", (2, 16, 12, 144), 5, 1, [True, False], "three chunks, ragged"),
    _c("bn1_k3_c528", "bn1", (3, 5, 9, 528), 3, 1, [True, False], "nine chunks, last of one quad; three images"),
    _c("bn1_k5_c528", "bn1", (3, 5, 9, 528), 5, 1, [True, False], "nine chunks, last of one quad; three images"),
    _c("bn1_k3_c68", "bn1", (2, 9, 7, 68), 3, 1, [True], "last chunk of one quad"),
    # ---- weight gradient
    _c("wg31", "bwd_weight", (2, 13, 9, 68), 3, 1, [True, False], "dw_wgrad<3,1>: nsplit clamped to ntiles"),
    _c("wg51", "bwd_weight", (2, 16, 16, 144), 5, 1, [True, False], "dw_wgrad<5,1>"),
    _c("wg32", "bwd_weight", (2, 16, 16, 96), 3, 2, [True, False], "dw_wgrad<3,2>"),
    _c("wg52", "bwd_weight", (2, 17, 12, 48), 5, 2, [True, False], "dw_wgrad<5,2>"),
    _c("wg_1x1", "bwd_weight", (2, 1, 1, 4), 5, 2, [True, False], "dw_wgrad<5,2> on a 1x1 map"),
    _c("wg32_split", "bwd_weight", (32, 9, 17, 1348), 3, 2, [True, False], "dw_wgrad<3,2>: nsplit = cdiv(2048, B*cchunks) = 3 < 4 tiles"),
    _c("wg51_split", "bwd_weight", (32, 9, 17, 1348), 5, 1, [True], "dw_wgrad<5,1>: nsplit 3 < 6 tiles"),
    _c("wg_rows_lw8", "bwd_weight", (2, 5, 256, 24), 3, 1, [True, False], "dw3_wgrad_rows<4,8>, rh 4, last row block 1 row"),
    _c("wg_rows_lw4", "bwd_weight", (2, 3, 259, 12), 3, 1, [True, False], "dw3_wgrad_rows<4,4>, rh = H = 3, two column blocks"),
]
CASE = {c["name"]: c for c in DW_CASES}
assert len(CASE) == len(DW_CASES)

# group mode of mmd_dwconv_fwd: (name, shape, k, s, pro, why); n = 3 nets, 2 images each
GROUP_N, GROUP_IMAGES = 3, 2
GROUP_CASES = [("group_rows", (6, 18, 40, 64), 3, 1, "none", "dw3_rows<2,16> EPI 3 + pool, three groups"),
               ("group_tile", (6, 17, 12, 48), 5, 2, "given", "dw_fwd<5,2> PRO 1 EPI 3 + pool, three groups")]

EPI_FLAGS = {"0": (False, False), "1": (True, False), "3": (False, True), "3a": (False, True), "4": (True, True)}


def route_mode(case, mode):
    B, H, W, C = case["shape"]
    k, s, e = case["k"], case["s"], case["entry"]
    if e == "fwd":
        pro, epi, slots = mode
        sums, out = EPI_FLAGS[epi]
        return route("fwd", B, H, W, C, k, s, pro=pro != "none", sums=sums, out=out, ws_slots=slots)
    if e == "bwd_data":
        kind, slots = mode
        return route("bwd_data", B, H, W, C, k, s, bn=kind != "plain", dwg=kind == "bnwg", ws_slots=slots)
    if e == "bn1":
        return route("bn1", B, H, W, C, k, 1)
    return route("bwd_weight", B, H, W, C, k, s, pro=mode)


# ------------------------------------------------------------------------------------------------ inputs
def _bn_of(g, x, C):
    """gamma, beta, float64 raw sums of x's rows and the fp32 (scale, shift, mean, invstd) bn_finalize gives; below 32 rows the sums are
    those of a 64-row batch that x is the head of (as elt_ref.bn_inputs: no degenerate statistics)"""
    rows = x.reshape(-1, C)
    if rows.shape[0] < 32:
        rows = torch.cat([rows, torch.randn(64 - rows.shape[0], C, generator=g) * 1.7 + 0.3])
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    r64 = rows.double()
    stats = torch.cat([r64.sum(0), (r64 * r64).sum(0)])
    v, _ = bn_finalize(stats, rows.shape[0], gamma.double(), beta.double())
    return {"gamma": gamma, "beta": beta, "stats": stats, "count": rows.shape[0], **{k: t.float() for k, t in v.items()}}


def case_inputs(case):
    """fp32 (float64 for the raw sums, int64 for the pool) CPU tensors of one case; the same for the CPU calibration and the GPU test"""
    B, H, W, C = case["shape"]
    k, s, e = case["k"], case["s"], case["entry"]
    g = rng(21, B, H, W, C, k * 2 + s)
    rn = lambda *sh: torch.randn(*sh, generator=g)
    OH, OW = same_pad_lo(H, k, s)[0], same_pad_lo(W, k, s)[0]
    d = {"w": rn(k * k, C) / k}
    if e in ("fwd", "bwd_weight"):
        d["x"] = rn(B, H, W, C) * 1.7 + 0.3
        d["bn"] = _bn_of(g, d["x"], C)
    if e == "fwd":
        d["osc"], d["osh"] = torch.rand(C, generator=g) + 0.5, rn(C) * 0.2
        d["stats0"] = rn(2 * C).double() * 3
        d["pool0"] = (rn(B, C).double() * 0.5 * Q36).round().to(torch.int64)
    if e == "bwd_weight":
        d["dy"], d["dw0"] = rn(B, OH, OW, C), rn(k * k, C)
    if e in ("bwd_data", "bn1"):
        d["bn_z"] = rn(B, H, W, C) * 1.7 + 0.3
        d["bn"] = _bn_of(g, d["bn_z"], C)
        d["sums0"], d["dw0"] = rn(2 * C).double() * 3, rn(k * k, C)
    if e == "bwd_data":
        d["dy"] = rn(B, OH, OW, C)
    if e == "bn1":
        d["g1"], d["z1"] = rn(B, H, W, C), rn(B, H, W, C) * 1.7 + 0.3
        d["q"] = _bn_of(g, d["z1"], C)
        d["gate"], d["add"] = torch.rand(B, C, generator=g) * 0.9 + 0.05, rn(B, C) * 0.1
        n = B * H * W
        d["q_sums"], d["q_count"] = rn(2 * C).double() * math.sqrt(n), 2 * n + 1
        d["dgamma0"], d["dbeta0"] = rn(C), rn(C)
    return d


def _to(d, dt, dev):
    """float tensors of a (nested) input dict in dtype dt on dev; float64 / int64 tensors keep their type"""
    out = {}
    for key, t in d.items():
        if isinstance(t, dict):
            out[key] = _to(t, dt, dev)
        elif isinstance(t, torch.Tensor):
            out[key] = t.to(dev) if t.dtype != torch.float32 else t.to(dev, dt)
        else:
            out[key] = t
    return out


def _pro_args(d, pro):
    """(scale, shift, A_shift, in_act) of a forward / weight-gradient producer in the dtype of d"""
    bn = d["bn"]
    if pro == "given":
        return bn["scale"], bn["shift"], None, 1
    if pro == "affine":
        return bn["scale"], bn["shift"], None, 0
    if pro == "act":
        return None, None, None, 1
    if pro == "live":
        v, m = bn_finalize(bn["stats"], bn["count"], bn["gamma"], bn["beta"])
        return v["scale"], v["shift"], m["shift"], 1
    return None, None, None, 0


def case_ref(case, mode, inp, dt, dev="cpu"):
    """reference of one (case, mode) in dtype dt -> {output name: (value, A)}"""
    B, H, W, C = case["shape"]
    k, s, e = case["k"], case["s"], case["entry"]
    d = _to(inp, dt, dev)
    r = route_mode(case, mode)
    if e == "fwd":
        pro, epi, _ = mode
        sums, out = EPI_FLAGS[epi]
        sc, sh, ash, act = _pro_args(d, pro)
        full = out and epi != "3a"
        return dw_fwd(d["x"], d["w"], k, s, sc, sh, ash, act, d["osc"] if full else None, d["osh"] if full else None, 1 if out else 0,
                      d["stats0"] if sums else None, d["pool0"].double() / Q36 if full else None, r["pool_blocks"])
    bn = d["bn"] if "bn" in d else None
    if e == "bwd_data":
        kind = mode[0]
        bnt = (d["bn_z"], bn["scale"], bn["shift"], bn["mean"], bn["invstd"]) if kind != "plain" else None
        return dw_bwd_data(d["dy"], d["w"], H, W, k, s, bnt, d["sums0"], d["dw0"] if kind == "bnwg" else None)
    if e == "bn1":
        q = d["q"]
        return dw_bwd_data_bn1(d["g1"], d["z1"], d["w"], k, q["scale"], q["shift"], q["mean"], q["invstd"], d["q_sums"], d["q_count"], d["gate"],
                               d["add"], (d["bn_z"], bn["scale"], bn["shift"], bn["mean"], bn["invstd"]), d["sums0"], d["dw0"],
                               d["dgamma0"] if mode else None, d["dbeta0"] if mode else None)
    sc, sh, _, act = _pro_args(d, "given" if mode else "none")
    return {"dw": dw_bwd_weight(d["x"], d["dy"], k, s, d["dw0"], sc, sh, act)}


FAMILY = {("fwd", "y"): "conv", ("fwd", "stats"): "sums", ("fwd", "pool"): "pool",
          ("bwd_data", "dx"): "conv", ("bwd_data", "bn_sums"): "bzsums", ("bwd_data", "dw_grad"): "wgrad",
          ("bn1", "dx"): "bn1_dx", ("bn1", "bn_sums"): "bzsums", ("bn1", "dw_grad"): "wgrad", ("bn1", "q_dgamma"): "bn1_dgamma",
          ("bn1", "q_dbeta"): "bn1_dgamma", ("bwd_weight", "dw"): "wgrad"}


def mode_label(mode):
    return "-".join(str(int(m) if isinstance(m, bool) else m) for m in mode) if isinstance(mode, tuple) else ("on" if mode else "off")


# ------------------------------------------------------------------------------------------------ group mode
def group_inputs(shape, k, s):
    """three nets' taps and folded coefficients inside flat buffers a stride apart (the strides are larger than the parameter blocks:
    a kernel that ignores them reads the filler)"""
    B, H, W, C = shape
    g = rng(22, B, H, W, C, k * 2 + s)
    rn = lambda *sh: torch.randn(*sh, generator=g)
    w_stride, bn_stride = k * k * C + 36, C + 20
    wbuf, isc, ish, osc, osh = (rn(GROUP_N * st) for st in (w_stride, bn_stride, bn_stride, bn_stride, bn_stride))
    isc, osc = isc.abs() * 0.5 + 0.5, osc.abs() * 0.5 + 0.5
    wbuf /= k
    return {"x": rn(B, H, W, C) * 1.7 + 0.3, "wbuf": wbuf, "isc": isc, "ish": ish * 0.2, "osc": osc, "osh": osh * 0.2,
            "w_stride": w_stride, "bn_stride": bn_stride, "pool0": (rn(B, C).double() * 0.5 * Q36).round().to(torch.int64)}


def group_ref(shape, k, s, pro, inp, dt, dev="cpu"):
    """each image against the reference with its group's taps and coefficients -> {"y", "pool"}"""
    B, H, W, C = shape
    d = _to(inp, dt, dev)
    r = route("fwd", B, H, W, C, k, s, pro=pro != "none", out=True)
    ys, ps = [], []
    for gi in range(GROUP_N):
        sl = slice(gi * GROUP_IMAGES, (gi + 1) * GROUP_IMAGES)
        wo, bo = gi * d["w_stride"], gi * d["bn_stride"]
        cf = lambda t: t[bo:bo + C]
        o = dw_fwd(d["x"][sl], d["wbuf"][wo:wo + k * k * C].view(k * k, C), k, s, cf(d["isc"]) if pro == "given" else None,
                   cf(d["ish"]) if pro == "given" else None, None, 1 if pro == "given" else 0, cf(d["osc"]), cf(d["osh"]), 1, None,
                   d["pool0"][sl].double() / Q36, r["pool_blocks"])
        ys.append(o["y"]); ps.append(o["pool"])
    cat = lambda xs: (torch.cat([v for v, _ in xs]), torch.cat([a for _, a in xs]))
    return {"y": cat(ys), "pool": cat(ps)}
