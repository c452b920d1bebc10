"""Helper (not a test): float64 restatement of three hand-written kernel groups - the frozen MBConv front half mmd_mbconv_expand_dw_fwd
(csrc/mbconv_fused.hip, grouped nets included), the fused expand backward mmd_mbconv_expand_bwd_fused (csrc/mbconv_bwd_fused.hip) and the stem:
mmd_stem_conv_fwd (mmd_pw_stem_gemm: pw_gemm_kernel<128, 32, nkl, fp32, PRO 2>), mmd_stem_conv_bwd_weight(_bn) (csrc/stem_wgrad.hip) and
mmd_stem_im2col - written from the contracts in include/mmdistill.h and the header comments of the .hip files, not from the kernels' loops;
a copy of the host dispatch of each (route); and the case tables that test_mb_ref_cpu.py and test_gpu_mb_float64.py share.

OUT OF SCOPE: the MMD_MBW_TM32 / MMD_MBW_GRID variants of the expand backward (test_mb_ref_cpu.py asserts that neither is set), the static
bf16-storage entry point of mbx (mmd_mbconv_expand_dw_fwd_w16: no public symbol), and MMD_STEM_DIRECT's direct stem kernel beyond what the
environment happens to select (route reports it, the cases still run).

Conventions are those of elt_ref.py / dw_ref.py / pw_ref.py / bd_ref.py.  Every reference computes in the dtype (and on the device) of its
tensor arguments: float64 is the oracle, float32 the "plain fp32" evaluation that calibrates K.  Every reference returns (value, A), A_i the
magnitude of what was summed into element i:
  * products: A_operand @ |w| (+ |residual|, + |initial value| where the kernel accumulates)
  * elementwise f(u): |f| + |f'| A_u (elt_ref.act_fwd); the folded BatchNorm A_z |scale| + |shift|
  * the depthwise conv: dw_ref.conv over the ZERO-padded activated tensor (value and magnitude 0 in the halo)
  * pool: as dw_ref - |pool0| + sum |y| * pool_scale + nblocks * 2^-36 (each block adds round(2^36 * partial mean))
  * BatchNorm backward operand: wg_ref.bn_operand; dgamma / dbeta: |start| + |sums|; upstream sums: bd_ref.xs_ref (the rounding of the kernel's
    own fp32 dx reaches them: sum A_dx |mul_b| (|xhat'|))
  * forward BatchNorm sums of the stem: pw_ref.pw_fwd's (sum: sum A_raw; sumsq: sum raw^2 + 2 |raw| A_raw)
Errors are judged per element, none left out: |got - ref64| <= K * 2^-24 * A + tiny, K = max(8, 4 * K32) per family, K32 the largest error of
the fp32 CPU evaluation of these references over the whole case table in the same unit (test_mb_ref_cpu.py measures it, asserts K32 <= K / 4
and that the K32 stored below is the one it measures).  mmd_stem_im2col is an exact gather (torch.equal).  No constant comes from a GPU run."""
import functools
import math
import os

import torch
import torch.nn.functional as F

from elt_ref import (swish, dswish, dswish_mag, act_fwd, ratio, rng, randn, rand, bn_inputs, bn_bwd_reduce, SENTINEL, f32, cdiv, U, TINY)      # noqa: F401
from dw_ref import conv, same_pad_lo, Q36, _to                                                                                            # noqa: F401
from pw_ref import pw_fwd
from wg_ref import bn_operand
from bd_ref import xs_ref

STATS_DEPTH = 128                    # MMD_STATS_DEPTH (common.h)

# K per family = max(8, 4 * K32).  K32 as test_mb_ref_cpu.py measures it (fp32 CPU evaluation of these references on every case):
K32 = {"mbx_y": 2.287, "mbx_pool": 3.825, "mbw_dx": 3.972, "mbw_dw": 2.436, "mbw_dsum": 1.759, "mbw_xs": 0.246, "stem_y": 5.299, "stem_stats": 0.759,
       "stem_dw": 3.270, "stem_dw_bn": 2.132, "stem_dsum": 1.780}
K_BY_FAMILY = {"mbx_y": 10.0, "mbx_pool": 16.0, "mbw_dx": 16.0, "mbw_dw": 10.0, "mbw_dsum": 8.0, "mbw_xs": 8.0, "stem_y": 22.0, "stem_stats": 8.0,
               "stem_dw": 14.0, "stem_dw_bn": 9.0, "stem_dsum": 8.0}


# ------------------------------------------------------------------------------------------------ references: mbx
def mbx_ref(x, w0, sc0, sh0, wd, sc1, sh1, k, s, pool0=None, nblocks=0):
    """mmd_mbconv_expand_dw_fwd: e = swish((x . w0^T) * sc0 + sh0) [B, H, W, Cmid]; the ACTIVATED tensor is zero-padded (TF-SAME);
    y = swish(dwconv_kxk/s(e, wd) * sc1 + sh1); pool += mean_hw y.  x [B, H, W, Cin], w0 [Cmid, Cin], wd [k*k, Cmid]; pool0: float64 [B, Cmid]
    = the Q36 integers / 2^36 (None: pool null)  -> {"y", "pool"} of (value, A)"""
    z, Az = x @ w0.t(), x.abs() @ w0.abs().t()
    e, Ae = act_fwd(z * sc0 + sh0, Az * sc0.abs() + sh0.abs(), 1)
    c, Ac = conv(e, Ae, wd, k, s)
    y, Ay = act_fwd(c * sc1 + sh1, Ac * sc1.abs() + sh1.abs(), 1)
    out = {"y": (y, Ay)}
    if pool0 is not None:
        ps = f32(1.0 / (y.shape[1] * y.shape[2]))
        out["pool"] = (pool0 + (y.sum((1, 2)) * ps).to(pool0.dtype), pool0.abs() + (y.abs().sum((1, 2)) * ps).to(pool0.dtype) + nblocks / Q36)
    return out


def mbx_group_ref(x, bufs, n, images, w_stride, bn_stride, Cin, Cmid, k, s, pool0=None, nblocks=0):
    """grouped nets: image b reads the parameter set of net b // images - w0 and wd w_stride floats, the four BatchNorm vectors bn_stride
    floats behind net 0's.  bufs: {"w0", "wd", "sc0", "sh0", "sc1", "sh1"} flat buffers"""
    ys, ps = [], []
    for gi in range(n):
        sl = slice(gi * images, (gi + 1) * images)
        wo, bo = gi * w_stride, gi * bn_stride
        cf = lambda key: bufs[key][bo:bo + Cmid]
        o = mbx_ref(x[sl], bufs["w0"][wo:wo + Cmid * Cin].view(Cmid, Cin), cf("sc0"), cf("sh0"), bufs["wd"][wo:wo + k * k * Cmid].view(k * k, Cmid),
                    cf("sc1"), cf("sh1"), k, s, None if pool0 is None else pool0[sl], nblocks)
        ys.append(o["y"])
        if pool0 is not None:
            ps.append(o["pool"])
    cat = lambda xs: (torch.cat([v for v, _ in xs]), torch.cat([a for _, a in xs]))
    out = {"y": cat(ys)}
    if ps:
        out["pool"] = cat(ps)
    return out


# ------------------------------------------------------------------------------------------------ references: mbw
def mbw_sums(g0, z0, scale, shift, mean, invstd):
    """the float64 numbers [2C] = [sum g', sum g' xhat], g' = g0 swish'(z0 scale + shift), that a reduce pass hands the launch (call with
    float64 tensors: elt_ref.bn_bwd_reduce, not mmd_bn_bwd_reduce)"""
    zero = torch.zeros(2 * z0.shape[1], dtype=torch.float64, device=z0.device)
    return bn_bwd_reduce(g0, z0, scale, shift, mean, invstd, 1, None, None, None, 1, zero)[2]


def mbw_ref(g0, z0, x, w, scale, shift, mean, invstd, sums, count, dw0, residual=None, dgamma0=None, dbeta0=None, xs=None):
    """mmd_mbconv_expand_bwd_fused: dz0 = scale (g' - m1 - xhat m2), [m1, m2] = sums / count; dx [M, Cin] = dz0 . w (+ residual);
    dw [Cmid, Cin] = dw0 + dz0^T . x; dgamma = dgamma0 + sums[C:], dbeta = dbeta0 + sums[:C]; xs (z, mean, invstd, mul_b or None, rpi, sums0):
    xs_sums [2 Cin] = sums0 + [sum g", sum g" xhat'] over the completed dx, g" = dx mul_b[row // rpi]
    -> {"dx", "dw", "dgamma", "dbeta", "xs_sums"} of (value, A)"""
    C = z0.shape[1]
    bn = {"z": z0, "scale": scale, "shift": shift, "mean": mean, "invstd": invstd, "sums": sums, "count": count, "act": 1, "mul_b": None, "rpi": 1}
    dz, Az = bn_operand(g0, bn)
    dx, A = dz @ w, Az @ w.abs()
    if residual is not None:
        dx, A = dx + residual, A + residual.abs()
    out = {"dx": (dx, A), "dw": (dw0 + dz.t() @ x, dw0.abs() + Az.t() @ x.abs())}
    if dgamma0 is not None:
        dt = z0.dtype
        out["dgamma"] = (dgamma0 + sums[C:].to(dt), dgamma0.abs() + sums[C:].abs().to(dt))
        out["dbeta"] = (dbeta0 + sums[:C].to(dt), dbeta0.abs() + sums[:C].abs().to(dt))
    if xs is not None:
        o = xs_ref(dx, A, xs)
        out["xs_sums"] = (torch.cat([o["xs_sum"][0], o["xs_sumsq"][0]]), torch.cat([o["xs_sum"][1], o["xs_sumsq"][1]]))
    return out


# ------------------------------------------------------------------------------------------------ references: stem
def kp_of(Cin):
    return cdiv(9 * Cin, 4) * 4


def stem_im2col_ref(x, Kp):
    """mmd_stem_im2col: x [B, Cin, H, W] NCHW -> col [B*OH*OW, Kp], col[(b, oh, ow)][ci*9 + i*3 + j] = x[b][ci][2 oh + i - pad_t][2 ow + j - pad_l]
    (zero outside the image: 3x3 / stride 2 TF-SAME), columns 9 Cin .. Kp - 1 zero.  An exact gather"""
    B, Cin, H, W = x.shape
    (OH, pt), (OW, pl) = same_pad_lo(H, 3, 2), same_pad_lo(W, 3, 2)
    xp = F.pad(x, (pl, 2 * OW + 1 - pl - W, pt, 2 * OH + 1 - pt - H))
    col = x.new_zeros(B, OH, OW, Kp)
    for ci in range(Cin):
        for i in range(3):
            for j in range(3):
                col[..., ci * 9 + i * 3 + j] = xp[:, ci, i:i + 2 * OH - 1:2, j:j + 2 * OW - 1:2]
    return col.view(B * OH * OW, Kp)


def stem_fwd_ref(x, w, out_scale=None, out_shift=None, out_act=0, stats0=None):
    """mmd_stem_conv_fwd: raw [B*OH*OW, Cout] = im2col(x) . w[Cout, Kp]^T; y = act(raw * out_scale + out_shift); stats = stats0 + [sum raw,
    sum raw^2] -> {"y", "stats"} of (value, A)"""
    o = pw_fwd(stem_im2col_ref(x, w.shape[1]), w, out_scale=out_scale, out_shift=out_shift, out_act=out_act, stats0=stats0)
    out = {"y": o["y"]}
    if stats0 is not None:
        out["stats"] = (torch.cat([o["sum"][0], o["sumsq"][0]]), torch.cat([o["sum"][1], o["sumsq"][1]]))
    return out


def stem_wgrad_ref(x, dz, Kp, dw0, bn=None):
    """mmd_stem_conv_bwd_weight: dw [Cout, Kp] = dw0 + dz^T . im2col(x) (the padding columns receive exactly 0).  bn (the dict of
    wg_ref.bn_operand with "dgamma0" / "dbeta0" or None): mmd_stem_conv_bwd_weight_bn - `dz` is the gradient g behind the BatchNorm (+act) and
    the operand is BnBwd(g, z); dgamma / dbeta += the sums  -> {"dw", "dgamma", "dbeta"} of (value, A)"""
    col = stem_im2col_ref(x, Kp)
    d, Ad = (dz, dz.abs()) if bn is None else bn_operand(dz, bn)
    out = {"dw": (dw0 + d.t() @ col, dw0.abs() + Ad.t() @ col.abs())}
    if bn is not None and bn.get("dgamma0") is not None:
        C, sums, dt = d.shape[1], bn["sums"], x.dtype
        out["dgamma"] = (bn["dgamma0"] + sums[C:].to(dt), bn["dgamma0"].abs() + sums[C:].abs().to(dt))
        out["dbeta"] = (bn["dbeta0"] + sums[:C].to(dt), bn["dbeta0"].abs() + sums[:C].abs().to(dt))
    return out


# ------------------------------------------------------------------------------------------------ the dispatch, copied
# Nothing checks these copies against the host code (except stem_wg_supported and the workspace size, which the GPU test compares with the
# library's): keep them in step by hand when the dispatch changes.
MBX_CINS = (16, 24, 32, 40, 48, 56)
MBX_KS = ((3, 1), (3, 2), (5, 1), (5, 2))
MBX_TILE = {(3, 1): (16, 16, 4), (5, 1): (16, 16, 4), (3, 2): (8, 8, 1), (5, 2): (8, 8, 1)}          # MbxCfg: TH, TW, R


def mbx_supported(Cin, Cmid, k, s):
    return (k, s) in MBX_TILE and Cmid > 0 and Cmid % 48 == 0 and Cin in MBX_CINS


def mbx_route(B, H, W, Cin, Cmid, k, s):
    """mbx_impl / mbx_launch (mbconv_fused.hip); None: refused"""
    if B <= 0 or H <= 0 or W <= 0 or not mbx_supported(Cin, Cmid, k, s):
        return None
    TH, TW, R = MBX_TILE[(k, s)]
    IH, IW = (TH - 1) * s + k, (TW - 1) * s + k
    PT = cdiv(IH * IW, 16)
    TPW = cdiv(PT, 4)
    (OH, pt), (OW, pl) = same_pad_lo(H, k, s), same_pad_lo(W, k, s)
    th, tw, cch = cdiv(OH, TH), cdiv(OW, TW), Cmid // 48
    grid = B * th * tw * cch
    return {"inst": (Cin // 4, k, s), "NK": Cin // 4, "vec": 4 if (Cin // 4) % 4 == 0 else 2, "PT": PT, "TPW": TPW, "partial_last": 4 * TPW > PT,
            "tiles": th * tw, "tiles_hw": (th, tw), "cchunks": cch, "grid": grid, "swizzled": (grid >> 3) << 3, "pad": (pt, pl), "out": (OH, OW),
            "ragged": (OH % TH != 0, OW % TW != 0), "tiles_per_block": 1}


MBW_PAIRS = {16: (96, 64, 768), 24: (144, 64, 512), 32: (192, 64, 256), 48: (288, 32, 256)}          # Cin -> Cmid, TM, persistent-grid cap


def mbw_supported(Cin, Cmid):
    """mmd_mbconv_expand_bwd_supported: "has a kernel AND pays" - (48, 288) only with MMD_MBW48"""
    if (Cin, Cmid) == (48, 288):
        return 1 if os.environ.get("MMD_MBW48") is not None else 0
    return 1 if Cin in MBW_PAIRS and MBW_PAIRS[Cin][0] == Cmid else 0


def mbw_route(M, Cin, Cmid):
    """mmd_mbconv_expand_bwd_fused / mbw_launch with neither MMD_MBW_TM32 nor MMD_MBW_GRID set; None: refused"""
    if M <= 0 or Cin not in MBW_PAIRS or MBW_PAIRS[Cin][0] != Cmid:
        return None
    C, TM, cap = MBW_PAIRS[Cin]
    ntiles = cdiv(M, TM)
    grid = min(ntiles, cap)
    return {"inst": (C, Cin, TM), "TM": TM, "cap": cap, "ntiles": ntiles, "grid": grid, "tiles_per_block": cdiv(ntiles, grid), "row_tail": M % TM,
            "col_mask": Cin % 16 != 0}


def stem_fwd_route(B, Cin, H, W, Kp, Cout, stats=False, ws_slots=0, scale_shift=(True, True)):
    """mmd_stem_conv_fwd / mmd_pw_stem_gemm; None: refused.  MMD_STEM_DIRECT in the environment: the direct VALU kernel"""
    if B <= 0 or Cin <= 0 or Cin > 64 or H <= 0 or W <= 0 or Kp < 9 * Cin or Cout not in (32, 40, 48, 56, 64) or scale_shift[0] != scale_shift[1]:
        return None
    M = B * cdiv(H, 2) * cdiv(W, 2)
    if os.environ.get("MMD_STEM_DIRECT") is not None or Kp & 3:
        nb = cdiv(M, 256)
        return {"kernel": "direct", "inst": Cout, "grid": nb, "nkl": None, "tiles_per_block": 1, "slotted": bool(stats and ws_slots > 1 and nb > STATS_DEPTH), "M": M}
    ntm, ntn = cdiv(M, 128), cdiv(Cout, 32)
    nkl = ((Kp - 1) % 32) // 8 + 1
    return {"kernel": "gemm", "inst": (128, 32, nkl, 2), "nkl": nkl, "ksteps": cdiv(Kp, 32), "ntm": ntm, "ntn": ntn, "grid": ntm * ntn, "tiles_per_block": 1,
            "row_tail": M % 128, "col_tail": Cout % 32, "slotted": bool(stats and ws_slots > 1 and ntm > STATS_DEPTH), "M": M}


SW_BLOCKS_MAX = 2048


def stem_wg_blocks():
    v = os.environ.get("MMD_STEM_WG_BLOCKS")
    b = 1024
    if v is not None:
        try:
            b = int(v.strip() or 0)
        except ValueError:
            b = 0
    return min(max(b, 1), SW_BLOCKS_MAX)


def stem_wg_supported(Cin, H, W, Kp, Cout):
    return int(1 <= Cin <= 8 and 9 * Cin <= Kp <= 80 and Kp % 4 == 0 and 4 <= Cout <= 48 and Cout % 4 == 0 and H >= 2 and W >= 2 and cdiv(W, 2) % 64 == 0)


def stem_wg_ws_floats(Cout):
    return SW_BLOCKS_MAX * 16 * cdiv(Cout, 16) * 80


def stem_wg_route(B, Cin, H, W, Kp, Cout, bn=False):
    """stem_wgrad_impl (stem_wgrad.hip); None: refused"""
    if B <= 0 or not stem_wg_supported(Cin, H, W, Kp, Cout):
        return None
    (OH, pt), (OW, pl) = same_pad_lo(H, 3, 2), same_pad_lo(W, 3, 2)
    ntiles = B * OH * (OW // 64)
    slots = min(ntiles, stem_wg_blocks())
    COT = cdiv(Cout, 16)
    return {"inst": (COT, bool(bn)), "COT": COT, "narrow": Cout < 16 * COT, "ntiles": ntiles, "slots": slots, "grid": slots, "tpr": OW // 64,
            "tiles_per_block": cdiv(ntiles, slots), "pad": (pt, pl), "kpad": Kp - 9 * Cin, "slotted": True,
            "fold": (fold_iters(slots)), "fold_grid": cdiv(Cout * Kp, 16)}


def fold_iters(slots):
    """(largest number of 64-strided iterations, of 16-strided tail iterations) any of the 16 lanes of an element of the fold kernel walks"""
    a = b = 0
    for part in range(16):
        k, n64, n16 = part, 0, 0
        while k + 48 < slots:
            k += 64
            n64 += 1
        while k < slots:
            k += 16
            n16 += 1
        a, b = max(a, n64), max(b, n16)
    return a, b


def route(family, *args, **kw):
    """family: "mbx" | "mbw" | "stem_fwd" | "stem_wg" -> the instantiation ("inst"), tiles per block, grid and the family's own fields (PT / TPW,
    nkl, COT, slots, slotted); None where the host refuses the call"""
    return {"mbx": mbx_route, "mbw": mbw_route, "stem_fwd": stem_fwd_route, "stem_wg": stem_wg_route}[family](*args, **kw)


# ------------------------------------------------------------------------------------------------ cases: mbx
def _x(name, B, Cin, Cmid, k, s, H, W, why, kind=""):
    return {"name": name, "B": B, "Cin": Cin, "Cmid": Cmid, "k": k, "s": s, "H": H, "W": W, "kind": kind, "why": why}


GROUP_N, GROUP_IMAGES = 3, 2
MBX_CASES = [
    _x("s1k3_exact", 3, 16, 48, 3, 1, 16, 16, "one exact 16x16 tile, one chunk: 3 blocks (< 8: the swizzle is the identity)"),
    _x("s1k3_ragged", 3, 24, 144, 3, 1, 19, 35, "2 x 3 ragged tiles, three chunks: 54 blocks = 48 swizzled + 6"),
    _x("s1k5_ragged", 3, 32, 48, 5, 1, 33, 17, "3 x 2 ragged tiles, 18 blocks"),
    _x("s1k5_h1", 3, 40, 144, 5, 1, 1, 5, "H = 1: the map is all halo but one row"),
    _x("s2k3_exact", 3, 48, 48, 3, 2, 16, 16, "16x16 -> one exact 8x8 tile, pad_lo 0"),
    _x("s2k3_odd", 3, 56, 144, 3, 2, 19, 35, "odd sizes at stride 2: pad_lo 1; 10 x 18 outputs = 2 x 3 ragged tiles"),
    _x("s2k5_odd", 3, 16, 144, 5, 2, 33, 17, "odd sizes, k 5: pad_lo 2; 17 x 9 outputs = 3 x 2 tiles"),
    _x("s2k5_even", 3, 24, 48, 5, 2, 20, 14, "even sizes, k 5: pad_lo 1; sub-tile width"),
    _x("one_block_w1", 1, 32, 48, 3, 1, 7, 1, "W = 1, B = 1: a single block"),
    _x("s2k3_h1", 3, 40, 48, 3, 2, 1, 9, "H = 1 at stride 2"),
    _x("shift0_3", 3, 48, 48, 3, 1, 10, 12, "|shift0| = 3: swish(BN0(0)) in the halo would be an O(1) error", "shift3"),
    _x("bn1_negative", 3, 56, 96, 5, 1, 9, 20, "u of BatchNorm-1 all negative; 12 blocks = 8 swizzled + 4", "negu"),
    _x("s2k3_even_multi", 3, 16, 96, 3, 2, 34, 20, "even sizes at stride 2, 3 x 2 tiles, pad_lo 0"),
    _x("s2k5_exact", 3, 48, 48, 5, 2, 16, 16, "16x16 -> one exact 8x8 tile, k 5"),
    _x("grid_multiple_of_8", 2, 24, 96, 3, 1, 17, 20, "2 x 2 tiles x 2 chunks x 2 images = 16 blocks: every block swizzled"),
] + [_x("lat_c%d_k%ds%d" % (Cin, k, s), 2, Cin, 48, k, s, 9 + (Cin // 8) % 3, 11 - (Cin // 8) % 2, "the instantiation lattice: NK %d, k %d, stride %d" % (Cin // 4, k, s))
     for Cin in MBX_CINS for k, s in MBX_KS]
MBX_GROUP_CASES = [
    _x("group_s1", GROUP_N * GROUP_IMAGES, 24, 96, 3, 1, 19, 20, "3 nets x 2 images, stride 1, float2 fragments", "group"),
    _x("group_s2", GROUP_N * GROUP_IMAGES, 32, 48, 5, 2, 17, 12, "3 nets x 2 images, stride 2, float4 fragments", "group"),
]
MBX = {c["name"]: c for c in MBX_CASES + MBX_GROUP_CASES}
assert len(MBX) == len(MBX_CASES) + len(MBX_GROUP_CASES)


def mbx_route_of(c):
    return mbx_route(c["B"], c["H"], c["W"], c["Cin"], c["Cmid"], c["k"], c["s"])


@functools.lru_cache(maxsize=None)
def _mbx_inputs(name):
    c = MBX[name]
    B, Cin, C, k, s, H, W = (c[key] for key in ("B", "Cin", "Cmid", "k", "s", "H", "W"))
    g = rng(61, B, H, W, Cin, C + 7 * k + s)
    OH, OW = same_pad_lo(H, k, s)[0], same_pad_lo(W, k, s)[0]
    d = {"x": randn(g, B, H, W, Cin), "pool0": (randn(g, B, C).double() * 0.5 * Q36).round().to(torch.int64)}
    if c["kind"] == "group":
        ws = cdiv(max(C * Cin, k * k * C), 4) * 4 + 36          # one stride serves both weight buffers; a multiple of 4 (float4 loads)
        bs = C + 20
        d["w_stride"], d["bn_stride"] = ws, bs
        d["w0"], d["wd"] = randn(g, GROUP_N * ws) / math.sqrt(Cin), randn(g, GROUP_N * ws) / k
        d["sc0"], d["sc1"] = rand(g, GROUP_N * bs) + 0.5, rand(g, GROUP_N * bs) + 0.5
        d["sh0"], d["sh1"] = randn(g, GROUP_N * bs) * 0.2, randn(g, GROUP_N * bs) * 0.2
        return d
    d.update(w0=randn(g, C, Cin) / math.sqrt(Cin), wd=randn(g, k * k, C) / k, sc0=rand(g, C) + 0.5, sh0=randn(g, C) * 0.2, sc1=rand(g, C) + 0.5,
             sh1=randn(g, C) * 0.2)
    if c["kind"] == "shift3":
        d["sh0"] = torch.where(rand(g, C) < 0.5, -1.0, 1.0) * (3.0 + rand(g, C) * 0.25)
    if c["kind"] == "negu":
        d["sc1"], d["sh1"] = rand(g, C) * 0.05 + 0.05, -(8.0 + rand(g, C))
    return d


def mbx_inputs(c):
    """fp32 (int64 for the pool) CPU tensors of one case; cached - do not modify"""
    return _mbx_inputs(c["name"])


def mbx_case_ref(c, inp, dt, dev="cpu", pool=True):
    d = _to(inp, dt, dev)
    r = mbx_route_of(c)
    p0 = d["pool0"].double() / Q36 if pool else None
    if c["kind"] == "group":
        return mbx_group_ref(d["x"], d, GROUP_N, GROUP_IMAGES, d["w_stride"], d["bn_stride"], c["Cin"], c["Cmid"], c["k"], c["s"], p0, r["tiles"])
    return mbx_ref(d["x"], d["w0"], d["sc0"], d["sh0"], d["wd"], d["sc1"], d["sh1"], c["k"], c["s"], p0, r["tiles"])


MBX_REFUSED = [(88, 528, 3, 1), (16, 100, 3, 1), (20, 48, 3, 1), (16, 48, 4, 1), (16, 48, 3, 3), (16, 0, 3, 1), (64, 48, 5, 2)]          # (Cin, Cmid, k, s)


# ------------------------------------------------------------------------------------------------ cases: mbw
XS_RPI = 35                          # rows per image of xs_mul_b: no multiple of a 32- or 64-row tile, several images meet inside one tile


def _w(Cin, M, res, xs, dsum, why):
    return {"name": "c%d_m%d_%s_%s_%s" % (Cin, M, res, xs, "dsum" if dsum else "nodsum"), "Cin": Cin, "Cmid": MBW_PAIRS[Cin][0], "M": M, "res": res,
            "xs": xs, "dsum": dsum, "why": why}


def _mbw_cases():
    cs = []
    for Cin, (C, TM, cap) in MBW_PAIRS.items():
        big = cap * TM + TM + 7
        cs += [_w(Cin, 1, "none", "off", True, "M = 1"),
               _w(Cin, TM - 1, "alias", "on", True, "one ragged tile, residual in place"),
               _w(Cin, TM, "sep", "mulb", False, "one exact tile, a separate residual, dgamma / dbeta null"),
               _w(Cin, TM + 1, "none", "mulb", True, "a second tile of one row: 63 (31) zero rows multiply into dW"),
               _w(Cin, 1000, "alias", "mulb", True, "a ragged few tiles"),
               _w(Cin, 1000, "sep", "on", False, "a ragged few tiles, separate residual"),
               _w(Cin, 1000, "none", "off", False, "no residual, no upstream sums, no dgamma"),
               _w(Cin, big, "alias", "mulb", True, "just past cap * TM: blocks 0 and 1 walk a second tile, the last one ragged")]
    return cs


MBW_CASES = _mbw_cases()
MBW = {c["name"]: c for c in MBW_CASES}
assert len(MBW) == len(MBW_CASES)


def mbw_inputs(c):
    """fp32 CPU tensors of one case (not cached: the largest are tens of MB), count != M"""
    M, Cin, C = c["M"], c["Cin"], c["Cmid"]
    g = rng(62, M, Cin, C)
    z0, _, _, _, coef = bn_inputs(g, M, C)
    d = {"g0": randn(g, M, C), "z0": z0, "x": randn(g, M, Cin), "w": randn(g, C, Cin) / math.sqrt(Cin), "scale": coef["scale"], "shift": coef["shift"],
         "mean": coef["mean"], "invstd": coef["invstd"], "count": 2 * M + 1, "dw0": randn(g, C, Cin), "dgamma0": randn(g, C), "dbeta0": randn(g, C),
         "res": randn(g, M, Cin), "xs_z": randn(g, M, Cin) * 0.8 + 0.1, "xs_mean": randn(g, Cin) * 0.2, "xs_invstd": rand(g, Cin) + 0.5,
         "xs_mul_b": rand(g, cdiv(M, XS_RPI)) + 0.5, "xs0": randn(g, 2 * Cin).double() * 3}
    if d["xs_mul_b"].numel() > 1:
        d["xs_mul_b"][1] = 0.0                                # a dropped sample
    return d


def mbw_case_sums(d64):
    return mbw_sums(d64["g0"], d64["z0"], d64["scale"], d64["shift"], d64["mean"], d64["invstd"])


def mbw_case_ref(c, d, sums):
    """reference of one case from the input dict d (any dtype / device) and the float64 sums"""
    xs = None
    if c["xs"] != "off":
        xs = {"z": d["xs_z"], "mean": d["xs_mean"], "invstd": d["xs_invstd"], "mul_b": d["xs_mul_b"] if c["xs"] == "mulb" else None, "rpi": XS_RPI,
              "sums0": d["xs0"]}
    return mbw_ref(d["g0"], d["z0"], d["x"], d["w"], d["scale"], d["shift"], d["mean"], d["invstd"], sums, d["count"], d["dw0"],
                   d["res"] if c["res"] != "none" else None, d["dgamma0"] if c["dsum"] else None, d["dbeta0"] if c["dsum"] else None, xs)


# ------------------------------------------------------------------------------------------------ cases: stem forward
def _sf(B, Cin, H, W, Cout, why, slots=0):
    return {"name": "b%d_c%d_%dx%d_n%d" % (B, Cin, H, W, Cout), "B": B, "Cin": Cin, "H": H, "W": W, "Kp": kp_of(Cin), "Cout": Cout, "slots": slots, "why": why}


STEM_FWD_MODES = ("stats", "fold0", "fold1")          # raw output + sums on a non-zero start | folded scale / shift, act 0 | ... + swish
STEM_FWD_CASES = [
    _sf(3, 1, 5, 7, 32, "Kp 12: nkl 2; odd H != W, 36 rows"),
    _sf(2, 2, 16, 16, 40, "Kp 20: nkl 3; M = 128 exactly; column tail 8"),
    _sf(1, 3, 2, 2, 48, "Kp 28: nkl 4; a 2 x 2 image, M = 1"),
    _sf(2, 8, 1, 1, 56, "Kp 72: three K steps, nkl 1; a 1 x 1 image, M = 2"),
    _sf(2, 9, 33, 18, 64, "Kp 84: nkl 3; two full column tiles; M = 306: three row tiles, tail 50"),
    _sf(4, 3, 16, 32, 32, "M = 512: four exact row tiles"),
    _sf(2, 8, 9, 6, 64, "Cin 8 with two column tiles"),
    _sf(2, 9, 4, 10, 40, "Cin 9 with the column tail"),
    _sf(3, 1, 7, 4, 56, "Cin 1, Cout 56"),
    _sf(1, 2, 3, 3, 48, "Cin 2, Cout 48, M = 4"),
    _sf(1, 3, 258, 258, 32, "16641 rows = 131 row tiles > MMD_STATS_DEPTH: slotted sums, the workspace must be zero afterwards", slots=64),
]
STEM_FWD = {c["name"]: c for c in STEM_FWD_CASES}
assert len(STEM_FWD) == len(STEM_FWD_CASES)


def stem_fwd_route_of(c, mode):
    return stem_fwd_route(c["B"], c["Cin"], c["H"], c["W"], c["Kp"], c["Cout"], stats=mode == "stats", ws_slots=c["slots"])


def stem_fwd_inputs(c):
    B, Cin, H, W, Kp, Cout = (c[k] for k in ("B", "Cin", "H", "W", "Kp", "Cout"))
    g = rng(63, B, Cin, H, W, Cout)
    w = randn(g, Cout, Kp) / math.sqrt(9 * Cin)          # (the padding columns are NOT zeroed: the gathered operand is zero there)
    return {"x": randn(g, B, Cin, H, W), "w": w, "osc": rand(g, Cout) + 0.5, "osh": randn(g, Cout) * 0.2, "stats0": randn(g, 2 * Cout).double() * 3}


def stem_fwd_case_ref(c, mode, inp, dt, dev="cpu"):
    d = _to(inp, dt, dev)
    if mode == "stats":
        return stem_fwd_ref(d["x"], d["w"], stats0=d["stats0"])
    return stem_fwd_ref(d["x"], d["w"], d["osc"], d["osh"], 1 if mode == "fold1" else 0)


STEM_FWD_REFUSED = [dict(Cout=36), dict(no_shift=True), dict(Kp=24)]          # on B 2, Cin 3, 8 x 8, Kp 28, Cout 32


# ------------------------------------------------------------------------------------------------ cases: stem weight gradient
def _sw(B, Cin, H, W, Cout, modes, why, Kp=None):
    Kp = Kp or kp_of(Cin)
    return {"name": "b%d_c%d_%dx%d_k%d_n%d" % (B, Cin, H, W, Kp, Cout), "B": B, "Cin": Cin, "H": H, "W": W, "Kp": Kp, "Cout": Cout, "modes": modes, "why": why}


# modes: "plain" (mmd_stem_conv_bwd_weight) | "bn0" / "bn1" (_bn with act 0 / 1, dgamma / dbeta on a non-zero start) | "bn1n" (act 1, both null)
_BN_ROT = ("bn1", "bn0", "bn1n")
STEM_WG_SLOTS = (1, 15, 16, 17, 48, 49, 64, 65, 113)
STEM_WG_CASES = [
    _sw(2, 1, 2, 127, 4, ("plain", "bn1"), "COT 1, Cout 4 < 16; W 127: pad_l 1, one tile per row; H = 2"),
    _sw(2, 3, 3, 128, 20, ("plain", "bn0"), "COT 2, Cout 20 < 32; W 128: pad_l 0; odd H"),
    _sw(2, 8, 5, 255, 32, ("plain", "bn1n"), "COT 2, Cout 32 = 32; W 255: pad_l 1, two tiles per row"),
    _sw(2, 1, 4, 256, 36, ("plain", "bn1"), "COT 3, Cout 36 < 48; Kp 80 with Cin 1: 71 padding columns; W 256: two tiles per row", Kp=80),
    _sw(2, 3, 7, 256, 48, ("plain", "bn0"), "COT 3, Cout 48 = 48"),
    _sw(1, 8, 6, 127, 48, ("plain", "bn1"), "Cin 8 (Kp 72), Cout 48"),
    _sw(2, 8, 3, 128, 4, ("plain", "bn1n"), "Cin 8, Cout 4"),
    _sw(1, 3, 2, 255, 36, ("plain", "bn0"), "Cin 3, Cout 36, H = 2, W 255"),
] + [_sw(1, 1, 2 * n, 128, (4, 20, 32, 36, 48)[i % 5], ("plain", _BN_ROT[i % 3]), "slots = %d: the fold loop's 64 / 16-strided boundaries" % n)
     for i, n in enumerate(STEM_WG_SLOTS)] + [
    _sw(2, 1, 1100, 128, 20, ("plain", "bn1"), "1100 tiles on 1024 blocks: blocks 0 .. 75 walk two tiles"),
]
STEM_WG = {c["name"]: c for c in STEM_WG_CASES}
assert len(STEM_WG) == len(STEM_WG_CASES)

# the truth table of mmd_stem_conv_bwd_weight_supported at its edges: (Cin, H, W, Kp, Cout)
STEM_WG_EDGES = [(3, 8, 126, 28, 32), (3, 8, 127, 28, 32), (3, 8, 128, 28, 32), (3, 8, 129, 28, 32), (3, 8, 130, 28, 32),          # OW 63 / 64 / 64 / 65 / 65
                 (0, 8, 128, 28, 32), (8, 8, 128, 72, 32), (9, 8, 128, 84, 32), (8, 8, 128, 80, 32), (3, 8, 128, 84, 32), (3, 8, 128, 24, 32),
                 (3, 8, 128, 30, 32), (3, 8, 128, 28, 0), (3, 8, 128, 28, 48), (3, 8, 128, 28, 52), (3, 8, 128, 28, 6), (3, 8, 128, 28, 4),
                 (3, 1, 128, 28, 32), (3, 2, 128, 28, 32), (3, 8, 256, 28, 32), (1, 2, 127, 80, 4)]


def stem_wg_route_of(c, mode="plain"):
    return stem_wg_route(c["B"], c["Cin"], c["H"], c["W"], c["Kp"], c["Cout"], bn=mode != "plain")


def stem_wg_inputs(c):
    B, Cin, H, W, Kp, Cout = (c[k] for k in ("B", "Cin", "H", "W", "Kp", "Cout"))
    g = rng(64, B, Cin, H, W, Cout)
    M = B * cdiv(H, 2) * cdiv(W, 2)
    z, _, _, _, coef = bn_inputs(g, M, Cout)
    return {"x": randn(g, B, Cin, H, W), "dz": randn(g, M, Cout), "z": z, "scale": coef["scale"], "shift": coef["shift"], "mean": coef["mean"],
            "invstd": coef["invstd"], "count": 2 * M + 1, "dw0": randn(g, Cout, Kp), "dgamma0": randn(g, Cout), "dbeta0": randn(g, Cout)}


def stem_wg_case_sums(d64, act):
    zero = torch.zeros(2 * d64["z"].shape[1], dtype=torch.float64, device=d64["z"].device)
    return bn_bwd_reduce(d64["dz"], d64["z"], d64["scale"], d64["shift"], d64["mean"], d64["invstd"], act, None, None, None, 1, zero)[2]


def stem_wg_act(mode):
    return 0 if mode == "bn0" else 1


def stem_wg_case_ref(c, mode, d, sums=None):
    if mode == "plain":
        return stem_wgrad_ref(d["x"], d["dz"], c["Kp"], d["dw0"])
    ds = mode != "bn1n"
    bn = {"z": d["z"], "scale": d["scale"], "shift": d["shift"], "mean": d["mean"], "invstd": d["invstd"], "sums": sums, "count": d["count"],
          "act": stem_wg_act(mode), "mul_b": None, "rpi": 1, "dgamma0": d["dgamma0"] if ds else None, "dbeta0": d["dbeta0"] if ds else None}
    return stem_wgrad_ref(d["x"], d["dz"], c["Kp"], d["dw0"], bn)


IM2COL_CASES = [(2, 1, 5, 7, 12), (2, 3, 8, 6, 28), (1, 8, 1, 1, 72), (2, 1, 4, 4, 80), (1, 9, 3, 2, 84), (2, 2, 2, 2, 20)]          # (B, Cin, H, W, Kp)

FAMILY = {("mbx", "y"): "mbx_y", ("mbx", "pool"): "mbx_pool", ("mbw", "dx"): "mbw_dx", ("mbw", "dw"): "mbw_dw", ("mbw", "dgamma"): "mbw_dsum",
          ("mbw", "dbeta"): "mbw_dsum", ("mbw", "xs_sums"): "mbw_xs", ("stem_fwd", "y"): "stem_y", ("stem_fwd", "stats"): "stem_stats",
          ("stem_wg", "dw"): "stem_dw", ("stem_wg_bn", "dw"): "stem_dw_bn", ("stem_wg_bn", "dgamma"): "stem_dsum", ("stem_wg_bn", "dbeta"): "stem_dsum"}
