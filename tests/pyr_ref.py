"""Helper (not a test): float64 restatement of the detection heads' feature-pyramid ("pyr") launches - mmd_dwconv3_pyr,
mmd_dwconv3_pyr_bwd_weight (csrc/dwconv.hip), mmd_pwconv_fwd_pyr, mmd_pwconv_fwd_pyr_bf16 (pw_fwd_pyr_impl in csrc/pw_gemm.hip, the row-slab
kernel of csrc/pw_rows.hip), mmd_bn_bwd_reduce_pyr, mmd_bn_bwd_apply_pyr, mmd_pyr_add_bnsums, mmd_slice_rows_pyr (csrc/elt.hip) and the
grouped-nets mode (mmd_set_group) of the two forward entry points - written from the contracts in include/mmdistill.h and the header
comments of those files, not from the kernels' loops; a copy of the host dispatch (route_dw, route_pw = pw_ref.route under a pyramid); and
the one case table (PYR_CASES) that test_pyr_ref_cpu.py and test_gpu_pyr_float64.py share.

A pyramid is ONE row buffer [row0[n], C]: level l (B images of H_l x W_l) occupies rows [row0[l], row0[l] + B*H_l*W_l), every level starts
at a multiple of 128 rows, per-level BatchNorm data lie lev_stride channels apart (the double sums 2 * lev_stride doubles).  Every
reference is "per level: slice the level's valid rows, apply the existing reference (dw_ref.conv / conv_bwd_data / conv_bwd_weight,
elt_ref.bn_bwd_reduce / bn_bwd_apply / bn_finalize / act_fwd, pw_ref.pw_fwd / live_coef / remap_index) with that level's own coefficients
and that level's own count B*H_l*W_l" and returns per level (value, A) under the conventions of those helpers: products are
A_operand @ |w|, accumulating outputs add |initial value|, the magnitude of an upstream value is carried through every factor
(A_y * elt_ref.dswish_mag, ... * |xhat|).  mmd_pyr_add_bnsums: out = a + b (+ c), A = |a| + |b| (+ |c|); sums_l += [sum out, sum out*xhat]
over the level's valid rows, A = |start| + sum A_out (|xhat|) - the rounding of the kernel's own fp32 out reaches the sums, as in
bd_ref.xs_ref.  mmd_slice_rows_pyr is an exact gather.

PADDING ROWS (up to 127 per level), read off the code of every entry point; the GPU test fills them with sentinel-sized finite garbage in
every input and with the sentinel in every output, and asserts bitwise:
  * mmd_dwconv3_pyr (tile and row-streaming kernel), mmd_bn_bwd_reduce_pyr (g_out), mmd_bn_bwd_apply_pyr (dz), mmd_pyr_add_bnsums (out):
    blocks stop at the level's valid rows - padding rows of the output are NOT written (the sentinel survives)
  * mmd_pwconv_fwd_pyr(_bf16): every variant - skinny 32x64, 128x32, 64x64, 128x64 (`row < Mv` in pw_gemm_body / pw_gemm_skinny) and the
    row-slab kernel (`rok[i]` / `rows_full` of pw_rows.hip) - masks its stores and its statistics by the level's valid count: NOT written.
    The variants agree; engine.py allocates these buffers zeroed where a consumer reduces over all rows
  * mmd_slice_rows_pyr: writes ZEROS
  * no reduction (stats, bn_sums, dw_grad, dw, sums, dgamma / dbeta, sums[l]) may see a padding row: each must equal the reference of the
    valid rows alone; the arrays between the level slots (lev_stride > C) must keep their contents.

Errors are judged per element: |got - ref64| <= K * unit * A + tiny, unit 2^-24 (2^-9 for the _bf16 families, against float64 of the
UNROUNDED operands), K = max(8, ceil(4 * K32)) per output family, K32 the largest error in that unit of the fp32 CPU model over every
(case, mode) of PYR_CASES (test_pyr_ref_cpu.py measures it and asserts that the constants below are the ones it gives).  The model is the
reference run in float32; for the GEMM the dot product is the strictly sequential chain pw_ref.seq_dot, the bf16 model rounds both operands
to bf16 with exact products (as pw_ref), the BatchNorm-backward apply is formed as a1*g + a2*(z - mean) + a3 (wg_ref.bn_operand's kernel
order).  No constant comes from a GPU run of the kernels.

The dispatch copies assume that none of the variables the host code of these paths reads is set (ENV_PREFIXES; asserted by the CPU test):
MMD_DW_ROWS_PYR, MMD_DW_ROWS, MMD_DW_NOSWZ, MMD_DW_LANES, MMD_DW_ROWS_RH, MMD_ROWS_*, MMD_NO_ROWS, MMD_STREAM, MMD_SKINNY_*, MMD_SQ_*,
MMD_BN32_GAIN, MMD_NO_LEAN, MMD_MFMA_F32, MMD_SK_*, MMD_NO_BQ_LDS, MMD_BQ_LDS_CAP_KB, and - read on the way although the long-K and slab
kernels refuse a pyramid - MMD_NO_LONGK, MMD_NO_SLAB, MMD_SLAB_BLOCKS.  (MMD_DEV is read in pw_rows_try only to gate MMD_ROWS_ABL, which the
MMD_ROWS_ prefix covers; on its own it changes nothing.)  The variants reachable only through such a variable
(the streaming GEMM, the tile kernel on wide pyramids, ...) are out of scope, as are the bf16 storage forms."""
import ctypes
import functools
import math

import torch

from elt_ref import (dswish, dswish_mag, act_fwd, ratio, rng, SENTINEL, bn_finalize, bn_bwd_g, bn_bwd_reduce, bn_bwd_apply, cdiv, U, TINY)   # noqa: F401
from dw_ref import conv, conv_bwd_data, conv_bwd_weight, producer
import pw_ref
from pw_ref import pw_fwd, live_coef, remap_index, seq_dot, UB

ENV_PREFIXES = ("MMD_DW_", "MMD_ROWS_", "MMD_NO_ROWS", "MMD_STREAM", "MMD_SKINNY_", "MMD_SQ_", "MMD_BN32_GAIN", "MMD_NO_LEAN", "MMD_MFMA_F32",
                "MMD_SK_", "MMD_NO_BQ_LDS", "MMD_BQ_LDS_CAP_KB", "MMD_NO_LONGK", "MMD_NO_SLAB", "MMD_SLAB_")
MAX_LEV = 5                          # MMD_MAX_LEV
WIDTHS = (64, 112, 160, 224)         # the widths the model builds

# K per family = max(8, ceil(4 * K32)).  K32 as test_pyr_ref_cpu.py measures it (the fp32 CPU models of the docstring on every case and mode):
K32 = {"dw": 4.661, "dw_live": 2.630, "dwgrad": 1.652, "bnsums": 2.091, "pw_y": 6.499, "pw_sum": 2.112, "pw_sumsq": 2.484, "pw_y_bf16": 2.108,
       "pw_sum_bf16": 1.790, "pw_sumsq_bf16": 1.304, "red_g": 7.858, "red_sums": 2.915, "app_dz": 7.326, "app_dsum": 1.753, "add_out": 1.845,
       "add_sums": 1.538}
K_BY_FAMILY = {f: float(max(8, math.ceil(4 * k))) for f, k in K32.items()}
UNIT = {f: (UB if f.endswith("_bf16") else U) for f in K32}


# ------------------------------------------------------------------------------------------------ the pyramid
class Pyr:
    """mmd_make_pyr restated: rows[l] = B*H_l*W_l, row0[l+1] = row0[l] + rows[l] rounded up to 128; flat = the host descriptor"""

    def __init__(self, B, sizes):
        self.B, self.sizes, self.n = B, [tuple(s) for s in sizes], len(sizes)
        self.rows = [B * h * w for h, w in self.sizes]
        self.row0 = [0]
        for r in self.rows:
            self.row0.append(self.row0[-1] + (r + 127) // 128 * 128)
        self.Mt = self.row0[-1]
        self.flat = [self.n, B] + [v for hw in self.sizes for v in hw]

    def desc(self):
        return (ctypes.c_int * len(self.flat))(*self.flat)

    def valid(self):
        """bool [Mt]: the rows that belong to a level"""
        m = torch.zeros(self.Mt, dtype=torch.bool)
        for l in range(self.n):
            m[self.row0[l]:self.row0[l] + self.rows[l]] = True
        return m


def pyramid(B, sizes):
    """-> (ctypes descriptor {n, B, H0, W0, ...}, row0 [n + 1], rows [n])"""
    p = Pyr(B, sizes)
    return p.desc(), p.row0, p.rows


def lvl(buf, P, l):
    return buf[P.row0[l]:P.row0[l] + P.rows[l]]


def co(arr, l, ls, C):
    """level l's [C] slice of a per-level array handed to the kernel (lev_stride channels apart)"""
    return None if arr is None else arr[l * ls:l * ls + C]


def co2(arr, l, ls, n2):
    """level l's slice of per-level double sums (2 * lev_stride doubles apart)"""
    return None if arr is None else arr[2 * l * ls:2 * l * ls + n2]


# ------------------------------------------------------------------------------------------------ references
def _wgrad_level(xl, f, Af):
    z = torch.zeros(9, xl.shape[-1], dtype=xl.dtype, device=xl.device)
    return conv_bwd_weight(f, xl, 3, 1, z)[0], conv_bwd_weight(Af, xl.abs(), 3, 1, z)[0]


def dw_pyr(P, C, x, w, flip, ls=0, in_scale=None, in_shift=None, in_act=0, live=None, wg=None, dw0=None, bn=None):
    """mmd_dwconv3_pyr.  flip 0: y_l = dwconv3x3_same(act(x_l * scale_l + shift_l), w), live = (float64 sums, gamma, beta): the coefficients
    from level l's sums with count B*H_l*W_l; flip 1: the input gradient of that conv.  wg = (wg_x, wg_scale, wg_shift, wg_act) with dw0:
    dw_grad = dw0 + sum_l conv_bwd_weight(act(wg_x_l * wg_scale_l + wg_shift_l), x_l); bn = (mean, invstd, sums0) per level:
    bn_sums_l = sums0_l + [sum g, sum g*xhat], g = y_l * swish'(wg_x_l*wg_scale_l + wg_shift_l), xhat = (wg_x_l - mean_l) * invstd_l.
    -> {"y": [(v, A)], "dw_grad": (v, A), "bn_sums": [(v, A)]}"""
    out = {"y": []}
    dv = dA = None
    for l, (H, W) in enumerate(P.sizes):
        xl = lvl(x, P, l).view(P.B, H, W, C)
        if flip:
            y, A = conv_bwd_data(xl, xl.abs(), w, H, W, 3, 1)
        else:
            sc = sh = ash = None
            if live is not None:
                sc, sh, ash = live_coef(co2(live[0], l, ls, 2 * C), P.rows[l], co(live[1], l, ls, C), co(live[2], l, ls, C))
            elif in_scale is not None:
                sc, sh = co(in_scale, l, ls, C), co(in_shift, l, ls, C)
            a, Aa = producer(xl, sc, sh, ash, in_act)
            y, A = conv(a, Aa, w, 3, 1)
        out["y"].append((y.reshape(-1, C), A.reshape(-1, C)))
        if dw0 is None:
            continue
        wx = lvl(wg[0], P, l).view(P.B, H, W, C)
        wsc, wsh = co(wg[1], l, ls, C), co(wg[2], l, ls, C)
        f, Af = producer(wx, wsc, wsh, None, wg[3])
        v, Av = _wgrad_level(xl, f, Af)
        dv, dA = (v, Av) if dv is None else (dv + v, dA + Av)
        if bn is not None:
            u, Au = wx * wsc + wsh, (wx * wsc).abs() + wsh.abs()
            g, Ag = y * dswish(u), A * dswish_mag(u, Au)
            xh = (wx - co(bn[0], l, ls, C)) * co(bn[1], l, ls, C)
            s0, d = co2(bn[2], l, ls, 2 * C), (0, 1, 2)
            out.setdefault("bn_sums", []).append((s0 + torch.cat([g.sum(d), (g * xh).sum(d)]).to(s0.dtype),
                                                  s0.abs() + torch.cat([Ag.sum(d), (Ag * xh.abs()).sum(d)]).to(s0.dtype)))
    if dw0 is not None:
        out["dw_grad"] = (dw0 + dv, dw0.abs() + dA)
    return out


def dw_wgrad_pyr(P, C, x, dy, dw0, ls=0, in_scale=None, in_shift=None, in_act=0):
    """mmd_dwconv3_pyr_bwd_weight: dw = dw0 + sum_l conv_bwd_weight(act(x_l * scale_l + shift_l), dy_l) -> (v, A)"""
    return dw_pyr(P, C, dy, torch.zeros(9, C, dtype=x.dtype, device=x.device), 1, ls, wg=(x, in_scale, in_shift, in_act), dw0=dw0)["dw_grad"]


def pw_pyr(P, x, w, bias=None, out_act=0, stats0=None, ls=0, dot=None, bf16=False):
    """mmd_pwconv_fwd_pyr(_bf16): per level pw_ref.pw_fwd; level l's statistics accumulate onto stats0[2*l*ls : 2*l*ls + 2N]
    -> {"y": [(v, A)], "sum": [...], "sumsq": [...]}"""
    N = w.shape[0]
    out = {"y": []}
    for l in range(P.n):
        o = pw_fwd(lvl(x, P, l), w, bias=bias, out_act=out_act, stats0=co2(stats0, l, ls, 2 * N), dot=dot, bf16=bf16)
        for k, v in o.items():
            out.setdefault(k, []).append(v)
    return out


def head_index(P, l, N, y_batch_stride, y_off, device="cpu"):
    """flat positions of level l's [rows_l, N] block in the strided head output: image * y_batch_stride + y_off_lev[l] + (row in image) * N + n"""
    H, W = P.sizes[l]
    return remap_index(P.rows[l], N, H * W, y_batch_stride, y_off[l], device)


def bn_reduce_pyr(P, C, g_in, z, scale, shift, mean, invstd, act, ls, sums0):
    """mmd_bn_bwd_reduce_pyr -> {"g": [(v, A)], "sums": [(v, A)]}"""
    out = {"g": [], "sums": []}
    for l in range(P.n):
        g, Ag, s, As = bn_bwd_reduce(lvl(g_in, P, l), lvl(z, P, l), co(scale, l, ls, C), co(shift, l, ls, C), co(mean, l, ls, C),
                                     co(invstd, l, ls, C), act, None, None, None, 1, co2(sums0, l, ls, 2 * C))
        out["g"].append((g, Ag))
        out["sums"].append((s, As))
    return out


def bn_apply_pyr(P, C, g, z, mean, invstd, gamma, sums, ls, dgamma0=None, dbeta0=None, scale=None, shift=None, act=0, kernel_order=False):
    """mmd_bn_bwd_apply_pyr: per level elt_ref.bn_bwd_apply with count = B*H_l*W_l; act 1: g recomputed as g * swish'(z*scale_l + shift_l).
    kernel_order (the fp32 model): dz = a1*g + a2*(z - mean) + a3.  -> {"dz": [(v, A)], "dgamma": [...], "dbeta": [...]}"""
    out = {"dz": []}
    for l in range(P.n):
        gl, zl = lvl(g, P, l), lvl(z, P, l)
        mu, istd, ga, sm = co(mean, l, ls, C), co(invstd, l, ls, C), co(gamma, l, ls, C), co2(sums, l, ls, 2 * C)
        if act:
            gl, Ag = bn_bwd_g(gl, zl, co(scale, l, ls, C), co(shift, l, ls, C), 1, None, None, None, 1)
        else:
            Ag = gl.abs()
        o = bn_bwd_apply(gl, Ag, zl, mu, istd, ga, sm, P.rows[l], co(dgamma0, l, ls, C), co(dbeta0, l, ls, C))
        if kernel_order:
            inv = 1.0 / float(P.rows[l])
            m1, m2 = (sm[:C] * inv).to(zl.dtype), (sm[C:] * inv).to(zl.dtype)
            k = ga * istd
            o["dz"] = (k * gl + (-k * istd * m2) * (zl - mu) + (-k * m1), o["dz"][1])
        for key, v in o.items():
            out.setdefault(key, []).append(v)
    return out


def add_bnsums(P, C, a, b, c, z, mean, invstd, sums0):
    """mmd_pyr_add_bnsums.  z / mean / invstd / sums0: lists of n per-level tensors (z[l] None: no sums for level l), z[l] the level's OWN
    [B*H*W, C] tensor -> {"out": [(v, A)], "sums": [(v, A) or None]}"""
    out = {"out": [], "sums": []}
    for l in range(P.n):
        v, A = lvl(a, P, l) + lvl(b, P, l), lvl(a, P, l).abs() + lvl(b, P, l).abs()
        if c is not None:
            v, A = v + lvl(c, P, l), A + lvl(c, P, l).abs()
        out["out"].append((v, A))
        if z[l] is None:
            out["sums"].append(None)
            continue
        xh, s0 = (z[l] - mean[l]) * invstd[l], sums0[l]
        out["sums"].append((s0 + torch.cat([v.sum(0), (v * xh).sum(0)]).to(s0.dtype),
                            s0.abs() + torch.cat([A.sum(0), (A * xh.abs()).sum(0)]).to(s0.dtype)))
    return out


def slice_rows_pyr(P, src, N, offs):
    """mmd_slice_rows_pyr: dst[row0[l] + b*HW_l + r, :] = src[b, offs[l] + r*N : + N] (src [B, batch_stride]); padding rows zero"""
    dst = torch.zeros(P.Mt, N, dtype=src.dtype, device=src.device)
    for l, (H, W) in enumerate(P.sizes):
        dst[P.row0[l]:P.row0[l] + P.rows[l]] = src[:, offs[l]:offs[l] + H * W * N].reshape(P.rows[l], N)
    return dst


def dw_pyr_grouped(P, C, x, w_buf, sc_buf, sh_buf, ls, n, images, w_stride, bn_stride, in_act=1):
    """mmd_dwconv3_pyr under mmd_set_group: image b reads the taps of net b // images w_stride floats and its folded coefficients bn_stride
    floats behind net 0's (dw_fwd_kernel: `a.w + gw`, `a.in_scale + gb + lo`) - the nets evaluated one by one -> [(v, A)] per level"""
    out = []
    for l, (H, W) in enumerate(P.sizes):
        xl = lvl(x, P, l).view(P.B, H, W, C)
        ys = []
        for g in range(n):
            w = w_buf[g * w_stride:g * w_stride + 9 * C].view(9, C)
            sc, sh = (t[g * bn_stride + l * ls:g * bn_stride + l * ls + C] for t in (sc_buf, sh_buf))
            a, Aa = producer(xl[g * images:(g + 1) * images], sc, sh, None, in_act)
            ys.append(conv(a, Aa, w, 3, 1))
        out.append((torch.cat([y for y, _ in ys]).reshape(-1, C), torch.cat([A for _, A in ys]).reshape(-1, C)))
    return out


def pw_pyr_grouped(P, x, w_buf, bias_buf, K, N, n, images, w_stride, out_act=0, dot=None, bf16=False):
    """mmd_pwconv_fwd_pyr under mmd_set_group: the rows of net g's images take w and bias g * w_stride floats behind net 0's -> [(v, A)]"""
    out = []
    for l, (H, W) in enumerate(P.sizes):
        xl, per = lvl(x, P, l), images * H * W
        ys = [pw_fwd(xl[g * per:(g + 1) * per], w_buf[g * w_stride:g * w_stride + N * K].view(N, K), bias=bias_buf[g * w_stride:g * w_stride + N],
                     out_act=out_act, dot=dot, bf16=bf16)["y"] for g in range(n)]
        out.append((torch.cat([y for y, _ in ys]), torch.cat([A for _, A in ys])))
    return out


# ------------------------------------------------------------------------------------------------ the dispatch, copied
TH, TW = 8, 8                        # DwCfg<3, 1>: tile of the depthwise tile kernel and of the weight-gradient kernel


def wgrad_nsplit(P):
    """mmd_dwconv3_pyr_bwd_weight: blocks per (image, 64-channel chunk) of each level, clamp(ntiles / 8, 1, 16)"""
    return [max(1, min(16, cdiv(H, TH) * cdiv(W, TW) // 8)) for H, W in P.sizes]


def route_dw(P, C, flip, pro, dw_grad=False, bn_sums=False):
    """Which kernel(s) a mmd_dwconv3_pyr call launches: a COPY of its host code with no MMD_DW_* variable set.  Without a producer
    transform, with C >= 64 and W[0] >= 64 the row-streaming kernel (4 columns per thread, 4-row blocks) runs on EVERY level and carries the
    weight gradient and the BatchNorm-backward sums itself ("fused"); otherwise the tile kernel runs and they are two follow-up launches
    ("separate": mmd_dwconv3_pyr_bwd_weight, mmd_bn_bwd_reduce_pyr).  `flip` changes no decision.  Nothing checks the copy against the
    host code: keep it in step by hand.  -> {"kernel", "riders", "nsplit", "blocks"}"""
    rows = (not pro) and C >= 64 and P.sizes[0][1] >= 64
    cch = cdiv(C, 64)
    if rows:
        blocks = [P.B * cch * cdiv(W, 64) * cdiv(H, 4) for H, W in P.sizes]
    else:
        blocks = [P.B * cdiv(H, TH) * cdiv(W, TW) * cch for H, W in P.sizes]
    riders = None if not dw_grad else ("fused" if rows else "separate")
    return {"kernel": "rows" if rows else "tile", "riders": riders, "bn_sums": bool(bn_sums) and riders,
            "nsplit": wgrad_nsplit(P) if riders == "separate" else None, "blocks": blocks}


def route_pw(P, K, N, bf16=False, stats=False, strided=False):
    """pw_ref.route with M = row0[n] under a pyramid (pw_rows_try refuses a gate, pw_longk_try and pw_slab_try a pyramid) -> (label, record),
    label one of skinny / t128x32 / t64x64 / t128x64 / rows"""
    r = pw_ref.route(0, 0, int(bf16), P.Mt, K, N, stats=stats, remap=strided, pyr=True)
    label = r["family"] if r["family"] != "tiled" else "t%dx%d" % (r["bm"], r["bn"])
    return label, r


def group_tile_rows(P, K, N, bf16=False):
    """rows of the row tile the grouped mode checks every level against: 32 skinny, 64 on 64x64, else 128 (pw_dispatch)"""
    label, _ = route_pw(P, K, N, bf16)
    return {"skinny": 32, "t64x64": 64}.get(label, 128)


# ------------------------------------------------------------------------------------------------ cases
PYRAMIDS = {
    "p1": (2, [(7, 5)]),                                              # n = 1, 70 rows
    "p1x": (1, [(16, 8)]),                                            # n = 1, exactly 128 rows: no padding
    "p3": (2, [(5, 3), (3, 1), (2, 2)]),                              # W = 1
    "p5": (1, [(16, 8), (9, 15), (7, 5), (1, 3), (1, 1)]),            # n = 5: 128 rows exactly; 135 (> 128, not a multiple); 7x5; H = 1; 1x1 at B = 1 (127 padding rows)
    "prow": (2, [(9, 64), (5, 33), (3, 7), (1, 1)]),                  # W[0] = 64: row-streaming route, H % 4 != 0, narrow tail levels; level 0: 16 tiles (nsplit 2)
    "p63": (1, [(9, 63), (4, 4)]),                                    # W[0] = 63: the tile route; level 0: 16 tiles (nsplit 2)
    "pg": (2, [(8, 8), (4, 8)]),                                      # grouped nets: 64 and 32 rows per image, whole 32-row tiles
    "pgbad": (2, [(8, 8), (5, 3)]),                                   # 15 rows per image: breaks the tile condition
    "mid": (2, [(72, 72), (7, 5), (1, 1)]),                           # 83 row tiles: 64x64 tiles at N = 112, 224; level 0 = 81 * 128 rows exactly
    "big": (1, [(227, 226), (5, 7), (1, 1)]),                         # 403 row tiles, M = 51584 >= 32768: 128x64 (big_tiles 806), the row-slab kernel, 128x32
}


@functools.lru_cache(maxsize=None)
def pyr_of(name):
    return Pyr(*PYRAMIDS[name])


def bn_layout(C):
    """(lev_stride, channel offset): lev_stride > C and a non-zero offset into the arrays, as the engine passes them (multiples of 4)"""
    return 2 * C + 12, 12


DW_MODES = ("fwd_plain", "fwd_given", "fwd_live", "bwd_plain", "bwd_wg_plain", "bwd_wg_pro", "bwd_wg_bn")
WG_MODES = ("plain", "pro")
RED_MODES = [(act, out) for act in (1, 0) for out in (True, False)]                      # (act, g_out stored)
APP_MODES = [(rec, grads) for rec in (False, True) for grads in (True, False)]           # (g recomputed with scale / shift + swish, dgamma / dbeta given)
ADD_MODES = [(c, alias) for c in (False, True) for alias in (False, True)]               # (c given, out aliasing a)


def _c(entry, pyr, C, **kw):
    name = "%s_%s_c%d" % (entry, pyr, C) + "".join("_%s%s" % (k, v) for k, v in sorted(kw.items()) if k not in ("why", "route"))
    return dict({"name": name, "entry": entry, "pyr": pyr, "C": C}, **kw)


def _cases():
    cs = []
    # ---- mmd_dwconv3_pyr: every mode on every width over the n = 5 pyramid (tile route) and over the wide one (row route where no prologue)
    for C in WIDTHS + (8,):
        cs.append(_c("dw", "p5", C))
        cs.append(_c("dw", "prow", C))               # C = 8 with W[0] = 64: pins the C >= 64 branch (tile)
    for p in ("p1", "p1x", "p3", "p63"):
        cs.append(_c("dw", p, 112))
    # ---- mmd_dwconv3_pyr_bwd_weight
    for p, C in (("p5", 112), ("prow", 112), ("p63", 160), ("p3", 8), ("p1", 64), ("prow", 224)):
        cs.append(_c("wg", p, C))
    # ---- mmd_pwconv_fwd_pyr(_bf16): (K, N, bias, out_act, stats, strided)
    def pw(p, K, N, bias, act, stats, strided, route, route16=None):
        cs.append(_c("pw", p, K, N=N, bias=int(bias), act=act, stats=int(stats), strided=int(strided), route=(route, route16 or route)))
    for K in WIDTHS:
        pw("p5", K, K, True, 0, True, False, "skinny")
    pw("p5", 112, 36, True, 2, False, True, "skinny")
    pw("p5", 112, 36, False, 0, True, False, "skinny")
    pw("p5", 112, 12, False, 2, True, True, "t128x32")
    pw("p5", 112, 12, True, 0, True, False, "t128x32")               # dense [Mt, N]: the 127 padding rows of the 1x1 level lie inside the buffer
    pw("p5", 8, 36, True, 0, True, False, "skinny")
    for p in ("p1", "p1x", "p3"):
        pw(p, 112, 36, True, 2, False, True, "skinny")
        pw(p, 64, 64, False, 0, True, False, "skinny")
    pw("prow", 160, 36, True, 2, False, True, "skinny")
    pw("mid", 112, 112, True, 0, True, False, "t64x64")
    pw("mid", 224, 224, False, 0, True, True, "t64x64")
    pw("mid", 64, 36, True, 2, False, True, "skinny")
    pw("big", 112, 112, True, 0, True, True, "t128x64")
    pw("big", 112, 112, True, 2, False, True, "rows", "t128x64")
    pw("big", 112, 36, True, 2, False, True, "t64x64")
    pw("big", 112, N32_BIG, False, 0, True, True, "t128x32")
    # dense [Mt, N] outputs (the layout of the heads' intermediate layers) on the three variants above: every padding row is in the buffer
    pw("big", 112, 112, False, 0, True, False, "t128x64")
    pw("big", 112, 112, True, 0, False, False, "rows", "t128x64")
    pw("big", 112, N32_BIG, True, 0, True, False, "t128x32")
    # ---- the two BatchNorm passes
    for p, C in (("p5", 112), ("p5", 8), ("p3", 160), ("p1", 64), ("p1x", 224), ("prow", 112)):
        cs.append(_c("red", p, C))
        cs.append(_c("app", p, C))
    # ---- mmd_pyr_add_bnsums: zmask bit l = level l has a z tensor
    for p, C, zm in (("p5", 112, 0b10110), ("p5", 8, 0b11111), ("p3", 160, 0b101), ("p1", 64, 0b1), ("p1x", 224, 0b0), ("prow", 112, 0b1011)):
        cs.append(_c("add", p, C, zmask=zm))
    # ---- mmd_slice_rows_pyr: (N, parity of the offsets): all even = the vec 2 path
    for p in ("p5", "p1"):
        for N, odd in ((36, 0), (36, 1), (9, 0)):
            cs.append(_c("slice", p, 0, N=N, odd=odd))
    # ---- grouped nets
    cs.append(_c("gdw", "pg", 112))
    cs.append(_c("gpw", "pg", 112, N=36))
    return cs


def _n32(pname):
    """the smallest N > 16 whose GEMM over the pyramid takes 32-wide column tiles (derived from the route)"""
    P = Pyr(*PYRAMIDS[pname])
    for N in range(20, 257, 4):
        if pw_ref.route(0, 0, 0, P.Mt, 112, N, stats=True, remap=True, pyr=True).get("bn") == 32:
            return N
    raise AssertionError("no 32-wide N")


N32_BIG = _n32("big")
GROUP_N, GROUP_IMAGES = 2, 1
PYR_CASES = _cases()
CASE = {c["name"]: c for c in PYR_CASES}
assert len(CASE) == len(PYR_CASES)


def cases_of(*entries):
    return [c["name"] for c in PYR_CASES if c["entry"] in entries]


def modes_of(case):
    return {"dw": DW_MODES, "wg": WG_MODES, "pw": (False, True), "red": RED_MODES, "app": APP_MODES, "add": ADD_MODES, "slice": (None,),
            "gdw": (None,), "gpw": (False, True)}[case["entry"]]


def dw_route_of(case, mode):
    P = pyr_of(case["pyr"])
    return route_dw(P, case["C"], mode.startswith("bwd"), mode in ("fwd_given", "fwd_live"), mode.startswith("bwd_wg"), mode == "bwd_wg_bn")


# ------------------------------------------------------------------------------------------------ inputs
def rowbuf(g, P, C, mul=1.0, add=0.0):
    """[Mt, C] fp32: the levels' valid rows random, every padding row sentinel-sized finite garbage"""
    t = (torch.rand(P.Mt, C, generator=g) + 0.5) * SENTINEL
    for l in range(P.n):
        t[P.row0[l]:P.row0[l] + P.rows[l]] = torch.randn(P.rows[l], C, generator=g) * mul + add
    return t


def level_stats(P, x, C, ls, o):
    """float64 [2 * (o + n * ls)]: level l's [sum, sum of squares] of its own valid rows at 2 * (o + l * ls)"""
    st = torch.zeros(2 * (o + P.n * ls), dtype=torch.float64)
    for l in range(P.n):
        r = lvl(x, P, l).double()
        st[2 * (o + l * ls):2 * (o + l * ls) + 2 * C] = torch.cat([r.sum(0), (r * r).sum(0)])
    return st


@functools.lru_cache(maxsize=None)
def _inputs(name):
    case = CASE[name]
    P, C, e = pyr_of(case["pyr"]), case["C"], case["entry"]
    g = rng(61, P.Mt, C, sum(map(ord, name)) % 9973)
    rn = lambda *sh: torch.randn(*sh, generator=g)
    ru = lambda *sh: torch.rand(*sh, generator=g)
    ls, o = bn_layout(max(C, case.get("N", 0)))
    na = o + P.n * ls                                                       # per-level coefficients drawn independently
    d = {"ls": ls, "o": o}
    if e in ("dw", "wg", "red", "app"):
        d.update(x=rowbuf(g, P, C, 1.3, 0.2), dy=rowbuf(g, P, C), w=rn(9, C) / 3, scale=ru(na) + 0.5, shift=rn(na) * 0.2, mean=rn(na) * 0.2,
                 invstd=ru(na) + 0.5, gamma=ru(na) + 0.5, beta=rn(na) * 0.2, dw0=rn(9, C), sums0=rn(2 * na).double() * 3,
                 dgamma0=rn(na), dbeta0=rn(na))
        d["stats"] = level_stats(P, d["x"], C, ls, o)
        d["sums"] = rn(2 * na).double() * 3                                 # the apply pass' [sum g, sum g xhat]: its own input
    elif e == "pw":
        K, N = C, case["N"]
        d.update(x=rowbuf(g, P, K, 1.3, 0.2), w=rn(N, K) / math.sqrt(K), bias=rn(N) * 0.1, stats0=rn(2 * na).double() * 3)
        d["bstride"], d["yoff"] = head_layout(P, N)
    elif e == "add":
        d.update(a=rowbuf(g, P, C), b=rowbuf(g, P, C, 0.7, 0.1), c=rowbuf(g, P, C, 1.1))
        on = [bool(case["zmask"] >> l & 1) for l in range(P.n)]
        d["z"] = [rn(P.rows[l], C) * 1.2 + 0.1 if on[l] else None for l in range(P.n)]
        d["mean"] = [rn(C) * 0.2 if on[l] else None for l in range(P.n)]
        d["invstd"] = [ru(C) + 0.5 if on[l] else None for l in range(P.n)]
        d["sums0"] = [rn(2 * C).double() * 3 if on[l] else None for l in range(P.n)]
    elif e == "slice":
        N = case["N"]
        offs, a0 = [], 6 + case["odd"]
        for l, (H, W) in enumerate(P.sizes):
            offs.append(a0)
            a0 += H * W * N + 2 * (l + 1)                                   # (gaps between the levels' blocks)
        d.update(offs=offs, bstride=a0 + 4, src=rn(P.B, a0 + 4))
    elif e in ("gdw", "gpw"):
        N = case.get("N", C)
        ws, bs = N * C + 9 * C + 36, na + 20                                # larger than any parameter block: a kernel that ignores them reads filler
        d.update(w_stride=ws, bn_stride=bs, x=rowbuf(g, P, C, 1.3, 0.2), w_buf=rn(GROUP_N * ws) / (3 if e == "gdw" else math.sqrt(C)),
                 bias_buf=rn(GROUP_N * ws) * 0.1, sc_buf=ru(GROUP_N * bs) + 0.5, sh_buf=rn(GROUP_N * bs) * 0.2)
    return d


def head_layout(P, N):
    """(y_batch_stride, y_off_lev) of a concatenated [B, A_total * c] head output with a gap in front of and between the levels' blocks"""
    offs, a0 = [], 8
    for l, (H, W) in enumerate(P.sizes):
        offs.append(a0)
        a0 += H * W * N + 4 * (l + 1)
    return a0 + 8, offs


def case_inputs(case):
    """fp32 (float64 for raw sums) CPU tensors of one case, the same for the CPU calibration and the GPU test; cached - do not modify"""
    return _inputs(case["name"])


def _to(d, dt, dev):
    def cv(t):
        if isinstance(t, torch.Tensor):
            return t.to(dev) if t.dtype != torch.float32 else t.to(dev, dt)
        if isinstance(t, list):
            return [cv(v) for v in t]
        return t
    return {k: cv(v) for k, v in d.items()}


FAMILY = {("dw", "y"): "dw", ("dw", "y_live"): "dw_live", ("dw", "dw_grad"): "dwgrad", ("dw", "bn_sums"): "bnsums", ("wg", "dw"): "dwgrad",
          ("pw", "y"): "pw_y", ("pw", "sum"): "pw_sum", ("pw", "sumsq"): "pw_sumsq", ("red", "g"): "red_g", ("red", "sums"): "red_sums",
          ("app", "dz"): "app_dz", ("app", "dgamma"): "app_dsum", ("app", "dbeta"): "app_dsum", ("add", "out"): "add_out",
          ("add", "sums"): "add_sums", ("gdw", "y"): "dw", ("gpw", "y"): "pw_y"}


def family_of(case, mode, out):
    e = case["entry"]
    if e == "dw" and out == "y" and mode == "fwd_live":
        return "dw_live"
    f = FAMILY[(e, out)]
    return f + "_bf16" if e in ("pw", "gpw") and mode else f


def case_ref(case, mode, inp, dt, dev="cpu", model=False):
    """reference of one (case, mode) in dtype dt -> {output: [(value, A) per level] or (value, A)}.  Offsets: the arrays are sliced at the
    channel offset o (2 * o for double sums) as the kernel's pointers are.  model: the fp32 model's operation order (seq_dot, kernel order)"""
    d = _to(inp, dt, dev)
    P, C, e = pyr_of(case["pyr"]), case["C"], case["entry"]
    ls, o = inp["ls"], inp["o"]
    at = lambda k: d[k][o:]
    at2 = lambda k: d[k][2 * o:]
    if e == "dw":
        if mode == "fwd_plain":
            return dw_pyr(P, C, d["x"], d["w"], 0)
        if mode == "fwd_given":
            return dw_pyr(P, C, d["x"], d["w"], 0, ls, at("scale"), at("shift"), 1)
        if mode == "fwd_live":
            return dw_pyr(P, C, d["x"], d["w"], 0, ls, in_act=1, live=(at2("stats"), at("gamma"), at("beta")))
        if mode == "bwd_plain":
            return dw_pyr(P, C, d["dy"], d["w"], 1)
        if mode == "bwd_wg_plain":
            return dw_pyr(P, C, d["dy"], d["w"], 1, 0, wg=(d["x"], None, None, 0), dw0=d["dw0"])
        wg = (d["x"], at("scale"), at("shift"), 1)
        return dw_pyr(P, C, d["dy"], d["w"], 1, ls, wg=wg, dw0=d["dw0"], bn=(at("mean"), at("invstd"), at2("sums0")) if mode == "bwd_wg_bn" else None)
    if e == "wg":
        if mode == "plain":
            return {"dw": dw_wgrad_pyr(P, C, d["x"], d["dy"], d["dw0"])}
        return {"dw": dw_wgrad_pyr(P, C, d["x"], d["dy"], d["dw0"], ls, at("scale"), at("shift"), 1)}
    if e == "pw":
        kw = {"bf16": True} if (model and mode) else ({"dot": seq_dot} if model else {})
        return pw_pyr(P, d["x"], d["w"], d["bias"] if case["bias"] else None, case["act"], at2("stats0") if case["stats"] else None, ls, **kw)
    if e == "red":
        return bn_reduce_pyr(P, C, d["dy"], d["x"], at("scale"), at("shift"), at("mean"), at("invstd"), mode[0], ls, at2("sums0"))
    if e == "app":
        rec, grads = mode
        return bn_apply_pyr(P, C, d["dy"], d["x"], at("mean"), at("invstd"), at("gamma"), at2("sums"), ls, at("dgamma0") if grads else None,
                            at("dbeta0") if grads else None, at("scale") if rec else None, at("shift") if rec else None, int(rec), kernel_order=model)
    if e == "add":
        return add_bnsums(P, C, d["a"], d["b"], d["c"] if mode[0] else None, d["z"], d["mean"], d["invstd"], d["sums0"])
    if e == "gdw":
        return {"y": dw_pyr_grouped(P, C, d["x"], d["w_buf"], d["sc_buf"][o:], d["sh_buf"][o:], ls, GROUP_N, GROUP_IMAGES, inp["w_stride"], inp["bn_stride"])}
    if e == "gpw":
        kw = {"bf16": True} if (model and mode) else ({"dot": seq_dot} if model else {})
        return {"y": pw_pyr_grouped(P, d["x"], d["w_buf"], d["bias_buf"], C, case["N"], GROUP_N, GROUP_IMAGES, inp["w_stride"], **kw)}
    raise KeyError(e)


def flat_pairs(ref):
    """{output: value} -> [(output, level or None, (value, A))], the absent entries (a level without sums) dropped"""
    out = []
    for k, v in ref.items():
        if isinstance(v, list):
            out += [(k, l, p) for l, p in enumerate(v) if p is not None]
        else:
            out.append((k, None, v))
    return out


def ratio_u(got, ref, A, unit):
    """elt_ref.ratio in the family's unit: max |got - ref| / (unit * A + tiny)"""
    return ratio(got, ref, A * (unit / U))


def worst(got, ref, A, unit):
    """(ratio, index tuple) of the worst element"""
    r = (got.detach().double().cpu() - ref.detach().double().cpu()).abs() / (unit * A.detach().double().cpu() + TINY)
    if not r.numel():
        return 0.0, ()
    i, idx = int(r.reshape(-1).argmax()), []
    v = float(r.reshape(-1)[i])
    for n in reversed(r.shape):
        idx.append(i % n)
        i //= n
    return v, tuple(reversed(idx))
