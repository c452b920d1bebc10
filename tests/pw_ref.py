"""Helper (not a test): float64 restatement of the FORWARD 1x1-conv GEMM entry points of csrc/pw_gemm.hip - mmd_pwconv_fwd,
mmd_pwconv_fwd_form (forms 0 auto, 1 thin-K row-slab kernel, 2 LDS-tiled kernels, 3 long-K kernel; each with and without
MMD_PW_FORM_NATIVE) and mmd_pwconv_fwd_bf16 - written from the contract of pw_fwd_impl (PwArgs in pw_args.h, bn_live_coef in common.h),
not from the kernels' loops; a copy of the host dispatch (route); and the one case table (PW_CASES) that test_pw_ref_cpu.py and
test_gpu_pw_float64.py share.

The weight gradient - the grouped launch of pw_wgrad_grouped.hip and the per-layer mmd_pwconv_bwd_weight* entry points, their
BatchNorm-backward operand forms included - lives in wg_ref.py, which takes its X operand from pw_operand below.  The input gradient - the
mmd_pwconv_bwd_data* entry points with their BatchNorm-backward operand forms, the slab kernel's <PRO 1> instantiations included - lives in
bd_ref.py, whose plain launches are pw_fwd below with the sizes swapped.
The feature-pyramid launches mmd_pwconv_fwd_pyr(_bf16), with the grouped-nets mode (mmd_set_group) over a pyramid, live in pyr_ref.py, which
calls pw_fwd and route (pyr=True) below.
OUT OF SCOPE still (pw_fwd is the forward of every one of them): the grouped-nets mode (mmd_set_group) of mmd_pwconv_fwd, the stem
im2col GEMM (mmd_pw_stem_gemm) and the stem weight gradient (both in mb_ref.py, which calls pw_fwd below), the forward slab family (form 4 of mmd_pwconv_fwd_form, pw_slab.hip: route
names it where the auto form could take a launch, and no case may land there) and the MMD_STREAM dev kernel.

Conventions are those of elt_ref.py / dw_ref.py.  pw_fwd computes in the dtype (and on the device) of its tensor arguments: float64 is the
oracle, float32 the "plain fp32" evaluation that calibrates K.  It returns {"y", "sum", "sumsq"} of (value, A), A_i the magnitude of
what element i was built from:
  * operand a = gate * act(x*scale + shift): elt_ref.act_fwd carries |x*scale| + |shift| through the activation (|f| + |f'| A_u), the gate
    scales it; live coefficients are elt_ref.bn_finalize's (the shift's magnitude |beta| + |mean*scale|)
  * raw = a @ w^T + bias: A_raw = A_a @ |w|^T + |bias|
  * y = act(raw*out_scale + out_shift) + residual: A_raw * |out_scale| + |out_shift| through act_fwd, + |residual|
  * statistics (taken from raw, BEFORE out_scale; the kernels accumulate onto what is there): sum: |start| + sum_rows A_raw; sumsq:
    |start| + sum_rows (raw^2 + 2 |raw| A_raw) - the rounding of raw reaches raw^2 through its derivative.  (dw_ref uses sum |y|: a
    depthwise output is built from 9 or 25 terms and A ~ |y|; a K = 1248 dot product is not, and a sum cannot be asked to be more
    accurate than its terms.)
Errors are judged per element: |got - ref64| <= K * unit * A + tiny, unit 2^-24 (2^-9 for mmd_pwconv_fwd_bf16), K = max(8, 4 * K32) per
output family, K32 the largest error in that unit of the CPU model over every (case, mode) of PW_CASES (test_pw_ref_cpu.py measures it
and asserts that the constants below are the ones it gives):
  * fp32 model: prologue and epilogue in fp32, the dot product a strictly sequential fp32 chain over k (multiply, round, add, round) - the
    order with the most accumulator roundings of any kernel here (v_mfma_f32 chain: K; three-way bf16 split: 6 K / 16; the K-split skinny /
    long-K kernels and the 16x16x4 row-slab kernel: fewer per partial chain); statistics: float64 sums of the fp32 raw values
  * bf16 model: the post-prologue operand and the weight rounded to bf16, exact products (float64 sum of the rounded operands), fp32
    prologue / epilogue, against float64 of the UNROUNDED operands.
No constant comes from a GPU run of the kernels."""
import math

import torch

from elt_ref import act_fwd, rng, SENTINEL, bn_finalize, cdiv, U, TINY      # noqa: F401

UB = 2.0 ** -9                       # half a bf16 ulp of a value of size 1: the unit of the bf16 entry point
# K per family = max(8, 4 * K32).  K32 as test_pw_ref_cpu.py measures it (CPU models of the docstring on every case and mode):
K32 = {"y": 14.507, "sum": 0.692, "sumsq": 0.453, "y_bf16": 3.749, "sum_bf16": 0.325, "sumsq_bf16": 0.448}
K_BY_FAMILY = {"y": 59.0, "sum": 8.0, "sumsq": 8.0, "y_bf16": 15.0, "sum_bf16": 8.0, "sumsq_bf16": 8.0}
UNIT = {f: (UB if f.endswith("_bf16") else U) for f in K_BY_FAMILY}

MMD_PW_FORM_NATIVE = 16
# form label -> (entry point, form, native, bf16)
FORMS = {"auto": ("mmd_pwconv_fwd", 0, 0, 0), "f0": ("mmd_pwconv_fwd_form", 0, 0, 0), "f0n": ("mmd_pwconv_fwd_form", 0, 1, 0),
         "f1": ("mmd_pwconv_fwd_form", 1, 0, 0), "f1n": ("mmd_pwconv_fwd_form", 1, 1, 0), "f2": ("mmd_pwconv_fwd_form", 2, 0, 0),
         "f2n": ("mmd_pwconv_fwd_form", 2, 1, 0), "f3": ("mmd_pwconv_fwd_form", 3, 0, 0), "f3n": ("mmd_pwconv_fwd_form", 3, 1, 0),
         "bf16": ("mmd_pwconv_fwd_bf16", 0, 0, 1)}


# ------------------------------------------------------------------------------------------------ reference
def live_coef(stats, count, gamma, beta):
    """(scale, shift, A_shift) as bn_live_coef (common.h) derives them from raw batch sums with eps 1e-3: elt_ref.bn_finalize's"""
    v, m = bn_finalize(stats, count, gamma, beta)
    return v["scale"], v["shift"], m["shift"]


def seq_dot(a, w):
    """a @ w^T as a strictly sequential chain over k in the dtype of a: acc = round(acc + round(a_k * w_k))"""
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=a.dtype, device=a.device)
    wt = w.t().contiguous()
    for k in range(a.shape[1]):
        acc += a[:, k:k + 1] * wt[k:k + 1]
    return acc


def remap_index(M, N, rpi, y_batch_stride, y_offset, device="cpu"):
    """flat position of y[m, n] in the destination: image * y_batch_stride + y_offset + (row in image) * N + n"""
    m = torch.arange(M, device=device)
    return ((m // rpi) * y_batch_stride + y_offset + (m % rpi) * N).unsqueeze(1) + torch.arange(N, device=device)


def pw_operand(x, in_scale=None, in_shift=None, A_shift=None, in_act=0, gate=None, rpi=0):
    """the GEMM's X operand a = gate[row // rpi] * act(x*scale + shift) with its magnitude (the forward's and the weight gradient's)"""
    if in_scale is None:
        u, Au = x, x.abs()
    else:
        u, Au = x * in_scale + in_shift, (x * in_scale).abs() + (in_shift.abs() if A_shift is None else A_shift)
    a, Aa = act_fwd(u, Au, in_act)
    if gate is not None:
        gr = gate[torch.arange(x.shape[0], device=x.device) // rpi]
        a, Aa = a * gr, Aa * gr.abs()
    return a, Aa


def pw_fwd(x, w, in_scale=None, in_shift=None, A_shift=None, in_act=0, live=None, gate=None, rpi=0, bias=None, out_scale=None,
           out_shift=None, out_act=0, residual=None, stats0=None, dot=None, bf16=False):
    """pw_fwd_impl: y = act(raw*out_scale + out_shift) + residual, raw = (gate[row // rpi] * act(x*scale + shift)) @ w^T + bias,
    stats0 + [sum raw, sum raw^2].  live = (float64 sums [2K], count, gamma, beta) instead of in_scale / in_shift.  dot: the product
    (default a @ w^T); bf16: operand and weight rounded to bf16, exact products.  -> {"y", "sum", "sumsq"} of (value, A), y as [M, N]"""
    dt = x.dtype
    if live is not None:
        in_scale, in_shift, A_shift = live_coef(*live)
    a, Aa = pw_operand(x, in_scale, in_shift, A_shift, in_act, gate, rpi)
    if bf16:
        raw = (a.bfloat16().double() @ w.bfloat16().double().t()).to(dt)
    else:
        raw = a @ w.t() if dot is None else dot(a, w)
    Ar = Aa @ w.abs().t()
    if bias is not None:
        raw, Ar = raw + bias, Ar + bias.abs()
    out = {}
    if stats0 is not None:
        N = w.shape[0]
        out["sum"] = (stats0[:N] + raw.double().sum(0), stats0[:N].abs() + Ar.double().sum(0))
        out["sumsq"] = (stats0[N:] + (raw * raw).double().sum(0), stats0[N:].abs() + (raw * raw + 2 * raw.abs() * Ar).double().sum(0))
    t, At = raw, Ar
    if out_scale is not None:
        t, At = t * out_scale + out_shift, At * out_scale.abs() + out_shift.abs()
    t, At = act_fwd(t, At, out_act)
    if residual is not None:
        t, At = t + residual, At + residual.abs()
    out["y"] = (t, At)
    return out


# ------------------------------------------------------------------------------------------------ the dispatch, copied
# prologue kind -> (coefficients: None | "given" | "live", in_act)
PRO_KINDS = {"plain": (None, 0), "wide": (None, 0), "affine": ("given", 0), "given": ("given", 1), "live": ("live", 1), "swish": (None, 1)}
ROWS_NKK = (2, 3, 4, 6, 11, 12, 14, 15, 16)          # pw_rows.hip rows_pick_k: the K / 8 the row-slab kernel is instantiated for
RW_AFF, RW_SWISH, RW_GATE = 1, 2, 4
STATS_DEPTH = 128                                    # MMD_STATS_DEPTH (common.h)


def _rows(form, M, K, N, aff, act, gate, rpi, stats, slots_on, pyr=False):
    """pw_rows_try (pw_rows.hip:302-361); None: refused"""
    if K < 16 or K > 128 or K & 7:                                                    # :307
        return None
    if form in (2, 3, 4):                                                             # :313
        return None
    if form != 1 and (M < 32768 or stats or N < 48):                                  # :314
        return None
    if gate and (pyr or rpi & 15):                                                    # :316 (a pyramid launch with a gate is refused)
        return None
    nkk, tiles, nslabs = K // 8, cdiv(N, 16), cdiv(M, 16)                             # :317-319
    C, best = 1, -1.0
    for c in (7, 4, 3, 1):                                                            # :321-327
        eff = tiles / (cdiv(tiles, c) * c) * (0.85 if c == 1 else 1.0)
        if eff > best + 1e-9:
            best, C = eff, c
    C_rule = C
    if nslabs * cdiv(tiles, C) < 512 and nslabs < 512:                                # :329 small_slabs
        C = 1
    if nkk not in ROWS_NKK:                                                           # :330-331
        return None
    LDB, nchunks = K + 4, cdiv(tiles, C)
    cpp = max(1, (120 * 1024) // (C * 16 * LDB * 4))                                  # :336-337
    cpp = min(cpp, nchunks)
    while cpp > 1 and nslabs * cdiv(nchunks, cpp) < 1024:                             # :338
        cpp -= 1
    pcols, npanels = cpp * C * 16, cdiv(nchunks, cpp)
    nlev = 1 if stats else 0
    if (pcols * LDB + 2 * K + 3 * pcols + nlev * 2 * pcols) * 4 > 150 * 1024:         # :344-345
        return None
    maxblk = 256
    if stats and not slots_on and maxblk > 128 * npanels:                             # :350
        maxblk = 128 * npanels
    bpp = min(max(1, maxblk // npanels), cdiv(nslabs, 8))                             # :351-352
    return {"family": "rows", "variant": C, "C": C, "C_rule": C_rule, "small_slabs": C != C_rule, "nkl": nkk, "mfma": "f32",
            "pro": (RW_AFF if aff else 0) | (RW_SWISH if act else 0) | (RW_GATE if gate else 0), "cpp": cpp, "npanels": npanels, "bpp": bpp,
            "nblk": npanels * bpp, "row_tail": M % 16, "col_tail": N % (C * 16), "slotted": slots_on}


def _longk(form, bf16, M, K, N, xf, gate, rpi, slots_on, remap, pyr=False):
    """pw_longk_try (pw_longk.hip:216-239); None: refused"""
    if form in (2, 1, 4) or bf16 or remap or pyr:                                     # :218
        return None
    if xf or slots_on:                                                                # :219-220
        return None
    if K < 256 or K > 3072 or N < 4:                                                  # :222
        return None
    if gate and rpi % 32:                                                             # :223
        return None
    blocks = cdiv(M, 32) * cdiv(N, 64)                                                # :224
    if form != 3 and (K < 512 or blocks > 256):                                       # :228
        return None
    return {"family": "longk", "variant": 0, "nkl": None, "mfma": "f32", "pro": 4 if gate else 3, "nblk": blocks, "ksteps": cdiv(K, 128),
            "k_tail": K % 128, "k_tail_chunks": (K % 128) // 4, "half_group": K % 8 == 4, "row_tail": M % 32, "col_tail": N % 64,
            "slotted": False}


def route(form, native, bf16, M, K, N, pro="plain", gate=False, stats=False, ws_slots=0, remap=False, residual=False, rpi=0, split_default=True,
          pyr=False):
    """Which kernel instantiation and geometry a forward call reaches: a COPY of the host decisions of pw_fwd_impl / pw_dispatch
    (pw_gemm.hip), pw_rows_try (pw_rows.hip) and pw_longk_try (pw_longk.hip), with no MMD_* variable set (split_default False: MMD_MFMA_F32).
    Nothing checks the copy against the host code: keep it in step by hand when the dispatch changes.  `residual` changes no decision.
    pyr: a pyramid launch (pyr_ref.py, M = row0[n]) - pw_rows_try then refuses a gate, pw_longk_try and pw_slab_try the launch."""
    aff, act = PRO_KINDS[pro]
    xf = aff is not None or act != 0
    ntm = cdiv(M, 128)
    big = ntm * cdiv(N, 64)                                                           # pw_gemm.hip:1154 big_tiles
    slots_on = bool(stats and ws_slots > 1 and ntm > STATS_DEPTH)                     # :1099
    take_skinny = big < 160 and N > 16                                                # :1170 (MMD_SKINNY_K 0, MMD_SKINNY_TILES 160, MMD_SQ_MIN 160)
    gain = 20 if bf16 else 10                                                         # :1172
    pad64, pad32 = cdiv(N, 64) * 64, cdiv(N, 32) * 32
    variant = 0 if take_skinny else (1 if (N <= 32 or ((pad64 - pad32) * 100 > gain * N and not big < 800)) else (2 if big < 800 else 3))   # :1174-1176
    if form == 0 and not bf16 and not remap and not pyr and not slots_on and take_skinny and N > 64 and K >= 256 and xf and N > 224:      # :1197, pw_slab_try
        return {"family": "slab", "big_tiles": big}                                   # out of scope: whether it takes the launch is slab_plan's
    r = None if bf16 else _rows(form, M, K, N, aff, act, gate, rpi, stats, slots_on, pyr)                                    # :1204
    r = r or _longk(form, bf16, M, K, N, xf, gate, rpi, slots_on, remap, pyr)                                                 # :1206
    if r:
        r["big_tiles"] = big
        return r
    lean = 0 if xf else (4 if gate else 3)                                            # :1215-1216, :1236-1237
    if variant == 0:                                                                  # :1212-1229; the skinny kernel adds to a.stats itself, a workspace stays zero
        return {"family": "skinny", "variant": 0, "bm": 32, "bn": 64, "nkl": None, "mfma": "bf16" if bf16 else "f32", "pro": lean,
                "ntn": cdiv(N, 64), "ntm": cdiv(M, 32), "nblk": cdiv(M, 32) * cdiv(N, 64), "row_tail": M % 32, "col_tail": N % 64,
                "ksteps": cdiv(K, 128), "k_tail": K % 128, "short_k": K < 128 and K // 32 < 3, "half_group": K % 8 == 4, "slotted": False,
                "big_tiles": big}
    nkl = ((K - 1) % 32) // 8 + 1                                                     # :1231
    mfma = "bf16" if bf16 else ("split" if (split_default and not native and K >= 64 and N > 48) else "f32")                 # :1232-1233
    bm, bn = {1: (128, 32), 2: (64, 64), 3: (128, 64)}[variant]                       # :1242-1258
    return {"family": "tiled", "variant": variant, "bm": bm, "bn": bn, "nkl": nkl, "mfma": mfma, "pro": lean, "ntn": cdiv(N, bn),
            "ntm": cdiv(M, bm), "nblk": cdiv(M, bm) * cdiv(N, bn), "row_tail": M % bm, "col_tail": N % bn, "ksteps": cdiv(K, 32),
            "half_group": K % 8 == 4, "slotted": slots_on, "big_tiles": big}


# ------------------------------------------------------------------------------------------------ cases
# mode = (prologue kind, gate, epilogue).  Epilogues:
EPI = {"0": {}, "b": {"bias": 1}, "s": {"bias": 1, "stats": 1}, "sw": {"bias": 1, "stats": 1, "ws": 64}, "osc": {"osc": 1},
       "sig": {"bias": 1, "act": 2}, "sw1": {"act": 1}, "res": {"res": 1}, "acc": {"res": 1, "acc": 1}, "remap": {"bias": 1, "act": 2, "remap": 1},
       "full": {"bias": 1, "stats": 1, "osc": 1, "act": 1, "res": 1}, "fullw": {"bias": 1, "stats": 1, "ws": 64, "osc": 1, "act": 1, "res": 1}}
REMAP_OFFSET, REMAP_SLACK = 68, 136          # y_offset and what a destination image is longer than rpi * N (both multiples of 4 floats)


def _c(name, M, K, N, B, forms, fam, modes, why):
    assert M % B == 0
    return {"name": name, "M": M, "K": K, "N": N, "B": B, "rpi": M // B, "forms": forms, "fam": fam, "modes": modes, "why": why}


P0, PG, PX = ("plain", False, "0"), ("plain", True, "b"), ("given", True, "full")
LEAN3 = [P0, PG, PX]                                         # lean plain (PRO 3), lean gated (PRO 4), non-lean (PRO 0) with the whole epilogue
NONLEAN = [("affine", False, "osc"), ("live", False, "s"), ("swish", False, "sig")]
T3 = ["f2", "f2n", "bf16"]
# row-slab cases: M = 8192 in 8 images (rows_per_image % 16 == 0: gated modes) alternating with M = 8200 in one image (a partial slab)
ROWS_MODES = [[[PG, ("given", True, "full")], [("plain", True, "acc"), ("swish", True, "sig")]],
              [[P0, ("live", False, "s")], [("affine", False, "osc"), ("given", False, "res")]]]
PW_CASES = [
    # ---- the 128x32 tile on one block: every K % 32 (nkl 1..4, each with and without the half 8-wide group), fp32 MFMA
    *[_c("t1_k%d" % K, 100, K, 16, 4, T3, "tiled", [P0] + ([PG, PX] if K in (12, 32) else []),
         "pw_gemm<128,32,nkl %d> fp32 MFMA, K %% 32 = %d, one block with 100 of 128 rows; N <= 16 is never skinny" % (((K - 1) % 32) // 8 + 1, K % 32))
      for K in (4, 8, 12, 16, 20, 24, 28, 32, 36)],
    _c("t1_nonlean", 100, 12, 16, 4, T3 + ["auto", "f0", "f0n"], "tiled", NONLEAN, "pw_gemm<128,32,2,PRO 0>: affine only, live, swish only"),
    _c("t1_m1", 1, 8, 16, 1, T3, "tiled", [P0, ("live", False, "s")], "pw_gemm<128,32>: M = 1"),
    _c("t1_m33", 33, 20, 12, 3, T3, "tiled", [P0, PG, ("plain", False, "remap")], "pw_gemm<128,32>: M = 33, N = 12; remap with N below the tile width"),
    _c("t1_n4", 100, 12, 4, 4, T3, "tiled", [P0, ("plain", False, "s")], "pw_gemm<128,32>: N = 4, one column quad (N % 32 = 4)"),
    _c("t1_acc", 260, 40, 16, 4, T3, "tiled", [("plain", False, "acc"), ("plain", False, "res")], "pw_gemm<128,32>: three row blocks, the output aliasing the residual"),
    # ---- skinny 32x64 kernel: K % 32, K shorter than the four-wave K split, tails
    *[_c("sk_k%d" % K, 300, K, 40, 4, T3, "skinny", [P0] + ([PG, PX] if K in (24, 160) else []),
         "pw_gemm_skinny: K = %d (K %% 32 = %d%s), 10 row blocks, row tail 12, col tail 40 of 64" % (K, K % 32, ", shorter than the four-wave K split" if K < 128 else ""))
      for K in (4, 8, 12, 16, 20, 24, 28, 32, 132, 160, 260)],
    _c("sk_nonlean", 300, 24, 40, 4, T3 + ["auto", "f0", "f0n"], "skinny", NONLEAN + [("plain", False, "acc")], "pw_gemm_skinny<PRO 0>: affine only, live, swish only; aliasing"),
    _c("sk_m1", 1, 24, 40, 1, T3, "skinny", [P0, ("live", False, "s")], "pw_gemm_skinny: M = 1"),
    _c("sk_m33", 33, 24, 68, 3, T3, "skinny", [P0, PG, PX], "pw_gemm_skinny: M = 33 (row tail 1), N = 68: N % 64 = 4, two column tiles"),
    _c("sk_remap", 96, 112, 36, 2, T3 + ["auto"], "skinny", [("plain", False, "remap"), ("given", True, "remap")], "pw_gemm_skinny: strided head output, non-zero y_offset, N = 36"),
    _c("sk_159", 20352, 16, 64, 4, T3 + ["auto"], "skinny", [P0, ("plain", False, "s")], "big_tiles 159: the last skinny shape, 636 row blocks"),
    # ---- 64x64 tiles (160 <= big_tiles < 800)
    _c("t2_160", 20480, 16, 64, 4, T3 + ["auto"], "tiled", [P0, ("plain", False, "s")], "big_tiles 160: the first 64x64 shape, nkl 2, fp32 MFMA"),
    _c("t2_k96", 20480, 96, 64, 4, T3 + ["auto", "f0", "f0n"], "tiled", LEAN3 + [("plain", False, "sw"), ("plain", False, "s"), ("given", False, "fullw")],
       "pw_gemm<64,64,nkl 4> split form (K >= 64, N > 48) / v_mfma_f32 under `native`; slotted sums with ws_slots 64 and direct"),
    *[_c("t2_k%d" % K, 20400, K, 52, 4, T3, "tiled", LEAN3, "pw_gemm<64,64,nkl %d> split / native / bf16, N = 52, row tail 48" % (((K - 1) % 32) // 8 + 1))
      for K in (72, 76, 84)],
    _c("t2_k60_n64", 20480, 60, 64, 4, T3, "tiled", [P0], "below the split-form switch: K = 60"),
    _c("t2_k64_n48", 20400, 64, 48, 4, T3, "tiled", [P0], "below the split-form switch: N = 48"),
    _c("t2_k64_n52", 20400, 64, 52, 4, T3, "tiled", LEAN3, "above the split-form switch: K = 64, N = 52, nkl 4"),
    _c("t2_n68", 10200, 72, 68, 4, T3, "tiled", [P0, ("wide", False, "0")], "pw_gemm<64,64>: N % 64 = 4, two column tiles; eight decades"),
    # ---- 128x32 tiles by the padding rule (big_tiles >= 800)
    _c("t1_pad208", 25500, 40, 208, 4, T3 + ["auto"], "tiled", [P0, ("given", False, "full")], "big_tiles 800: fp32 128x32 (gain 10), bf16 128x64 (gain 20)"),
    _c("t1_pad88", 51100, 40, 88, 4, T3, "tiled", [P0, PG], "128x32 by the padding rule, col tail 24 of 32, nkl 1"),
    *[_c("t1_k%d" % K, 51100, K, 68, 4, T3, "tiled", LEAN3, "pw_gemm<128,32,nkl %d> split / native / bf16, N %% 32 = 4, row tail 28" % (((K - 1) % 32) // 8 + 1))
      for K in (68, 80, 88, 96)],
    # ---- 128x64 tiles (big_tiles >= 800)
    _c("t3_801", 34100, 64, 192, 4, T3 + ["auto"], "tiled", [P0, ("wide", False, "0")], "big_tiles 801: 128x64, row tail 52, split form; eight decades"),
    *[_c("t3_k%d" % K, 11300, K, 576, 4, T3, "tiled", LEAN3, "pw_gemm<128,64,nkl %d> split / native / bf16, row tail 36" % (((K - 1) % 32) // 8 + 1))
      for K in (72, 80, 84, 96)],
    # ---- form 1: the thin-K row-slab kernel, every <K / 8, C> instantiation
    *[_c("rows_k%d_c%d" % (K, C), 8200 if i % 2 else 8192, K, Nn, 1 if i % 2 else 8, ["f1"] + (["f1n"] if K == 16 else []), "rows",
         ROWS_MODES[i % 2][j % 2], "pw_rows<%d,%d>: chunk width %d, M %% 16 = %d" % (K // 8, C, C, 8 if i % 2 else 0))
      for i, K in enumerate(8 * n for n in ROWS_NKK) for j, (C, Nn) in enumerate(((7, 112), (4, 64), (3, 44), (1, 16)))],
    _c("rows_small", 48, 112, 36, 1, ["f1"], "rows", [("plain", False, "b"), ("plain", False, "remap")], "pw_rows<14,1>: the small_slabs override (rule 3 -> 1), 3 slabs; remap"),
    _c("rows_panels", 2048, 128, 352, 8, ["f1"], "rows", [P0, PG], "pw_rows<16,4>: six panels of one chunk"),
    _c("rows_panels7", 8200, 128, 528, 1, ["f1"], "rows", [P0, ("plain", False, "s")], "pw_rows<16,3>: eleven chunks, three panels of up to four chunks"),
    _c("rows_slotted", 16400, 24, 48, 1, ["f1"], "rows", [("plain", False, "sw"), ("live", False, "sw")], "pw_rows<3,3>: slotted statistics"),
    _c("rows_auto", 32800, 16, 48, 1, ["auto", "f0"], None, [P0, ("given", False, "osc")], "the auto form's shape filter: M >= 32768, no statistics, N >= 48"),
    _c("rows_refused_k132", 8192, 132, 112, 8, ["f1", "f1n"], "skinny", [P0, PG], "K = 132 > 128: pw_rows_try refuses, the skinny kernel runs"),
    _c("rows_refused_gate", 8200, 112, 112, 8, ["f1", "f1n"], "skinny", [PG], "gate with rows_per_image = 1025: pw_rows_try refuses"),
    _c("rows_refused_k40", 20480, 40, 64, 4, ["f1"], "tiled", [P0], "K / 8 = 5 has no instantiation: pw_rows_try refuses, 64x64 tiles run"),
    # ---- form 3: the long-K kernel
    _c("lk_k256", 2048, 256, 64, 8, ["f3", "f3n"], "longk", [PG, P0], "pw_longk: two K steps, tail 0, gate"),
    _c("lk_k528", 1024, 528, 88, 4, ["f3"], "longk", [("plain", True, "osc"), ("plain", True, "res")], "pw_longk<4>: K tail 16, N tail 24"),
    _c("lk_k720", 1050, 720, 120, 1, ["f3", "auto", "f0"], "longk", [P0, ("plain", False, "s"), ("plain", False, "acc")], "pw_longk<3>: K tail 80, row tail, statistics, aliasing"),
    _c("lk_k260", 100, 260, 36, 1, ["f3"], "longk", [P0, ("plain", False, "sig")], "pw_longk<3>: K % 8 = 4 (K tail 4), row tail 4"),
    _c("lk_n4", 96, 388, 4, 3, ["f3"], "longk", [("plain", False, "sig"), PG], "pw_longk: N = 4, K % 8 = 4"),
    _c("lk_refused_k252", 100, 252, 36, 1, ["f3", "f3n"], "skinny", [P0], "K = 252 < 256: pw_longk_try refuses, the skinny kernel runs"),
]
CASE = {c["name"]: c for c in PW_CASES}
assert len(CASE) == len(PW_CASES)


def mode_label(mode):
    return "%s%s-%s" % (mode[0], "+gate" if mode[1] else "", mode[2])


def route_mode(case, mode, flabel, split_default=True):
    _, form, native, bf16 = FORMS[flabel]
    e = EPI[mode[2]]
    return route(form, native, bf16, case["M"], case["K"], case["N"], pro=mode[0], gate=mode[1], stats=bool(e.get("stats")),
                 ws_slots=e.get("ws", 0), remap=bool(e.get("remap")), residual=bool(e.get("res")), rpi=case["rpi"], split_default=split_default)


# ------------------------------------------------------------------------------------------------ inputs
def case_inputs(case, wide=False):
    """fp32 (float64 for the raw sums) CPU tensors of one case; the same for the CPU calibration and the GPU test.  wide: both operands
    spread over eight decades (as test_split3_precision)"""
    M, K, N, B = case["M"], case["K"], case["N"], case["B"]
    g = rng(23, M, K, N, B, int(wide))
    rn = lambda *sh: torch.randn(*sh, generator=g)
    x, w = rn(M, K) * 1.3 + 0.2, rn(N, K) / math.sqrt(K)
    if wide:
        x = x * torch.exp2(torch.randint(-13, 14, (M, K), generator=g).float())
        w = w * torch.exp2(torch.randint(-13, 14, (N, K), generator=g).float())
    rows = x if M >= 32 else torch.cat([x, rn(64 - M, K) * 1.3 + 0.2])      # (below 32 rows: no degenerate statistics, as elt_ref.bn_inputs)
    gamma, beta = torch.rand(K, generator=g) + 0.5, rn(K) * 0.2
    r64 = rows.double()
    in_stats = torch.cat([r64.sum(0), (r64 * r64).sum(0)])
    v, _ = bn_finalize(in_stats, rows.shape[0], gamma.double(), beta.double())
    return {"x": x, "w": w, "gamma": gamma, "beta": beta, "in_stats": in_stats, "in_count": rows.shape[0], "scale": v["scale"].float(),
            "shift": v["shift"].float(), "gate": torch.rand(B, K, generator=g) * 0.9 + 0.05, "bias": rn(N) * 0.1,
            "osc": torch.rand(N, generator=g) + 0.5, "osh": rn(N) * 0.2, "res": rn(M, N), "stats0": rn(2 * N).double() * 3}


def _to(d, dt, dev):
    return {k: (t.to(dev) if t.dtype != torch.float32 else t.to(dev, dt)) if isinstance(t, torch.Tensor) else t for k, t in d.items()}


def ref_kwargs(case, mode, d):
    """the keyword arguments of pw_fwd for one mode, from the input dict d (any dtype / device)"""
    pro, gate, epi = mode
    aff, act = PRO_KINDS[pro]
    e = EPI[epi]
    kw = {"in_act": act, "rpi": case["rpi"], "out_act": e.get("act", 0)}
    if aff == "given":
        kw.update(in_scale=d["scale"], in_shift=d["shift"])
    elif aff == "live":
        kw.update(live=(d["in_stats"], d["in_count"], d["gamma"], d["beta"]))
    if gate:
        kw["gate"] = d["gate"]
    if e.get("bias"):
        kw["bias"] = d["bias"]
    if e.get("osc"):
        kw.update(out_scale=d["osc"], out_shift=d["osh"])
    if e.get("res"):
        kw["residual"] = d["res"]
    if e.get("stats"):
        kw["stats0"] = d["stats0"]
    return kw


def case_ref(case, mode, inp, dt, dev="cpu", **model):
    """reference of one (case, mode) in dtype dt -> {"y", "sum", "sumsq"} of (value, A); model: dot= / bf16= of pw_fwd"""
    d = _to(inp, dt, dev)
    return pw_fwd(d["x"], d["w"], **ref_kwargs(case, mode, d), **model)


def inputs_of(case, mode):
    return case_inputs(case, wide=mode[0] == "wide")


# ------------------------------------------------------------------------------------------------ shared by the GPU test modules
GPU_ERROR = []          # a launch or runtime error met by an earlier test: nothing more is launched on a device that may have faulted


class Out:
    """an output tensor of `shape` followed by 16 guard rows; fill: 'nan' (must be overwritten), 'sent' (the sentinel: only a window of it
    is written) or a CPU tensor (must be accumulated on)"""

    def __init__(self, shape, fill, dtype=torch.float32, device="cuda"):
        n = math.prod(shape)
        self.n = n
        self.buf = torch.full((n + 16 * shape[-1],), SENTINEL, dtype=dtype, device=device)
        self.t = self.buf[:n].view(shape)
        if isinstance(fill, str):
            if fill == "nan":
                self.t.fill_(float("nan"))
        else:
            self.t.copy_(fill.to(dtype))

    def get(self):
        assert bool((self.buf[self.n:] == SENTINEL).all()), "guard rows behind the output were written"
        return self.t
