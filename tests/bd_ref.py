"""Helper (not a test): float64 restatement of the 1x1-conv INPUT GRADIENT entry points of csrc/pw_gemm.hip / pw_slab.hip - mmd_pwconv_bwd_data,
_bf16, mmd_pwconv_bwd_data_bn, _bn_bf16, mmd_pwconv_bwd_data_bn2, _bn2_bf16 and mmd_pwconv_bwd_data_bn2_form (forms 0 auto, 2 LDS-tiled kernels,
4 all-N K-sliced slab kernel; each with and without MMD_PW_FORM_NATIVE) - written from the contracts in include/mmdistill.h and the header
comments of pw_args.h (BnBwdOp, BnSumOp, Pool5Op), not from the kernels' loops; a copy of the host decisions for a BatchNorm-operand launch
(route, slab_plan); and the case tables (BD_CASES, PLAIN_CASES) that test_bd_ref_cpu.py and test_gpu_bd_float64.py share.

SIZES follow the C ABI: a conv with M rows, K input and N output channels; g, z, dz_out are [M, N], wt is [K, N], dx [M, K].  The GEMM inside
reduces over N and writes K columns: Kg = N is the REDUCTION LENGTH, Ng = K the OUTPUT WIDTH.  Everything that speaks of the dispatch (route,
the case table, the names of the cases) uses Kg / Ng; a case carries both spellings.

OUT OF SCOPE here: the w16 storage flags of pw_bwd_data_bn2_impl (no public entry point), the grouped-nets mode, MMD_SK_BQ_LDS / MMD_SK_PF2 and
the other dispatch variables (test_bd_ref_cpu.py asserts that none is set), the fused expand backward (mmd_mbconv_expand_bwd_fused: mb_ref.py,
which takes xs_ref below).

Conventions are those of elt_ref.py / pw_ref.py / wg_ref.py.  bd_fwd computes in the dtype (and on the device) of its tensor arguments: float64 is
the oracle, float32 the model that calibrates K.  It returns a dict of (value, A), A_i the magnitude of what element i was built from:
  * dz [M, N]: wg_ref.bn_operand - the evaluated BatchNorm backward dz = scale*(g' - m1 - xhat*m2), g' = g * mul_b[image] * act'(z*scale + shift),
    m = sums / count.  `sums` are float64 numbers the kernel is handed: the test computes them with elt_ref.bn_bwd_reduce in float64 (case_sums),
    not with mmd_bn_bwd_reduce
  * dx [M, K] = dz @ W (+ residual), A = A_dz @ |W| + |residual|
  * dgamma = d0 + sums[N:], dbeta = d0 + sums[:N], A = |d0| + |sums| (as wg_ref)
  * xs_sum / xs_sumsq [K] = the two halves of xs_sums: start + [sum g', sum g' * xhat'] over the COMPLETED dx, g' = dx * xs_mul_b[image],
    xhat' = (xs_z - xs_mean) * xs_invstd.  The kernel sums its own fp32 dx, so the rounding of dx reaches the sums:
    A = |start| + sum A_dx |mul_b| and |start| + sum A_dx |mul_b| |xhat'| (pw_ref does the same for sumsq)
  * p5 [5][p5_B][K] = elt_ref.chan_pool_bwd with g1 = dx: start + sum (g1*a, g1*s', g1*s'*xhat, s', s'*xhat); A_dx in place of |g1| in the
    three planes that contain g1
  * the plain entry points are pw_ref.pw_fwd with the sizes swapped (plain_ref).
Errors are judged per element, none left out: |got - ref64| <= K * unit * A + tiny, unit 2^-24; K = max(8, ceil(4 * K32)) per output family,
K32 the largest error in that unit of the CPU model over every (case, mode) of the tables (test_bd_ref_cpu.py measures it and asserts that the
K32 stored below is the one it gives to within 5 % + 0.01, that no model exceeds K / 4 and that K is the ceiling of four times the stored K32;
below K32 = 2 the floor K = 8 decides and the stored value is not compared):
  * fp32 model: dz in fp32 in the kernel's operation order a1*g' + a2*(z - mu) + a3 (bn_operand(kernel_order=True)); the product a strictly
    sequential fp32 chain over Kg (pw_ref.seq_dot: the order with the most accumulator roundings of any kernel here), the residual added last;
    the upstream sums and the pool planes float64 sums of fp32 terms taken from the fp32 dx
  * bf16 entry points (families *_bf16, unit 2^-9): both MFMA operands - dz and W - rounded to bf16, exact products, fp32 prologue, against
    float64 of the UNROUNDED operands.  dz_out, dgamma and dbeta of a bf16 entry point are fp32 values that no bf16 rounding has touched: they
    are judged in the fp32 families "dz" / "dsum", which is the stricter reading.
No constant comes from a GPU run of the kernels."""
import math

import torch

from elt_ref import bn_bwd_reduce, chan_pool_bwd, swish, dswish, bn_inputs, rng, randn, rand, cdiv, U, TINY, SENTINEL      # noqa: F401
from pw_ref import pw_fwd, seq_dot, UB, Out, GPU_ERROR, MMD_PW_FORM_NATIVE      # noqa: F401
import pw_ref
from wg_ref import bn_operand

# K per family = max(8, ceil(4 * K32)).  K32 as test_bd_ref_cpu.py measures it (CPU models of the docstring on every case and mode):
K32 = {"dx": 5.811, "dz": 8.660, "dsum": 1.885, "xs_sum": 0.650, "xs_sumsq": 0.413, "p5": 1.082,
       "dx_bf16": 2.473, "xs_sum_bf16": 0.371, "xs_sumsq_bf16": 0.252, "p5_bf16": 0.244}
K_BY_FAMILY = {"dx": 24.0, "dz": 35.0, "dsum": 8.0, "xs_sum": 8.0, "xs_sumsq": 8.0, "p5": 8.0,
               "dx_bf16": 10.0, "xs_sum_bf16": 8.0, "xs_sumsq_bf16": 8.0, "p5_bf16": 8.0}
UNIT = {f: (UB if f.endswith("_bf16") else U) for f in K_BY_FAMILY}
BF16_FAMILIES = ("dx", "xs_sum", "xs_sumsq", "p5")          # the outputs that the bf16 rounding of the MFMA operands reaches

BN_RPI, XS_RPI = 7, 5          # rows_per_image of mul_b / xs_mul_b: neither divides a 32-, 64- or 128-row tile
STATS_DEPTH = 128              # MMD_STATS_DEPTH (common.h)
PW_BM = 128


# ------------------------------------------------------------------------------------------------ reference
def _img(M, rpi, device):
    return torch.arange(M, device=device) // rpi


def xs_ref(dx, A_dx, xs, bf=False):
    """the two halves of xs_sums: start + [sum g', sum g' * xhat'], g' = dx * mul_b[image]; float64 sums of terms in the dtype of dx"""
    K = dx.shape[1]
    gp, Ag = dx, A_dx
    if xs.get("mul_b") is not None:
        mb = xs["mul_b"][_img(dx.shape[0], xs["rpi"], dx.device)].unsqueeze(1)
        gp, Ag = dx * mb, A_dx * mb.abs()
    xh = (xs["z"] - xs["mean"]) * xs["invstd"]
    t2 = gp * (xs["z"] - xs["mean"]) * xs["invstd"]
    s0 = xs["sums0"]
    sfx = "_bf16" if bf else ""
    return {"xs_sum" + sfx: (s0[:K] + gp.double().sum(0), s0[:K].abs() + Ag.double().sum(0)),
            "xs_sumsq" + sfx: (s0[K:] + t2.double().sum(0), s0[K:].abs() + (Ag * xh.abs()).double().sum(0))}


def p5_ref(dx, A_dx, p5):
    """[5][B][K]: elt_ref.chan_pool_bwd with g1 = dx (float64: chan_pool_bwd itself; the fp32 model: float64 sums of its fp32 terms), A_dx
    carried through the three planes that contain g1"""
    B, rpi, K = p5["B"], dx.shape[0] // p5["B"], dx.shape[1]
    z, out0 = p5["z"], p5["out0"]
    u = z * p5["scale"] + p5["shift"]
    a, sp, xh = swish(u), dswish(u), (z - p5["mean"]) * p5["invstd"]
    pool = lambda t: t.double().view(B, rpi, K).sum(1)
    v, A = chan_pool_bwd(z, p5["scale"], p5["shift"], p5["mean"], p5["invstd"], dx, out0, B, rpi)
    if dx.dtype != torch.float64:
        v = torch.stack([pool(t) for t in (dx * a, dx * sp, dx * sp * xh, sp, sp * xh)]) + out0.double()
    A = A.double().clone()
    A[:3] = torch.stack([pool(A_dx * a.abs()), pool(A_dx * sp.abs()), pool(A_dx * (sp * xh).abs())]) + out0.double().abs()[:3]
    return v.double(), A


def bd_fwd(g, z, wt, bn, residual=None, xs=None, p5=None, bf16=False, dot=None, kernel_order=False):
    """the _bn / _bn2 entry points (see the module docstring).  bn: the dict of wg_ref.bn_operand (z, scale, shift, mean, invstd, sums float64 [2N],
    count, act, mul_b or None, rpi) with "dgamma0" / "dbeta0" (or None); xs: z, mean, invstd, mul_b (or None), rpi, sums0 float64 [2K]; p5: z,
    scale, shift, mean, invstd, out0 [5, B, K], B.  dot: the product (default dz @ wt^T); bf16: dz and wt rounded to bf16, exact products"""
    dt = g.dtype
    dz, Az = bn_operand(g, bn, kernel_order)
    if bf16:
        dx = (dz.bfloat16().double() @ wt.bfloat16().double().t()).to(dt)
    else:
        dx = dz @ wt.t() if dot is None else dot(dz, wt)
    A = Az @ wt.abs().t()
    if residual is not None:
        dx, A = dx + residual, A + residual.abs()
    out = {"dz": (dz, Az), "dx_bf16" if bf16 else "dx": (dx, A)}
    if bn.get("dgamma0") is not None:
        N, sums = z.shape[1], bn["sums"]
        out["dgamma"] = (bn["dgamma0"] + sums[N:].to(dt), bn["dgamma0"].abs() + sums[N:].abs().to(dt))
        out["dbeta"] = (bn["dbeta0"] + sums[:N].to(dt), bn["dbeta0"].abs() + sums[:N].abs().to(dt))
    if xs is not None:
        out.update(xs_ref(dx, A, xs, bf16))
    if p5 is not None:
        out["p5_bf16" if bf16 else "p5"] = p5_ref(dx, A, p5)
    return out


def family_of(out):
    """the K family an output of bd_fwd is judged in"""
    return "dsum" if out in ("dgamma", "dbeta") else out


# ------------------------------------------------------------------------------------------------ the dispatch, copied
def slab_plan(M, Kg, Ng, pro=1):
    """A COPY of slab_plan (pw_slab.hip:439-466) without MMD_SLAB_BLOCKS; None: the slab kernel does not cover the shape.  The GPU test compares
    part_floats with mmd_pwconv_slab_ws_floats(M, Kg, Ng, 1): the one place where this module's copies meet the host code."""
    if M <= 0 or Kg & 3 or Ng & 3 or Kg < 128 or Ng < 36:                             # :440
        return None
    tiles = cdiv(Ng, 32)
    nchunk = cdiv(tiles, 7)                                                           # :442
    nt32 = cdiv(tiles, nchunk)
    if nt32 < 2:                                                                      # :444
        return None
    nslab = cdiv(M, 32)
    blocks, gtot = nslab * nchunk, cdiv(Kg, 32)
    ns = 1 if blocks >= 256 else 256 // blocks                                        # :450
    ns = max(1, min(min(ns, 8), gtot // 8))                                           # :451
    gran = cdiv(gtot, ns)
    nslice = cdiv(gtot, gran)
    nco, ktab, nw = (5 if pro == 1 else 2), gran * 32, nt32 * 32
    nc4 = nw // 4
    lg = 4 if nc4 <= 16 else (5 if nc4 <= 32 else 6)                                  # :457
    stage_f, red_f = 4 * (32 + nw) * 36, nt32 * 3 * 1024 + 32 * nw + 2 * (256 >> lg) * nw      # :460
    lds = (nco * ktab + max(stage_f, red_f)) * 4
    if lds > 158 * 1024:                                                              # :462
        return None
    if pro == 1 and cdiv(gran * 32, 256) > nslab:                                     # :463
        return None
    return {"nt32": nt32, "nchunk": nchunk, "nslab": nslab, "nslice": nslice, "gran": gran, "ktab": ktab, "lg": lg, "lds": lds,
            "part_floats": nslice * nslab * 32 * nchunk * nw if nslice > 1 else 0, "row_tail": M % 32, "col_tail": Ng % 32}


def slab_refusal(M, Kg, Ng):
    """True where slab_plan refuses a BatchNorm-operand launch by its last rule alone (:463): a plan exists for the plain operand"""
    return slab_plan(M, Kg, Ng, 1) is None and slab_plan(M, Kg, Ng, 0) is not None


def route(form, native, bf16, M, Kg, Ng, dz_out=True, xs=False, ws_slots=0, p5_B=0, slab_ws=False, split_default=True):
    """Which kernel instantiation a BatchNorm-operand launch (bb.z set) reaches: a COPY of the host decisions of pw_bwd_data_bn2_impl
    (pw_gemm.hip:1545-1588), pw_dispatch (:1149-1262), pw_bq_lds (:513-527) and pw_slab_try (pw_slab.hip:478-518), with no MMD_* variable set
    (split_default False: MMD_MFMA_F32).  slab_ws: the caller passes a workspace of slab_plan's part_floats.  -> dict; {"rc": -22}: refused.
    pw_rows_try (pw_rows.hip:305) and pw_longk_try (pw_longk.hip:218) refuse every launch with bb.z or xs.z."""
    slotted = bool(xs and ws_slots > 1 and cdiv(M, 64) > STATS_DEPTH)                 # pw_gemm.hip:1574
    p5 = None
    if p5_B:
        p5 = "epilogue" if (M // p5_B) % PW_BM == 0 else "standalone"                 # :1579, :1584-1585
    big = cdiv(M, PW_BM) * cdiv(Ng, 64)                                               # :1154 big_tiles
    take_skinny = big < 160 and Ng > 16                                               # :1170 (MMD_SKINNY_K 0, MMD_SKINNY_TILES 160, MMD_SQ_MIN 160)
    variant = 0 if take_skinny else (1 if Ng <= 32 else 2)                            # :1174-1176 with bb.z: never 128x64, no padding rule
    common = {"pro": 1, "slotted": slotted, "p5": p5, "big_tiles": big, "half_group": Kg % 8 == 4}
    slab_auto = take_skinny and p5 != "epilogue" and Ng > 64 and Kg >= 256            # :1197 (bb.z)
    if form in (0, 4) and (form == 4 or slab_auto) and not bf16 and p5 != "epilogue" and not slotted:      # pw_slab.hip:481-483
        p = slab_plan(M, Kg, Ng, 1)                                                   # :490
        if p is not None and p["nslice"] > 1 and not slab_ws:                         # :491-494
            if form == 4:
                return {"rc": -22}
            p = None
        if p is not None:
            dzk = 1 if (dz_out and M % 32 == 0) else 2                                # :498
            return {**common, **p, "family": "slab", "mfma": "f32", "table": True, "dzk": dzk, "comb": (p["nslice"], p["lg"]) if p["nslice"] > 1 else None}
    if variant == 0:                                                                  # pw_gemm.hip:1212-1229; :1227 no table on the skinny kernel
        return {**common, "family": "skinny", "variant": 0, "bm": 32, "bn": 64, "nkl": None, "mfma": "bf16" if bf16 else "f32", "table": False,
                "ntn": cdiv(Ng, 64), "ntm": cdiv(M, 32), "row_tail": M % 32, "col_tail": Ng % 64, "short_k": Kg < 128, "k_tail": Kg % 128}
    nkl = ((Kg - 1) % 32) // 8 + 1                                                    # :1231
    mfma = "bf16" if bf16 else ("split" if (split_default and not native and Kg >= 64 and Ng > 48) else "f32")      # :1232-1233
    bm, bn = ((128, 32), (64, 64))[variant - 1]                                       # :1246, :1254
    table = 20 * Kg + (37 if mfma == "split" else 28) * 1024 <= 48 * 1024             # :1260, :517-520
    return {**common, "family": "tiled", "variant": variant, "bm": bm, "bn": bn, "nkl": nkl, "mfma": mfma, "table": table, "ntn": cdiv(Ng, bn),
            "ntm": cdiv(M, bm), "row_tail": M % bm, "col_tail": Ng % bn}


# ------------------------------------------------------------------------------------------------ cases
# form label -> (entry point, form or None, bf16, a slab workspace is passed)
FORMS = {"bn": ("mmd_pwconv_bwd_data_bn", None, 0, 0), "bn_bf16": ("mmd_pwconv_bwd_data_bn_bf16", None, 1, 0),
         "bn2": ("mmd_pwconv_bwd_data_bn2", None, 0, 0), "bf16": ("mmd_pwconv_bwd_data_bn2_bf16", None, 1, 0),
         "f0": ("mmd_pwconv_bwd_data_bn2_form", 0, 0, 0), "f0w": ("mmd_pwconv_bwd_data_bn2_form", 0, 0, 1),
         "f2": ("mmd_pwconv_bwd_data_bn2_form", 2, 0, 0), "f2n": ("mmd_pwconv_bwd_data_bn2_form", 2 | MMD_PW_FORM_NATIVE, 0, 0),
         "f4": ("mmd_pwconv_bwd_data_bn2_form", 4, 0, 0), "f4w": ("mmd_pwconv_bwd_data_bn2_form", 4, 0, 1)}
# mode: blank-separated tokens.  act: swish; mulb: mul_b with rows_per_image 7 and a dropped sample; nodz / nodsum: dz_out / dgamma + dbeta null;
# res / alias: a residual in its own tensor / aliasing dx; xs / xsm: upstream sums without / with xs_mul_b; ws: stats_ws with 64 slots (the
# launch is repeated with ws_slots = 0); p5: the five-plane pool with p5_B = the case's B
TOKENS = {"act", "mulb", "nodz", "nodsum", "res", "alias", "xs", "xsm", "ws", "p5"}
S0, SA, SB = "", "act mulb", "nodz nodsum"
SX, SR, SP = "act mulb alias xsm", "res xs nodsum", "act p5"
SW = ["xsm ws", "act alias xs ws"]
B3 = ["f2", "f2n", "bf16"]
ALL = B3 + ["bn", "bn_bf16", "bn2"]


def _nkl(Kg):
    return ((Kg - 1) % 32) // 8 + 1


def _c(name, M, Kg, Ng, forms, fam, modes, why, B=1, fam_by_form=None):
    assert M % B == 0 and all(set(m.split()) <= TOKENS for m in modes)
    return {"name": name, "M": M, "Kg": Kg, "Ng": Ng, "K": Ng, "N": Kg, "B": B, "forms": forms, "fam": fam, "fam_by_form": fam_by_form or {},
            "modes": modes, "why": why}


BD_CASES = [
    # ---- 128x32 <PRO 1> on one block: every Kg % 32 (nkl 1..4, each with and without the half 8-wide group); Ng <= 16 is never skinny
    *[_c("t1_k%d" % Kg, 100, Kg, 16, ALL if Kg == 12 else B3, "tiled", [SA] + ([S0, SX, SB] if Kg in (12, 32) else []),
         "pw_gemm<128,32,nkl %d,PRO 1>, Kg %% 32 = %d, one block with 100 of 128 rows, images of 7 rows" % (_nkl(Kg), Kg % 32))
      for Kg in (4, 8, 12, 16, 20, 24, 28, 32, 36)],
    _c("t1_m1", 1, 8, 16, B3, "tiled", [S0, SR], "pw_gemm<128,32,PRO 1>: M = 1"),
    _c("t1_m33", 33, 20, 12, B3, "tiled", [SA, SX], "pw_gemm<128,32,PRO 1>: M = 33, Ng = 12 below the tile width"),
    _c("t1_n4", 100, 12, 4, B3, "tiled", [S0, SR], "pw_gemm<128,32,PRO 1>: Ng = 4, one column quad"),
    _c("t1_rows3", 260, 40, 16, B3, "tiled", [SX, SB, SR], "pw_gemm<128,32,PRO 1>: three row blocks - dgamma / dbeta added by one of them"),
    _c("t1_p5", 256, 24, 16, B3, "tiled", [SP, "p5 mulb nodz"], "128x32: the pool in the epilogue, two images of 128 rows: one per row tile", B=2),
    _c("t1_p5r", 100, 24, 16, B3, "tiled", [SP], "128x32: images of 25 rows, the pool as its own launch", B=4),
    _c("t1_n32", 20400, 40, 32, B3, "tiled", [SA], "16 < Ng <= 32 at big_tiles 160: the first 128x32 shape of that width, row tail 48"),
    _c("sk_n32", 20352, 40, 32, B3, "skinny", [SA], "16 < Ng <= 32 at big_tiles 159: the last skinny shape of that width"),
    _c("t1_tab1024", 100, 1024, 16, B3, "tiled", [SA], "the coefficient table in LDS: 20 * 1024 + 28 KB = 48 KB, the last Kg with it"),
    _c("t1_tab1028", 100, 1028, 16, B3, "tiled", [SA], "Kg = 1028: the table does not fit, coefficients from the batch sums per K step"),
    # ---- skinny <PRO 1, PF 1>: Kg % 32, Kg shorter than the four-wave K split, tails
    *[_c("sk_k%d" % Kg, 300, Kg, 40, ALL if Kg == 24 else B3, "skinny", [SA] + ([S0, SX, SB] if Kg in (24, 160) else []),
         "pw_gemm_skinny<PRO 1>: Kg = %d (Kg %% 32 = %d%s), 10 row blocks, row tail 12, col tail 40 of 64"
         % (Kg, Kg % 32, ", shorter than the four-wave K split" if Kg < 128 else ""))
      for Kg in (4, 8, 12, 16, 20, 24, 28, 32, 132, 160, 260)],
    _c("sk_m1", 1, 24, 40, B3, "skinny", [S0, SR], "pw_gemm_skinny<PRO 1>: M = 1"),
    _c("sk_m33", 33, 24, 68, B3, "skinny", [SA, SX, SB], "pw_gemm_skinny<PRO 1>: M = 33 (row tail 1), Ng = 68: two column tiles, Ng % 64 = 4"),
    _c("sk_p5", 256, 24, 40, B3, "skinny", [SP, "p5 mulb nodz"], "skinny: the pool in the epilogue, four 32-row tiles per image", B=2),
    _c("sk_p5r", 300, 24, 40, B3, "skinny", [SP], "skinny: images of 75 rows, the pool as its own launch", B=4),
    _c("sk_slot", 8200, 24, 40, B3, "skinny", SW, "skinny with cdiv(M, 64) = 129 > 128 and a slot workspace: it must stay zero"),
    # ---- 64x64 <PRO 1> (big_tiles >= 160, Ng > 32)
    *[_c("t2_k%d" % Kg, 20400, Kg, 52, B3, "tiled", [SA] + ([S0, SX, SB] if Kg in (72, 96) else []),
         "pw_gemm<64,64,nkl %d,PRO 1> split / native / bf16, Kg %% 32 = %d, Ng = 52, row tail 48" % (_nkl(Kg), Kg % 32))
      for Kg in (68, 72, 76, 80, 84, 88, 92, 96)],
    *[_c("t2_n68_k%d" % Kg, 10200, Kg, 68, B3, "tiled", [SX, SR], "pw_gemm<64,64,nkl %d,PRO 1> split / native / bf16: two column tiles, Ng %% 64 = 4 - "
         "dz stored by the first column tile, dgamma / dbeta added once" % _nkl(Kg)) for Kg in (68, 76, 88, 96)],
    _c("t2_k60_n52", 20400, 60, 52, B3, "tiled", [SA], "below the split-form switch: Kg = 60"),
    _c("t2_k64_n48", 20400, 64, 48, B3, "tiled", [SA], "below the split-form switch: Ng = 48"),
    _c("t2_k64_n52", 20400, 64, 52, B3, "tiled", [SA, S0], "above the split-form switch: Kg = 64, Ng = 52, nkl 4"),
    # (40 images: a seam between two images every eighth 64-row tile, and eight fp32 atomic adds per pool element - the model of K sums in
    #  float64, and the chain of one add per row tile that the kernels have instead grows with the rows of an image)
    _c("t2_p5", 20480, 24, 52, B3, "tiled", [SP], "64x64: the pool in the epilogue, 40 images of 512 rows = eight row tiles", B=40),
    _c("t2_p5r", 20400, 24, 52, B3, "tiled", [SP], "64x64: 40 images of 510 rows, the pool as its own launch", B=40),
    _c("t2_slot", 20400, 24, 52, B3, "tiled", SW, "64x64 with slotted upstream sums (ws_slots 64) and direct (0)"),
    _c("t2_tab560", 20400, 560, 52, B3, "tiled", [SA], "split form: 20 * 560 + 37 KB = 48 KB - 64, the last Kg with the table"),
    _c("t2_tab564", 20400, 564, 52, B3, "tiled", [SA], "split form: Kg = 564, no table (v_mfma_f32 and bf16 keep it up to 1024)"),
    # ---- slab kernel <NT32, 1, DZK>, unsliced (Kg = 256: one slice of 8 granules)
    *[_c("sl_nt%d" % nt, 64, 256, Ng, ["f4", "f2"] + (["bn2"] if Ng > 64 else []), "slab", [SA if nt % 2 else S0] + ([SX, SB] if nt in (3, 6) else []),
         "pw_slab_kernel<%d,1,DZK>: Ng = %d, two whole slabs (DZK 1; 2 where dz_out is null)" % (nt, Ng), fam_by_form={"f2": "skinny"})
      for nt, Ng in ((2, 64), (3, 68), (4, 100), (5, 132), (6, 164), (7, 196))],
    _c("sl_ragged", 40, 256, 100, ["f4", "bn2"], "slab", [SA, SX], "pw_slab_kernel<4,1,2>: M = 40, a last slab of 8 rows: M % 32 != 0 is DZK 2"),
    _c("sl_chunks", 64, 256, 260, ["f4", "bn2"], "slab", [SX, SB], "pw_slab_kernel<5,1,*>: Ng = 260 > 224, two column chunks of five tiles"),
    _c("sl_p5r", 64, 256, 100, ["bn2", "f4"], "slab", [SP], "the slab kernel with the pool as its own launch (images of 32 rows)", B=2),
    _c("sl_p5", 256, 256, 100, ["bn2", "f4"], "skinny", [SP], "a pool in the epilogue: the slab kernel refuses, also forced", B=2),
    # ---- slab kernel, sliced: combine kernel <nslice, lg>
    _c("sl_s2_lg4", 32, 512, 64, ["f4w"], "slab", [SX, SB], "two slices, combine<2,4> (Ng = 64)"),
    _c("sl_s3_lg5", 32, 768, 100, ["f4w", "f0w"], "slab", [SX, SB], "three slices, combine<3,5> (Ng = 100)"),
    _c("sl_s5_lg5", 40, 1280, 68, ["f4w", "f0w"], "slab", [SX, SA], "five slices on a ragged slab, combine<5,5> (Ng = 68)"),
    _c("sl_s8_lg6", 32, 2048, 164, ["f4w", "f0w"], "slab", [SX, SB], "eight slices, combine<8,6> (Ng = 164)"),
    _c("sl_refused", 32, 288, 68, ["f4", "bn2"], "skinny", [SA, SX], "one slab, a slice of 9 granules: cdiv(288, 256) = 2 > nslab = 1, slab_plan refuses"),
    _c("sl_auto", 64, 512, 68, ["f0w", "f0"], "slab", [SA, SX], "auto form on a sliced shape: the slab kernel with a workspace, the LDS kernels without",
       fam_by_form={"f0": "skinny"}),
]
CASE = {c["name"]: c for c in BD_CASES}
assert len(CASE) == len(BD_CASES)

# plain mmd_pwconv_bwd_data / _bf16 (pw_fwd with the sizes swapped, the output aliasing the residual where accumulate = 1): one case of
# pw_ref.PW_CASES per kernel family, its K the launch's Kg and its N the launch's Ng
PLAIN_CASES = [("t1_acc", "tiled"), ("sk_nonlean", "skinny"), ("t2_k72", "tiled"), ("t3_k72", "tiled"), ("lk_k720", "longk")]
PLAIN_BF16_FAMILY = {"lk_k720": "skinny"}          # pw_longk_try refuses bf16


def flags(mode):
    t = set(mode.split())
    return {"act": int("act" in t), "mulb": "mulb" in t, "dz": "nodz" not in t, "dsum": "nodsum" not in t,
            "res": "alias" if "alias" in t else ("res" if "res" in t else None), "xs": "xsm" if "xsm" in t else ("xs" if "xs" in t else None),
            "ws": 64 if "ws" in t else 0, "p5": "p5" in t}


def bn_only(mode):
    """a mode the mmd_pwconv_bwd_data_bn entry points can express"""
    f = flags(mode)
    return not (f["res"] or f["xs"] or f["p5"])


def runs(case):
    """(mode, form label) of every launch of a case: the _bn entry points take the modes they can express"""
    return [(m, f) for m in case["modes"] for f in case["forms"] if bn_only(m) or not f.startswith("bn") or f == "bn2"]


def expected_family(case, form):
    return case["fam_by_form"].get(form, case["fam"])


def route_mode(case, mode, form, ws_slots=None, split_default=True):
    _, fm, bf16, sws = FORMS[form]
    f = flags(mode)
    fm = 0 if fm is None else fm
    return route(fm & ~MMD_PW_FORM_NATIVE, bool(fm & MMD_PW_FORM_NATIVE), bf16, case["M"], case["Kg"], case["Ng"], dz_out=f["dz"], xs=bool(f["xs"]),
                 ws_slots=f["ws"] if ws_slots is None else ws_slots, p5_B=case["B"] if f["p5"] else 0, slab_ws=bool(sws), split_default=split_default)


# ------------------------------------------------------------------------------------------------ inputs
def case_inputs(case):
    """fp32 CPU tensors of one case (every mode takes what it needs from them); the same for the CPU calibration and the GPU test"""
    M, K, N, B = case["M"], case["K"], case["N"], case["B"]
    g = rng(37, M, K, N, B)
    z, _, _, _, coef = bn_inputs(g, M, N)
    mul_b = rand(g, cdiv(M, BN_RPI)) + 0.2
    if mul_b.numel() > 1:
        mul_b[1] = 0.0                                    # a dropped sample (drop-connect)
    return {"g": randn(g, M, N), "z": z, "wt": randn(g, K, N) / math.sqrt(N), "scale": coef["scale"], "shift": coef["shift"], "mean": coef["mean"],
            "invstd": coef["invstd"], "mul_b": mul_b, "dgamma0": randn(g, N), "dbeta0": randn(g, N), "res": randn(g, M, K),
            "xs_z": randn(g, M, K) * 0.8 + 0.1, "xs_mean": randn(g, K) * 0.2, "xs_invstd": rand(g, K) + 0.5, "xs_mul_b": rand(g, cdiv(M, XS_RPI)) + 0.5,
            "xs0": randn(g, 2 * K).double() * 3, "p5_z": randn(g, M, K) * 1.1, "p5_scale": rand(g, K) + 0.5, "p5_shift": randn(g, K) * 0.1,
            "p5_mean": randn(g, K) * 0.2, "p5_invstd": rand(g, K) + 0.5, "p5_0": randn(g, 5, B, K)}


def to(d, dt, dev="cpu"):
    return {k: (t.to(dev) if t.dtype != torch.float32 else t.to(dev, dt)) if isinstance(t, torch.Tensor) else t for k, t in d.items()}


def case_sums(case, mode, d64):
    """the float64 sums [2N] = [sum g', sum g' * xhat] a reduce pass hands the launch: elt_ref.bn_bwd_reduce on the float64 inputs"""
    f = flags(mode)
    z = d64["z"]
    zero = torch.zeros(2 * z.shape[1], dtype=torch.float64, device=z.device)
    return bn_bwd_reduce(d64["g"], z, d64["scale"], d64["shift"], d64["mean"], d64["invstd"], f["act"], None, d64["mul_b"] if f["mulb"] else None, None,
                         BN_RPI, zero)[2]


def case_ref(case, mode, d, sums, **model):
    """reference of one (case, mode) from the input dict d (any dtype / device) and the float64 sums -> dict of (value, A)"""
    f = flags(mode)
    bn = {"z": d["z"], "scale": d["scale"], "shift": d["shift"], "mean": d["mean"], "invstd": d["invstd"], "sums": sums, "count": case["M"],
          "act": f["act"], "mul_b": d["mul_b"] if f["mulb"] else None, "rpi": BN_RPI, "dgamma0": d["dgamma0"] if f["dsum"] else None,
          "dbeta0": d["dbeta0"] if f["dsum"] else None}
    xs = p5 = None
    if f["xs"]:
        xs = {"z": d["xs_z"], "mean": d["xs_mean"], "invstd": d["xs_invstd"], "mul_b": d["xs_mul_b"] if f["xs"] == "xsm" else None, "rpi": XS_RPI,
              "sums0": d["xs0"]}
    if f["p5"]:
        p5 = {"z": d["p5_z"], "scale": d["p5_scale"], "shift": d["p5_shift"], "mean": d["p5_mean"], "invstd": d["p5_invstd"], "out0": d["p5_0"],
              "B": case["B"]}
    return bd_fwd(d["g"], d["z"], d["wt"], bn, residual=d["res"] if f["res"] else None, xs=xs, p5=p5, **model)


def plain_ref(name, acc, dt, dev="cpu", **model):
    """mmd_pwconv_bwd_data(dy, wt, dx, M, K, N, accumulate) = pw_fwd(x = dy [M, N], w = wt [K, N], residual = dx where it accumulates) on the
    inputs of pw_ref's case `name` -> (inputs in dt, (dx, A))"""
    pc = pw_ref.CASE[name]
    d = pw_ref._to(pw_ref.case_inputs(pc), dt, dev)
    return d, pw_fwd(d["x"], d["w"], residual=d["res"] if acc else None, **model)["y"]
