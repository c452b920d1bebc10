"""Helper (not a test): float64 restatement of the 1x1-conv WEIGHT GRADIENT - the grouped launch of csrc/pw_wgrad_grouped.hip
(mmd_wgrad_plan, mmd_wgrad_grouped, mmd_wgrad_grouped_bf16, mmd_wgrad_grouped_form in its default rectangular form: wgrad_grouped_rect_kernel
<BF, R32>, wgrad_grouped_split_kernel<4>, wgrad_fold_rect_kernel) and the per-layer pw_wgrad_kernel behind mmd_pwconv_bwd_weight, _bf16, _bn and
_bn_bf16 (pw_gemm.hip) - written from the contracts in include/mmdistill.h and the header comments of pw_args.h, not from the kernels' loops;
copies of the two host planners (plan: mmd_wgrad_plan; per_layer_plan: pw_wgrad_impl) with what each case exists for (describe); and the
tables (WG_TABLES, PER_LAYER_CASES) that test_wg_ref_cpu.py and test_gpu_wg_float64.py share.

OUT OF SCOPE here: the square tile forms (wgrad_grouped_kernel<64 / 128>, wgrad_fold_kernel<T>: MMD_WG_TILE), the MMD_WG_SPLIT_W3 / MMD_WG_XCD8 /
MMD_WG_BLOCKS knobs, the w16 storage flags, the stem weight gradient (mb_ref.py has it).

Conventions are those of elt_ref.py / pw_ref.py.  wg_fwd computes in the dtype (and on the device) of its tensor arguments: float64 is the
oracle, float32 the model that calibrates K.  It returns {"dw"} (with `bn` also {"dgamma", "dbeta"}) of (value, A):
  * X operand a = gate[row // rpi] * act(x*scale + shift): pw_ref.pw_operand, the forward's
  * dY operand d = dy, A_d = |dy|; with `bn` the evaluated BatchNorm backward of pw_args.h, dz = scale*(g' - m1 - xhat*m2),
    g' = g * mul_b[image] * act'(z*scale + shift), m = sums / count from the float64 sums the kernel is handed: elt_ref.bn_bwd_g and
    elt_ref.bn_bwd_apply with k = scale (the kernel's a1)
  * dw = dw0 + d^T @ a, A = |dw0| + A_d^T @ A_a (the grouped launch WRITES dW: dw0 None; the per-layer launches accumulate)
  * dgamma = d0 + sums[C:], dbeta = d0 + sums[:C], A = |d0| + |sums|
Errors are judged per element, none left out: |got - ref64| <= K * unit * A + tiny, unit 2^-24 (2^-9 for the bf16 forms), K = max(8, ceil(4 * K32))
per output family, K32 the largest error in that unit of the CPU model over every case of the tables (test_wg_ref_cpu.py measures it and
asserts that the K32 stored below is the one it gives to within 5 % + 0.01 - the last digits are one ulp of the host's fp32 sigmoid - that
no model exceeds K / 4, and that K is the ceiling of four times the stored K32; below K32 = 2 the floor K = 8 decides and the stored
value is not compared):
  * fp32 model: prologue and BatchNorm-backward evaluation in fp32, the latter in the kernel's operation order a1*g' + a2*(z - mu) + a3
    (a2 = -a1*invstd*m2, a3 = -a1*m1); the reduction a strictly sequential fp32 chain over the rows m (multiply, round, add, round) - the order
    with the most accumulator roundings of any kernel here (v_mfma_f32 chain per split: mchunk; three-way bf16 split: 6 mchunk / 16; then one
    add per split in the fold, or one atomic per split); dw0 added last
  * bf16 model: both post-prologue operands rounded to bf16, exact products (pw_ref's), fp32 prologue, against float64 of the UNROUNDED operands.
No constant comes from a GPU run of the kernels."""
import torch

from elt_ref import bn_bwd_g, bn_bwd_apply, bn_inputs, rng, randn, rand, cdiv, U, TINY, SENTINEL      # noqa: F401
from pw_ref import pw_operand, seq_dot, UB

# K per family = max(8, ceil(4 * K32)).  K32 as test_wg_ref_cpu.py measures it (CPU models of the docstring on every case of the tables):
K32 = {"dw": 9.327, "dw_bn": 5.487, "dw_bf16": 3.296, "dw_bn_bf16": 1.998, "dsum": 1.761}
K_BY_FAMILY = {"dw": 38.0, "dw_bn": 22.0, "dw_bf16": 14.0, "dw_bn_bf16": 8.0, "dsum": 8.0}
UNIT = {f: (UB if f.endswith("_bf16") else U) for f in K_BY_FAMILY}

GW_BR, GW_MAXL, GW_MAXL3 = 32, 512, 255       # pw_wgrad_grouped.hip: rows per step, the planner's layer limit, the split kernel's
PLAN_FIELDS = ("pad_", "ntn", "ntk", "mchunk", "nsplit", "item0", "tile0", "ws_off")
PLAN_ENV = ("MMD_WG_TILE", "MMD_WG_RECT_MIN", "MMD_WG_RECT_ROWS")      # set: the planner is not in its default form, `plan` does not describe it


# ------------------------------------------------------------------------------------------------ reference
def seq_rows(d, a):
    """d^T @ a as a strictly sequential chain over the rows m in the dtype of d: pw_ref.seq_dot with the rows as its reduction index"""
    return seq_dot(d.t().contiguous(), a.t().contiguous())


def bn_operand(g_in, bn, kernel_order=False):
    """the dY operand of the _bn entry points: (dz, A).  bn: z, scale, shift, mean, invstd [C], sums float64 [2C], count, act, mul_b (or None),
    rpi.  kernel_order: the value as bn_bwd_coef / bn_bwd_eval (pw_args.h) form it, a1*g' + a2*(z - mu) + a3 (the fp32 model)"""
    z, scale, sums = bn["z"], bn["scale"], bn["sums"]
    g, Ag = bn_bwd_g(g_in, z, scale, bn["shift"], bn["act"], None, bn.get("mul_b"), None, bn["rpi"])
    dz, A = bn_bwd_apply(g, Ag, z, bn["mean"], bn["invstd"], None, sums, bn["count"], k=scale)["dz"]
    if kernel_order:
        C, inv = z.shape[1], 1.0 / float(bn["count"])
        m1, m2 = (sums[:C] * inv).to(z.dtype), (sums[C:] * inv).to(z.dtype)
        a2, a3 = -scale * bn["invstd"] * m2, -scale * m1
        dz = scale * g + a2 * (z - bn["mean"]) + a3
    return dz, A


def wg_fwd(dy, x, in_scale=None, in_shift=None, in_act=0, gate=None, rpi=0, bn=None, dw0=None, bf16=False, dot=None, kernel_order=False):
    """dw [N, K] = dw0 + d^T @ a (see the module docstring).  dot: the product (default d^T @ a); bf16: both operands rounded to bf16, exact
    products; bn: the dict of bn_operand, with "dgamma0" / "dbeta0" (or None) -> also "dgamma" / "dbeta"."""
    dt = x.dtype
    a, Aa = pw_operand(x, in_scale, in_shift, None, in_act, gate, rpi)
    d, Ad = (dy, dy.abs()) if bn is None else bn_operand(dy, bn, kernel_order)
    if bf16:
        dw = (d.bfloat16().double().t() @ a.bfloat16().double()).to(dt)
    else:
        dw = d.t() @ a if dot is None else dot(d, a)
    A = Ad.t() @ Aa
    if dw0 is not None:
        dw, A = dw0 + dw, dw0.abs() + A
    out = {"dw": (dw, A)}
    if bn is not None and bn.get("dgamma0") is not None:
        C, sums = d.shape[1], bn["sums"]
        out["dgamma"] = (bn["dgamma0"] + sums[C:].to(dt), bn["dgamma0"].abs() + sums[C:].abs().to(dt))
        out["dbeta"] = (bn["dbeta0"] + sums[:C].to(dt), bn["dbeta0"].abs() + sums[:C].abs().to(dt))
    return out


# ------------------------------------------------------------------------------------------------ the planners, copied
def plan(layers, rows_per_item):
    """A COPY of mmd_wgrad_plan (pw_wgrad_grouped.hip) in its default rectangular form (none of PLAN_ENV set): TN x 64 output tiles, TN = 128
    for N > 64 with half the rows per item.  layers: (M, K, N, flags, B).  -> (per-layer dicts, n_items, n_tiles, ws_floats).  The GPU test reads
    the table the C planner fills and compares every field with this copy."""
    rows_per_item = max(rows_per_item, GW_BR)
    out, items, tiles, ws = [], 0, 0, 0
    for M, K, N, flags, B in layers:
        TN = 128 if N >= 65 else 64
        ntn, ntk = cdiv(N, TN), cdiv(K, 64)
        rows = max(rows_per_item // 2, GW_BR) if TN == 128 else rows_per_item
        mchunk = cdiv(cdiv(M, cdiv(M, rows)), GW_BR) * GW_BR
        nsplit = cdiv(M, mchunk)
        out.append({"M": M, "K": K, "N": N, "gate": "gate" in flags, "rpi": cdiv(M, B), "pad_": TN, "ntn": ntn, "ntk": ntk, "mchunk": mchunk,
                    "nsplit": nsplit, "item0": items, "tile0": tiles, "ws_off": ws})
        items += nsplit * ntn * ntk
        tiles += ntn * ntk
        ws += nsplit * ntn * ntk * TN * 64
    return out, items, tiles, ws


def describe(lp):
    """what a planned layer exercises: tile width; per output tile the (nu, nv) of its block's four waves (wn, wk) - the live 32x32 sub-tiles
    along N (0..2) and K (0..1) that pick the row-loop instantiation (a wave with nu == 0 or nv == 0 runs the zero-sub-tile one); rows of the
    last split and its tail below a 32-row step; the fold's rounds of 8 and remainder; whether the fold's second 4096-float half runs; for a
    gated layer the image boundaries that fall strictly inside a 32-row step, and the steps behind an item's first in which the carried image
    index of some row advances (carried; carried2: by two images or more)"""
    M, K, N, TN = lp["M"], lp["K"], lp["N"], lp["pad_"]
    wide = TN == 128
    tiles = []
    for tn in range(lp["ntn"]):
        for tk in range(lp["ntk"]):
            waves = []
            for wn in (0, 1):
                for wk in (0, 1):
                    nb = tn * TN + (wn * 64 if wide else wn * 32)
                    nu = int(nb < N) + int(wide and nb + 32 < N)
                    waves.append((nu, int(tk * 64 + wk * 32 < K)))
            tiles.append(tuple(waves))
    inside = carried = carried2 = 0
    if lp["gate"]:
        for s in range(lp["nsplit"]):
            mbeg, mend = s * lp["mchunk"], min(M, (s + 1) * lp["mchunk"])
            for mb in range(mbeg, mend, GW_BR):
                inside += sum(1 for r in range(mb + 1, min(mb + GW_BR, mend)) if r % lp["rpi"] == 0)
                if mb > mbeg:          # the image index is divided out at an item's first step only, then carried from step to step
                    adv = max((mb + r) // lp["rpi"] - (mb - GW_BR + r) // lp["rpi"] for r in range(GW_BR) if mb + r < mend)
                    carried += adv >= 1
                    carried2 += adv >= 2
    return {"wide": wide, "tiles": tiles, "insts": {w for t in tiles for w in t}, "last_rows": M - (lp["nsplit"] - 1) * lp["mchunk"],
            "row_tail": M % GW_BR, "rounds8": lp["nsplit"] // 8, "rem8": lp["nsplit"] % 8, "second_half": wide, "inside_step": inside, "carried": carried, "carried2": carried2,
            "mixed_0_2": any(any(nu == 2 and nv for nu, nv in t) and any(nu == 0 or nv == 0 for nu, nv in t) for t in tiles)}


def per_layer_plan(M, K, N):
    """A COPY of the splits / mchunk / grid arithmetic of pw_wgrad_impl (pw_gemm.hip) without MMD_WG_BLOCKS: 64 x 64 tiles, at most 1024
    blocks, splits of at least 64 rows (M <= 8192) or 256 rows"""
    ntn, ntk = cdiv(N, 64), cdiv(K, 64)
    tiles = ntn * ntk
    splits = min(max(1024 // tiles, 1), cdiv(M, 64 if M <= 8192 else 256))
    mchunk = cdiv(cdiv(M, splits), 32) * 32
    splits = cdiv(M, mchunk)
    nblk = tiles * splits
    idle = {(wn, wk) for tn in range(ntn) for tk in range(ntk) for wn in (0, 1) for wk in (0, 1)
            if tn * 64 + wn * 32 >= N or tk * 64 + wk * 32 >= K}
    return {"ntn": ntn, "ntk": ntk, "mchunk": mchunk, "splits": splits, "nblk": nblk, "grid": cdiv(nblk, 8) * 8, "idle_waves": idle,
            "row_tail": M % 32}


# ------------------------------------------------------------------------------------------------ tables
# layer = (M, K, N, flags, B): flags of "aff" (in_scale / in_shift + swish), "gate" (B images of cdiv(M, B) rows, the last one ragged where B
# does not divide M), "wide" (both operands spread over eight decades)
GRIDS = (1, 7, 64, 100, 0)          # persistent blocks: one block walking every layer; a partial XCD group; one whole group of 64; one whole group
#                                     and a trailing partial one; the default (1024, clamped to n_items)
_TAILS = [
    (1, 4, 4, "", 1),               # smallest layer, nsplit 1
    (33, 68, 36, "", 1),            # row tail 1; K tail 4 in a second K tile; 64-wide tile whose second sub-tile has 4 live columns
    (100, 60, 64, "", 1),           # N = 64, the last thin width
    (100, 64, 68, "", 1),           # first wide width: a wave with two live sub-tiles beside a wave with one
    (95, 132, 132, "", 1),          # last N tile of 4 columns: zero-sub-tile waves share a block with working ones; third K tile of 4 columns
    (200, 32, 100, "", 1),          # K = 32: the wk = 1 waves idle beside two-sub-tile waves
    (608, 24, 48, "gate", 4),       # thin tile, nsplit 19: two fold rounds of 8 plus 3; images of 152 rows: boundaries inside steps
    (608, 24, 144, "gate", 87),     # wide tile, nsplit 19; images of 7 rows, shorter than a step, the last one ragged
    (256, 16, 16, "", 1),           # nsplit 8 exactly
    (50, 40, 24, "aff gate", 2),    # prologue with a gated layer, images of 25 rows
    (96, 72, 80, "wide", 1),        # eight decades
]
_ROWS32 = [
    (32, 4, 4, "", 1), (32, 68, 36, "", 1), (64, 60, 64, "", 1), (64, 64, 68, "", 1), (96, 132, 132, "", 1), (96, 32, 100, "", 1),
    (608, 24, 48, "gate", 4),       # images of 152 rows: boundaries inside steps on the R32 path, thin tile, nsplit 10
    (608, 24, 144, "gate", 4),      # the same on the wide tile, nsplit 19
    (96, 40, 24, "aff gate", 6),    # images of 16 rows
    (256, 64, 68, "", 1),           # wide, nsplit 8 exactly: the fold's second half without a remainder round
    (2048, 112, 112, "", 1), (64, 1248, 208, "", 1),      # kept from test_wgrad_grouped_rows32_forms
    (96, 72, 80, "wide", 1),
]
_STEPS = [                          # 128 rows per item: items of several steps, so that a gate's image index is carried (one-step items divide it out)
    (192, 24, 144, "gate", 28),     # wide tile, two steps per item; images of 7 rows: the carry advances four or five images per step
    (256, 40, 48, "aff gate", 3),   # thin tile, four steps per item; images of 86 rows: boundaries inside carried steps
    (608, 72, 80, "gate", 4),       # wide tile, K tail; images of 152 rows
    (96, 8, 8, "", 1),
]
_MANY = [(64, 8, 8, "", 1) if i % 2 == 0 else (32, 4, 12, "", 1) for i in range(GW_MAXL)]
WG_TABLES = [
    {"name": "tails", "layers": _TAILS, "rows_per_item": 32, "grids": GRIDS, "rows32": (0,), "prefixes": (len(_TAILS),)},
    {"name": "rows32", "layers": _ROWS32, "rows_per_item": 64, "grids": GRIDS, "rows32": (0, 1), "prefixes": (len(_ROWS32),)},
    {"name": "steps", "layers": _STEPS, "rows_per_item": 128, "grids": GRIDS, "rows32": (0, 1), "prefixes": (len(_STEPS),)},
    {"name": "many", "layers": _MANY, "rows_per_item": 32, "grids": GRIDS, "rows32": (0, 1), "prefixes": (GW_MAXL3, GW_MAXL3 + 1, GW_MAXL)},
]
TABLE = {t["name"]: t for t in WG_TABLES}

# per-layer kernel: (M, K, N, B)
PER_LAYER_CASES = [
    (1, 4, 4, 1),                   # smallest; a grid of 1 padded to 8
    (33, 68, 36, 3),                # row tail 1, K tail 4 in a second tile
    (200, 8, 8, 4),                 # four 64-row splits
    (8192, 8, 8, 4),                # the last M with 64-row splits: 128 of them
    (8224, 8, 8, 4),                # the first M with 256-row splits: 33 of them, grid 40
    (130, 112, 180, 2),
    (300, 32, 100, 3),              # K = 32: idle waves
    (100, 68, 132, 2),              # tiles * splits = 12: four padded blocks leave
]
PL_MODES = ("", "aff", "gate", "aff gate")                                                    # prologue flags
BN_MODES = [(act, mul_b, dsum) for act in (0, 1) for mul_b in (False, True) for dsum in (True, False)]      # act, mul_b given, dgamma / dbeta given
BN_RPI = 7                          # bn_rows_per_image of the mul_b cases: divides no 32-row step


def per_layer_modes():
    """-> (prologue modes of the plain entry points, [(prologue, BatchNorm mode)] of the _bn ones), the same for every case of PER_LAYER_CASES:
    all four prologues, and all four crossed with all eight BatchNorm modes"""
    return PL_MODES, [(flags, m) for flags in PL_MODES for m in BN_MODES]


# ------------------------------------------------------------------------------------------------ inputs
def layer_inputs(idx, M, K, N, flags, B):
    """fp32 CPU tensors of layer `idx` of a table (operands as pw_ref.case_inputs draws them; "wide": both over eight decades)"""
    g = rng(29, M, K, N, B, idx)
    x, dy = randn(g, M, K) * 1.3 + 0.2, randn(g, M, N)
    if "wide" in flags:
        x = x * torch.exp2(torch.randint(-13, 14, (M, K), generator=g).float())
        dy = dy * torch.exp2(torch.randint(-13, 14, (M, N), generator=g).float())
    return {"x": x, "dy": dy, "scale": rand(g, K) + 0.5, "shift": randn(g, K) * 0.2, "gate": rand(g, B, K) * 0.9 + 0.05, "dw0": randn(g, N, K)}


def bn_layer_inputs(M, N):
    """the BatchNorm side of a _bn launch: z with the coefficients of its batch statistics, sums as a reduce pass would leave them, count != M"""
    g = rng(31, M, N)
    z, _, _, _, coef = bn_inputs(g, M, N)
    return {"z": z, "scale": coef["scale"], "shift": coef["shift"], "mean": coef["mean"], "invstd": coef["invstd"],
            "sums": randn(g, 2 * N).double() * M ** 0.5, "count": 2 * M + 1, "mul_b": rand(g, cdiv(M, BN_RPI)) + 0.2,
            "dgamma0": randn(g, N), "dbeta0": randn(g, N)}


def to(d, dt, dev="cpu"):
    return {k: (t.to(dev) if t.dtype != torch.float32 else t.to(dev, dt)) if isinstance(t, torch.Tensor) else t for k, t in d.items()}


def layer_ref(layer, d, bn=None, bn_mode=None, flags=None, with_dw0=False, **model):
    """reference of one layer from its input dict d (any dtype / device).  flags: the prologue (default: the layer's own); bn / bn_mode: the
    BatchNorm side and (act, mul_b, dsum) of a _bn launch"""
    M, K, N, lflags, B = layer
    flags = lflags if flags is None else flags
    aff, gate = "aff" in flags, "gate" in flags
    b = None
    if bn is not None:
        act, mul_b, dsum = bn_mode
        b = {**bn, "act": act, "rpi": BN_RPI, "mul_b": bn["mul_b"] if mul_b else None}
        if not dsum:
            b["dgamma0"] = b["dbeta0"] = None
    return wg_fwd(d["dy"], d["x"], d["scale"] if aff else None, d["shift"] if aff else None, 1 if aff else 0, d["gate"] if gate else None,
                  cdiv(M, B), bn=b, dw0=d["dw0"] if with_dw0 else None, **model)
