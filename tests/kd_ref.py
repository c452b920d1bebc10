"""Helper (not a test): float64 restatement of the knowledge-distillation kernels of csrc/loss.hip - mmd_mta_attention, mmd_mta_attention_bwd,
mmd_mta_kl, mmd_mta_kl_multi (pairwise and list mode), mmd_at_loss_multi - written from the formulas in the comments of loss.hip and the
definitions of the reference's MTALoss / AttentionLoss (as oracle/losses_ref.py restates them), not from the kernels' loops; a copy of the
host and kernel dispatch (route); and the one case table (KD_CASES) that test_kd_ref_cpu.py and test_gpu_kd_float64.py share.

Conventions are those of elt_ref.py and node_ref.py.  Every reference computes in the dtype (and on the device) of its tensor arguments:
float64 is the oracle, float32 the "plain fp32" evaluation that calibrates K.  Every reference returns (value, A), A_i the magnitude of what
was summed or multiplied into element i, carried through every product, reduction and normalisation:
  * a[r] = sum_c f^p / C:  A = sum_c |f|^p / C;  df = (df0 +) da p f^(p-1) / C:  A = (|df0| +) |da p f^(p-1) / C|
  * ahat = a / max(||a||_2, 1e-12): a quotient of a value and an all-positive sum, A = |ahat|
  * list mode: q = prod_k ahat_k (A = nt |q|), l1 = max(sum |q|, 1e-12) (A = sum A_q), that = q / l1 (A = A_q / l1 + |that| A_l1 / l1)
  * softmax: d = x - max x (A_d = A_x + |max x|), e = exp(d) with A_e = e (2 + A_d + 2 |d|) (see below), s = sum e (A_s = sum A_e),
    u = e / s with A_u = A_e / s + u A_s / s
  * kl = sum_j [v log v - v u]:  A = sum_j [A_v (|log v| + 1) + 2 |v log v| + A_v u + v A_u];  loss += kl / B:  A = |loss before| + A_kl / B
  * the two dot products of the backward:  <g, u> = -sum v u (A = sum A_v u + v A_u);  w = -v - <g, u> (A_w = A_v + A_<g,u>);
    dahat = u w / T (A = (A_u |w| + u A_w) / T);  <ahat, dahat> (A = sum |ahat| (|dahat| + A_dahat));
    da = (dahat - ahat <ahat, dahat>) / ns * gscale / B,  A = (A_dahat + |ahat| A_<> + |ahat <>|) / ns * gscale / B, summed over the
    teachers of a pairwise launch and on top of |da before| where the kernel accumulates
  * AttentionLoss: d_t = ahat_s - ahat_t (A = |ahat_s| + |ahat_t|), part = sum_j d_t^2 (A = sum 2 |d_t| A_d + d_t^2),
    loss = sum_b part / (B HW); G = sum_t d_t (A_G = sum A_d), <ahat_s, G> (A = sum |ahat_s| (A_G + |G|)),
    da = cg (G - ahat_s <>) / ns (A = cg (A_G + |ahat_s| A_<> + |ahat_s <>|) / ns), or cg G / 1e-12 (A = cg A_G / 1e-12) where ||a_s|| <= 1e-12
Quirks kept: kl_div is fed probabilities (sum v (log v - u) / B); the list-mode teacher is the L1-normalised product (fabs) of the
L2-normalised maps; the clamps are the C float 1e-12f; v log v is taken only where v > 0; AttentionLoss divides by B * HW.

The fast intrinsics.  The KD kernels call __expf and __logf.  The compiler's HIP math header (__clang_hip_math.h) defines
    __expf(x) = __builtin_amdgcn_exp2f(0x1.715476p+0f * x)        __logf(x) = __builtin_logf(x)
  * __expf: the float constant is log2(e) rounded to fp32 (relative error < 2^-24) and the product is rounded once more (2^-24): the
    argument of the hardware exp2 carries a relative error of up to 2 * 2^-24, i.e. x is off by 2 * 2^-24 |x|, and d/dx exp(x) = exp(x)
    turns that into 2 |x| exp(x) units of 2^-24.  v_exp_f32 itself is specified to 1 ulp = 2 units of |exp(x)|.  Together with the rounding
    error the argument d = x - max already has (A_d): A_e = e (2 + A_d + 2 |d|).
  * __logf: __builtin_logf is the full-precision expansion unless the translation unit is built with fast-math flags, and the build
    (mm_distillnet_amd/build.py FLAGS) passes none; its error is 1 ulp of |log v| (2 units), with no argument-dependent term:
    2 |v log v| in A_kl beside the propagated A_v (|log v| + 1).
  * powf (p != 2) is the OCML pow, documented to 1 ulp (2 units): |f|^p enters A three times instead of once.
These terms enter A from the header, the ISA / library documentation and arithmetic only, never from a GPU run.

Errors are judged per element: |got - ref64| <= K * 2^-24 * A + tiny, K = max(8, 4 * K32) per family, K32 the largest error of the fp32
CPU evaluation over every case of KD_CASES in the same unit (test_kd_ref_cpu.py measures it and asserts K32 <= K / 4).  No constant comes
from a GPU run of the kernels."""
import functools

import torch

from elt_ref import ratio, rng, SENTINEL, f32, cdiv, U, TINY                                   # noqa: F401

CLAMP = f32(1e-12)                   # the C float 1e-12f the kernels clamp with
MTA_RC = AT_RC = 16                  # register slots per thread (loss.hip)
MTA_MAX_LEV, MTA_MAX_T = 5, 4
EXP_UNITS = 2.0                      # v_exp_f32 / OCML pow / __builtin_logf: 1 ulp = 2 units of 2^-24

# K per family = max(8, 4 * K32).  K32 as test_kd_ref_cpu.py measures it (fp32 CPU evaluation of these references on every case):
K32 = {"att": 3.521, "att_bwd": 1.663, "kl_loss": 0.503, "kl_da": 0.988, "at_loss": 0.547, "at_part": 0.735, "at_da": 3.596}
K_BY_FAMILY = {"att": 15.0, "att_bwd": 8.0, "kl_loss": 8.0, "kl_da": 8.0, "at_loss": 8.0, "at_part": 8.0, "at_da": 15.0}


# ------------------------------------------------------------------------------------------------ references
def attention(f, p):
    """a[r] = mean_c f[r, c]^p.  f [rows, C]"""
    C = f.shape[1]
    t = f * f if p == 2 else f.pow(p)
    return t.sum(1) / C, t.abs().sum(1) * (1.0 if p == 2 else 1.0 + EXP_UNITS) / C


def attention_bwd(f, da, p, df0=None):
    """df[r, c] = (df0 +) da[r] * p * f^(p-1) / C"""
    C = f.shape[1]
    k = (da * p / C).unsqueeze(1)
    v = k * (f if p == 2 else f.pow(p - 1))
    A = v.abs() * (1.0 if p == 2 else 1.0 + EXP_UNITS)
    return (v, A) if df0 is None else (df0 + v, df0.abs() + A)


def l2hat(a):
    """F.normalize over HW: -> (ahat, A, clamped norm, raw norm), all [B, HW] / [B, 1]"""
    raw = (a * a).sum(1, keepdim=True).sqrt()
    n = raw.clamp_min(CLAMP)
    h = a / n
    return h, h.abs(), n, raw


def teacher_hat(ts):
    """one map: its L2 normalisation; several (list mode): the L1-normalised product of the L2-normalised maps"""
    if len(ts) == 1:
        return l2hat(ts[0])[:2]
    q = None
    for t in ts:
        h = l2hat(t)[0]
        q = h if q is None else q * h
    Aq = q.abs() * len(ts)
    l1 = q.abs().sum(1, keepdim=True).clamp_min(CLAMP)
    that = q / l1
    return that, Aq / l1 + that.abs() * Aq.sum(1, keepdim=True) / l1


def softmax(x, Ax):
    mx = x.max(1, keepdim=True)[0]
    d = x - mx
    e = torch.exp(d)
    Ae = e * (EXP_UNITS + Ax + mx.abs() + 2 * d.abs())
    s = e.sum(1, keepdim=True)
    u = e / s
    return u, Ae / s + u * Ae.sum(1, keepdim=True) / s


def mta_pair(a_s, ts, T, gscale):
    """One (student, teacher(s)) pair of one level.  -> (kl [B], A_kl [B], d [B, HW], A_d): the launch adds kl.sum() / B to its loss
    slot and d to (or stores it as) da_s"""
    B = a_s.shape[0]
    ah, Aah, ns, _ = l2hat(a_s)
    that, Ath = teacher_hat(ts)
    u, Au = softmax(ah / T, Aah / T)
    v, Av = softmax(that / T, Ath / T)
    pos = v > 0
    lg = torch.where(pos, torch.log(torch.where(pos, v, torch.ones_like(v))), torch.zeros_like(v))
    vlv = v * lg
    kl = (vlv - v * u).sum(1)
    Akl = (Av * (lg.abs() + 1) + EXP_UNITS * vlv.abs() + Av * u + v * Au).sum(1)
    dot = -(v * u).sum(1, keepdim=True)
    Adot = (Av * u + v * Au).sum(1, keepdim=True)
    w, Aw = -v - dot, Av + Adot
    dah, Adah = u * w / T, (Au * w.abs() + u * Aw) / T
    dad = (ah * dah).sum(1, keepdim=True)
    Adad = (Aah * (dah.abs() + Adah)).sum(1, keepdim=True)
    sc = gscale / B
    d = (dah - ah * dad) / ns * sc
    Ad = (Adah + ah.abs() * Adad + (ah * dad).abs()) / ns * abs(sc)
    return kl, Akl, d, Ad


def mta_kl(a_s, ts, T, gscale, loss0, da0=None):
    """mmd_mta_kl (list of teachers multiplied) -> {"loss": loss0 + sum_b kl / B, "da": (da0 +) d}"""
    B = a_s.shape[0]
    kl, Akl, d, Ad = mta_pair(a_s, ts, T, gscale)
    out = {"loss": (loss0 + kl.sum() / B, loss0.abs() + Akl.sum() / B)}
    out["da"] = (d, Ad) if da0 is None else (da0 + d, da0.abs() + Ad)
    return out


def mta_multi(a_s, a_t, list_mode, T, gscale, loss0, da0=None):
    """mmd_mta_kl_multi.  a_s [lev], a_t [teacher][lev].  pairwise: loss[t * nlev + l], da[l] = (da0[l] +) sum_t d; list: loss[l], da[l] = d
    -> {"loss": ([slots], A), "da": [(value, A) per level]}"""
    nlev, nt = len(a_s), len(a_t)
    loss, Aloss, da = loss0.clone(), loss0.abs(), []
    for l in range(nlev):
        B = a_s[l].shape[0]
        groups = [[a_t[k][l] for k in range(nt)]] if list_mode else [[a_t[k][l]] for k in range(nt)]
        tot = Atot = None
        for t, ts in enumerate(groups):
            kl, Akl, d, Ad = mta_pair(a_s[l], ts, T, gscale)
            loss[t * nlev + l] += kl.sum() / B
            Aloss[t * nlev + l] += Akl.sum() / B
            tot, Atot = (d, Ad) if tot is None else (tot + d, Atot + Ad)
        if da0 is not None and not list_mode:
            tot, Atot = da0[l] + tot, da0[l].abs() + Atot
        da.append((tot, Atot))
    return {"loss": (loss, Aloss), "da": da}


def at_multi(a_s, a_t, gscale):
    """mmd_at_loss_multi -> {"loss": [nt * nlev], "part": [nt * nlev * B], "da": [per level]}"""
    nlev, nt = len(a_s), len(a_t)
    B = a_s[0].shape[0]
    z = a_s[0].new_zeros
    loss, Aloss, part, Apart, das = z(nt * nlev), z(nt * nlev), z(nt * nlev * B), z(nt * nlev * B), []
    for l in range(nlev):
        HW = a_s[l].shape[1]
        ah, Aah, ns, raw = l2hat(a_s[l])
        G = AG = None
        for k in range(nt):
            th, Ath = l2hat(a_t[k][l])[:2]
            d, Ad = ah - th, Aah + Ath
            p_, Ap_ = (d * d).sum(1), (2 * d.abs() * Ad + d * d).sum(1)
            i = k * nlev + l
            part[i * B:(i + 1) * B], Apart[i * B:(i + 1) * B] = p_, Ap_
            loss[i], Aloss[i] = p_.sum() / (B * HW), Ap_.sum() / (B * HW)
            G, AG = (d, Ad) if G is None else (G + d, AG + Ad)
        dot = (ah * G).sum(1, keepdim=True)
        Adot = (Aah * (AG + G.abs())).sum(1, keepdim=True)
        cg = 2.0 * gscale / (float(B) * float(HW))
        clamped = ~(raw > CLAMP)
        da = torch.where(clamped, cg * G / CLAMP, cg * (G - ah * dot) / ns)
        Ada = torch.where(clamped, abs(cg) * AG / CLAMP, abs(cg) * (AG + ah.abs() * Adot + (ah * dot).abs()) / ns)
        das.append((da, Ada))
    return {"loss": (loss, Aloss), "part": (part, Apart), "da": das}


# ------------------------------------------------------------------------------------------------ the dispatch, copied
def route_att(rows, C):
    """mmd_mta_attention -> (blocks of 4 rows, rows in the last block, float4 trips of `c = lane * 4; c < C; c += 256`, lanes active in the
    last trip); None: refused (C % 4).  A COPY of loss.hip's host code and loop bounds: keep it in step by hand"""
    if rows <= 0 or C <= 0 or C & 3:
        return None
    return cdiv(rows, 4), (rows - 1) % 4 + 1, cdiv(C, 256), ((C - 1) % 256) // 4 + 1


def route_att_bwd(rows, C):
    """mmd_mta_attention_bwd -> (blocks, float4s in the last block)"""
    if rows <= 0 or C <= 0 or C & 3:
        return None
    n = rows * (C // 4)
    return cdiv(n, 256), (n - 1) % 256 + 1


def route_kl(list_mode, HW, nt):
    """one level of mmd_mta_kl_multi -> (body, register slots that hold data, how da is written)"""
    if list_mode:
        return ("generic", 0, "store")
    how = "atomic" if nt > 1 else "store"
    if HW <= 256 * MTA_RC:
        return ("cached", cdiv(HW, 256), how)
    return ("generic", 0, how)


def route_at(HW):
    """one level of mmd_at_loss_multi -> (register chunks, slots that hold data in the last chunk)"""
    nch = cdiv(HW, 256 * AT_RC)
    return nch, cdiv(HW - (nch - 1) * 256 * AT_RC, 256)


def refused_multi(nlev, nt, T=1.0, B=1):
    return nlev < 1 or nlev > MTA_MAX_LEV or nt < 1 or nt > MTA_MAX_T or B <= 0 or not T > 0


# ------------------------------------------------------------------------------------------------ cases
def _att(name, rows, C, p, kind="signed", why=""):
    return {"name": name, "entry": "att", "rows": rows, "C": C, "p": p, "kind": kind, "why": why}


def _lv(name, entry, levels, nt, B=2, T=9.0, list_mode=False, flags=(), signed=False, gscale=0.005, why=""):
    return {"name": name, "entry": entry, "levels": list(levels), "nt": nt, "B": B, "T": T, "list": list_mode, "flags": tuple(flags),
            "signed": signed, "gscale": gscale, "why": why}


SPECIAL = ("zero_s", "zero_t", "spike")          # image 0: all-zero student map; image B-1: all-zero last teacher map; image 1: one spike
PYRAMID = (64, 16, 4, 1, 1)                      # five levels' pixel counts of one image, concatenated in one launch


def _cases():
    cs = []
    # ---- attention maps, forward and backward
    for C in (4, 12, 64, 252, 256, 260, 288, 384):
        cs.append(_att("att_r5_c%d_p2" % C, 5, C, 2.0, why="%d float4 trip(s), %d lanes in the last" % route_att(5, C)[2:]))
    cs.append(_att("att_r1_c4_p2", 1, 4, 2.0, why="one row, one lane"))
    cs.append(_att("att_r1_c260_p3", 1, 260, 3.0, why="one row, second trip with one lane, powf on signed features"))
    cs.append(_att("att_r1029_c12_p2", 1029, 12, 2.0, why="258 blocks, the last holds one row; backward: 3087 float4s, 13 blocks"))
    cs.append(_att("att_r1029_c260_p1", 1029, 260, 1.0, kind="zeros", why="p = 1 on signed features with exact zeros: powf(0, 0) in the backward"))
    cs.append(_att("att_r5_c12_p3", 5, 12, 3.0, why="powf, signed"))
    cs.append(_att("att_r5_c12_p1", 5, 12, 1.0, kind="zeros", why="p = 1"))
    cs.append(_att("att_r5_c288_p3", 5, 288, 3.0, why="powf across two trips"))
    cs.append(_att("att_r5_c64_p2.5", 5, 64, 2.5, kind="positive", why="non-integer p on positive features"))
    cs.append(_att("att_r5_c260_p2.5", 5, 260, 2.5, kind="positive", why="non-integer p, two trips"))
    cs.append(_att("att_pyramid_c64_p2", 2 * sum(PYRAMID), 64, 2.0, why="five levels' rows of two images in one launch"))
    cs.append(_att("att_pyramid_c288_p3", 2 * sum(PYRAMID), 288, 3.0, why="the same at the 288-wide BiFPN with cfg p = 3"))
    # ---- mmd_mta_kl: HW x B, nt cycling; every accumulate mode and da_s = NULL is run on each
    i = 0
    for HW in (1, 2, 63, 256, 257, 1000):
        for B in (1, 3):
            cs.append(_lv("kl_hw%d_b%d" % (HW, B), "kl", [HW], 1 + i % 3, B=B, T=(9.0, 1.0, 0.05)[(i // 3) % 3], why="nt %d" % (1 + i % 3)))
            i += 1
    cs.append(_lv("kl_special_nt1", "kl", [257], 1, B=3, flags=SPECIAL, why="zero student, zero teacher, spike"))
    cs.append(_lv("kl_special_nt3", "kl", [257], 3, B=3, T=0.05, flags=SPECIAL, signed=True, why="the same in list form, signed teachers, sharp T"))
    # ---- mmd_mta_kl_multi, pairwise
    cs.append(_lv("pair_nlev1_nt1", "multi", [4096], 1, why="the exact register boundary, store mode"))
    cs.append(_lv("pair_nlev3_nt2", "multi", [1, 4097, 256], 2, why="generic body beside cached ones, atomics"))
    cs.append(_lv("pair_nlev5_nt3", "multi", [255, 257, 1024, 4095, 4352], 3, why="1, 2, 4, 16 slots and the generic body, atomics"))
    cs.append(_lv("pair_nlev5_nt1_T1", "multi", [4096, 1, 4097, 255, 1024], 1, T=1.0, why="store mode across both bodies"))
    cs.append(_lv("pair_special_T05", "multi", [257, 4097, 4096], 2, B=3, T=0.05, flags=SPECIAL, why="zero / spike images in both bodies, sharp T"))
    cs.append(_lv("pair_special_nt1", "multi", [257, 4352], 1, B=3, flags=SPECIAL, why="zero / spike images, store mode"))
    # ---- mmd_mta_kl_multi, list mode
    for nt in (1, 2, 3, 4):
        cs.append(_lv("list_nt%d" % nt, "multi", [63, 4097, 256], nt, list_mode=True, T=(9.0, 1.0)[nt % 2], why="list of %d" % nt))
    cs.append(_lv("list_signed_nt3", "multi", [257, 1024], 3, list_mode=True, signed=True, why="signed teacher maps: fabs in the L1 norm"))
    cs.append(_lv("list_special_nt4", "multi", [255, 4096, 1], 4, B=3, T=0.05, list_mode=True, flags=SPECIAL, why="zero / spike images, sharp T, 4 maps"))
    cs.append(_lv("list_nlev5_nt2", "multi", [1, 255, 257, 1024, 4352], 2, list_mode=True, why="five levels"))
    # ---- mmd_at_loss_multi
    cs.append(_lv("at_nlev5_nt3", "at", [1, 255, 4096, 4097, 8193], 3, why="1, 1, 1, 2, 3 chunks"))
    cs.append(_lv("at_nlev1_nt4", "at", [8193], 4, why="three chunks, four teachers"))
    cs.append(_lv("at_nlev1_nt1", "at", [4096], 1, B=1, why="the exact chunk boundary, one image"))
    cs.append(_lv("at_nlev1_nt2", "at", [4097], 2, B=3, why="one element in the second chunk"))
    cs.append(_lv("at_special_nlev5", "at", [255, 4097, 1, 8193, 4096], 2, B=3, flags=SPECIAL, why="zero student (the g / 1e-12 branch), zero teacher, spike"))
    return cs


KD_CASES = _cases()
CASE = {c["name"]: c for c in KD_CASES}
assert len(CASE) == len(KD_CASES)


def cases_of(*entries):
    return [c["name"] for c in KD_CASES if c["entry"] in entries]


def _gen(case):
    g = rng(71, sum(map(ord, case["name"])) % 9973)
    rn = lambda *sh: torch.randn(*sh, generator=g)
    ru = lambda *sh: torch.rand(*sh, generator=g)
    if case["entry"] == "att":
        rows, C = case["rows"], case["C"]
        f = rn(rows, C) * 1.3
        if case["kind"] == "positive":
            f = f.abs() + 0.05
        if case["kind"] == "zeros":
            f[:, 1::3] = 0.0
        da = rn(rows) * 0.1
        da[::3] = 0.0                                                    # rows whose gradient is exactly zero
        return {"f": f, "da": da, "df0": rn(rows, C) * 0.3}
    B, nt, nlev = case["B"], case["nt"], len(case["levels"])
    d = {"a_s": [], "a_t": [[] for _ in range(nt)], "da0": []}
    for HW in case["levels"]:
        a = ru(B, HW) * 1.5 + 0.1                                        # attention maps of even p are means of powers: positive
        ts = [(rn(B, HW) if case["signed"] else ru(B, HW) * (1.0 + k) + 0.05) for k in range(nt)]
        if "zero_s" in case["flags"]:
            a[0] = 0.0
        if "zero_t" in case["flags"]:
            ts[nt - 1][B - 1] = 0.0
        if "spike" in case["flags"]:
            a[1 % B] = 0.0
            a[1 % B, HW // 2] = 2.5
            ts[0][1 % B] = 0.0
            ts[0][1 % B, HW // 3] = 0.7
        d["a_s"].append(a)
        for k in range(nt):
            d["a_t"][k].append(ts[k])
        d["da0"].append(rn(B, HW) * 1e-3)
    d["loss0"] = rn((1 if case["list"] else nt) * nlev) * 0.5
    return d


@functools.lru_cache(maxsize=None)
def _inputs(name):
    return _gen(CASE[name])


def case_inputs(case):
    """fp32 CPU tensors of one case, the same for the CPU calibration and the GPU test; cached - do not modify"""
    return _inputs(case["name"])


def to(x, dt, dev="cpu"):
    if isinstance(x, torch.Tensor):
        return x.to(device=dev, dtype=dt)
    if isinstance(x, list):
        return [to(v, dt, dev) for v in x]
    if isinstance(x, dict):
        return {k: to(v, dt, dev) for k, v in x.items()}
    return x


def case_ref(case, inp, dt, dev="cpu", start=None):
    """reference of one case in dtype dt.  start: what da_s holds on entry where the launch adds to it - None (a store, or zeros) or "da0"
      att   -> {"a", "df" (accumulate 0), "df_acc" (accumulate 1)}
      kl    -> {"loss", "da"}          multi -> {"loss", "da": [per level]}          at -> {"loss", "part", "da": [per level]}"""
    d = to(inp, dt, dev)
    e = case["entry"]
    if e == "att":
        p = case["p"]
        return {"a": attention(d["f"], p), "df": attention_bwd(d["f"], d["da"], p), "df_acc": attention_bwd(d["f"], d["da"], p, d["df0"])}
    gs = f32(case["gscale"])
    T = f32(case["T"])
    da0 = d["da0"] if start == "da0" else None
    if e == "kl":
        return mta_kl(d["a_s"][0], [t[0] for t in d["a_t"]], T, gs, d["loss0"][0], None if da0 is None else da0[0])
    if e == "multi":
        return mta_multi(d["a_s"], d["a_t"], case["list"], T, gs, d["loss0"], da0)
    return at_multi(d["a_s"], d["a_t"], gs)


FAMILY = {("att", "a"): "att", ("att", "df"): "att_bwd", ("att", "df_acc"): "att_bwd", ("kl", "loss"): "kl_loss", ("kl", "da"): "kl_da",
          ("multi", "loss"): "kl_loss", ("multi", "da"): "kl_da", ("at", "loss"): "at_loss", ("at", "part"): "at_part", ("at", "da"): "at_da"}


def flat(ref):
    """{name: (value, A) | [(value, A) per level]} -> [(name, label, value, A)]"""
    out = []
    for k, v in ref.items():
        if isinstance(v, list):
            out += [(k, "%s[%d]" % (k, l), a, b) for l, (a, b) in enumerate(v)]
        else:
            out.append((k, k, v[0], v[1]))
    return out
