"""CPU checks of tests/bd_ref.py, the float64 reference of the 1x1-conv input-gradient entry points (mmd_pwconv_bwd_data*, csrc/pw_gemm.hip and
pw_slab.hip).  Sizes as in bd_ref: M rows, K input and N output channels; the GEMM reduces over Kg = N and writes Ng = K columns.
  1. the reference against torch autograd in float64 of conv1x1 -> BatchNorm2d(train) -> [swish] -> * mul_b on two small shapes (dx, dz, dgamma,
     dbeta, with the sums of elt_ref.bn_bwd_reduce), and its epilogue jobs (residual, upstream sums, five-plane pool) against formulas written
     independently with explicit loops;
  2. the tolerance constants K of bd_ref are calibrated here, on the CPU models its docstring describes, on every (case, mode) the GPU test
     runs: the stored K32 is the measured one to within 5 % + 0.01 (not compared below 2, where the floor K = 8 decides), no model exceeds
     K / 4, and K = max(8, ceil(4 * K32));
  3. through the copy of the host dispatch (bd_ref.route / slab_plan) the case table reaches every branch the GPU test exists for, every forced
     case lands in the family it names, and the copy reproduces values worked out by hand from the source."""
import functools
import os

import pytest
import torch

import bd_ref as R
import pw_ref
from elt_ref import ratio, swish, chan_pool_bwd, U, EPS

D, S32 = torch.float64, torch.float32


# ------------------------------------------------------------------------------------------------ 1. the reference
@pytest.mark.parametrize("B,H,K,N,act,mulb", [(3, 7, 12, 8, 1, True), (2, 14, 8, 20, 0, True), (3, 7, 12, 8, 0, False), (2, 14, 8, 20, 1, False)])
def test_reference_matches_float64_autograd(B, H, K, N, act, mulb):
    """two shapes, images of 7 (= BN_RPI) rows: dx, dz, dgamma, dbeta of the reference are autograd's"""
    M = B * H
    assert M % R.BN_RPI == 0
    g = R.rng(51, B, H, K, N)
    nimg = M // R.BN_RPI
    x = torch.randn(nimg, K, R.BN_RPI, 1, generator=g, dtype=D).requires_grad_(True)
    conv = torch.nn.Conv2d(K, N, 1, bias=False).double()
    bnm = torch.nn.BatchNorm2d(N, eps=EPS).double().train()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(N, K, 1, 1, generator=g, dtype=D) / K ** 0.5)
        bnm.weight.copy_(torch.rand(N, generator=g, dtype=D) + 0.5)
        bnm.bias.copy_(torch.randn(N, generator=g, dtype=D) * 0.2)
    mul_b = torch.rand(nimg, generator=g, dtype=D) + 0.2
    mul_b[1] = 0.0
    gy = torch.randn(nimg, N, R.BN_RPI, 1, generator=g, dtype=D)
    z4 = conv(x)
    z4.retain_grad()
    y = bnm(z4)
    a = swish(y) if act else y
    if mulb:
        a = a * mul_b.view(-1, 1, 1, 1)
    (a * gy).sum().backward()
    rows = lambda t: t.detach().permute(0, 2, 3, 1).reshape(M, -1)
    z = rows(z4)
    mean, var = z.mean(0), z.var(0, unbiased=False)
    invstd = (var + EPS).rsqrt()
    scale = bnm.weight.detach() * invstd
    d = {"g": rows(gy), "z": z, "wt": conv.weight.detach().view(N, K).t().contiguous(), "scale": scale, "shift": bnm.bias.detach() - mean * scale,
         "mean": mean, "invstd": invstd, "mul_b": mul_b, "dgamma0": torch.zeros(N, dtype=D), "dbeta0": torch.zeros(N, dtype=D)}
    case = {"M": M, "K": K, "N": N, "B": 1}
    mode = " ".join((["act"] if act else []) + (["mulb"] if mulb else []))
    sums = R.case_sums(case, mode, d)
    out = R.case_ref(case, mode, d, sums)
    for name, want in (("dx", rows(x.grad)), ("dz", rows(z4.grad)), ("dgamma", bnm.weight.grad), ("dbeta", bnm.bias.grad)):
        v, A = out[name]
        assert v.shape == want.shape and float(((v - want).abs() / A).max()) <= 1e-12, name
        assert bool((A >= v.abs() * (1 - 1e-12)).all()) and bool((A > 0).all()), name
    assert float((out["dz"][0].t() @ rows(x) - conv.weight.grad.view(N, K)).abs().max()) <= 1e-11          # the weight gradient the stored dz is for


def test_epilogue_jobs_match_naive_formulas():
    """residual, upstream sums (with and without xs_mul_b) and the five-plane pool from the completed dx, with explicit loops"""
    case = R._c("naive", 20, 12, 8, ["bn2"], None, ["act mulb res xsm", "alias xs", "act p5"], "", B=2)
    M, K, N = case["M"], case["K"], case["N"]
    d = R.to(R.case_inputs(case), D)
    for mode in case["modes"]:
        f = R.flags(mode)
        sums = R.case_sums(case, mode, d)
        out = R.case_ref(case, mode, d, sums)
        base = R.case_ref(case, " ".join(t for t in mode.split() if t in ("act", "mulb")), d, sums)["dx"][0]
        dx = base + (d["res"] if f["res"] else 0)
        assert float((out["dx"][0] - dx).abs().max()) <= 1e-13
        if f["xs"]:
            s, q = d["xs0"][:K].clone(), d["xs0"][K:].clone()
            for m in range(M):
                mb = float(d["xs_mul_b"][m // R.XS_RPI]) if f["xs"] == "xsm" else 1.0
                for k in range(K):
                    gp = float(dx[m, k]) * mb
                    s[k] += gp
                    q[k] += gp * (float(d["xs_z"][m, k]) - float(d["xs_mean"][k])) * float(d["xs_invstd"][k])
            for name, want in (("xs_sum", s), ("xs_sumsq", q)):
                v, A = out[name]
                assert float(((v - want).abs() / A).max()) <= 1e-13 and bool((A >= v.abs() * (1 - 1e-12)).all()), name
        if f["p5"]:
            v, A = out["p5"]
            want, A0 = chan_pool_bwd(d["p5_z"], d["p5_scale"], d["p5_shift"], d["p5_mean"], d["p5_invstd"], dx, d["p5_0"], case["B"], M // case["B"])
            assert torch.equal(v, want) and v.shape == (5, case["B"], K)
            assert bool((A[:3] >= A0[:3] * (1 - 1e-12)).all()) and torch.equal(A[3:], A0[3:])
            rpi = M // case["B"]
            u = d["p5_z"] * d["p5_scale"] + d["p5_shift"]
            want0 = d["p5_0"][0, 1] + (dx * swish(u))[rpi:].sum(0)          # plane 0 of the second image: its own rows only
            assert float((v[0, 1] - want0).abs().max()) <= 1e-12


def test_plain_reference_is_the_forward_with_sizes_swapped():
    d, (dx, A) = R.plain_ref("t1_acc", True, D)
    assert float((dx - (d["x"] @ d["w"].t() + d["res"])).abs().max()) <= 1e-13 and dx.shape == d["res"].shape
    _, (dx0, _) = R.plain_ref("t1_acc", False, D)
    assert float((dx0 - d["x"] @ d["w"].t()).abs().max()) <= 1e-13


# ------------------------------------------------------------------------------------------------ 2. calibration of K
@functools.lru_cache(maxsize=None)
def _k32():
    """K32 per family over every (case, mode) of BD_CASES and every plain case, where each family's worst sits, and the smallest A met"""
    k32 = {f: (0.0, "") for f in R.K_BY_FAMILY}
    a_min = [float("inf")]

    def take(where, model, r64, bf):
        for out, (v, A) in r64.items():
            a_min[0] = min(a_min[0], float(A.min()))
            fam = R.family_of(out)
            if bf:
                if fam not in R.BF16_FAMILIES:
                    continue          # (dz / dgamma / dbeta of a bf16 entry point are the fp32 model's: judged in the fp32 families)
                fam, got = fam + "_bf16", model[out + "_bf16"][0]
            else:
                got = model[out][0]
            r = ratio(got, v, A) * (U / R.UNIT[fam])
            if r > k32[fam][0]:
                k32[fam] = (r, where)

    for case in R.BD_CASES:
        inp = R.case_inputs(case)
        d64, d32 = R.to(inp, D), R.to(inp, S32)
        has_bf16 = any(R.FORMS[f][2] for f in case["forms"])
        for mode in case["modes"]:
            sums = R.case_sums(case, mode, d64)
            r64 = R.case_ref(case, mode, d64, sums)
            where = "%s [%s]" % (case["name"], mode)
            take(where, R.case_ref(case, mode, d32, sums, dot=R.seq_dot, kernel_order=True), r64, False)
            if has_bf16:
                take(where, R.case_ref(case, mode, d32, sums, bf16=True, kernel_order=True), r64, True)
    for name, _ in R.PLAIN_CASES:
        for acc in (0, 1):
            r64 = {"dx": R.plain_ref(name, acc, D)[1]}
            where = "plain %s acc %d" % (name, acc)
            take(where, {"dx": R.plain_ref(name, acc, S32, dot=R.seq_dot)[1]}, r64, False)
            take(where, {"dx_bf16": R.plain_ref(name, acc, S32, bf16=True)[1]}, r64, True)
    return k32, a_min[0]


@pytest.mark.parametrize("family", sorted(R.K_BY_FAMILY))
def test_stored_constant_is_the_calibrated_one(family):
    """K = max(8, ceil(4 * K32)), K32 measured here on the CPU models; nothing of it comes from the kernels"""
    k32, where = _k32()[0][family]
    K = R.K_BY_FAMILY[family]
    print("BD K32 %-14s %.3f  (K %.1f, unit 2^%d)  worst at %s" % (family, k32, K, -9 if family.endswith("bf16") else -24, where))
    if max(k32, R.K32[family]) >= 2.0:          # (below 2 the floor K = 8 decides, and the last digits of K32 - one ulp of the CPU's fp32 sigmoid - do not matter)
        assert abs(R.K32[family] - k32) <= 0.05 * k32 + 0.01, "the K32 recorded in bd_ref.py is not the one measured"
    assert K == max(8.0, float(-(-4 * R.K32[family] // 1))), "K is not max(8, ceil(4 * K32))"
    assert k32 <= K / 4 or K == 8.0 and k32 <= 2.0


def test_inputs_are_well_conditioned():
    """no output element with A == 0; every mul_b of two images or more has its dropped sample; the images divide no tile"""
    assert _k32()[1] > 0
    for case in R.BD_CASES:
        if case["M"] > R.BN_RPI:
            assert float(R.case_inputs(case)["mul_b"][1]) == 0.0
    assert all(t % R.BN_RPI and t % R.XS_RPI for t in (32, 64, 128))


def test_small_faults_exceed_the_constants():
    """the bounds are not so wide that the faults this suite exists for hide under them: on the fp32 model, a dropped Kg % 8 == 4 tail, dgamma
    added by a second column tile, coefficients read one channel off for the last four channels, and a pool that takes one 32-row tile of
    the neighbouring image each exceed K (none of them moves its tensor's largest element by 5e-4)"""
    def worst(fam, got, ref):
        return ratio(got, ref[0], ref[1]) / R.K_BY_FAMILY[fam]

    case, mode = R.CASE["t1_k12"], R.SA
    inp = R.case_inputs(case)
    d64, d32 = R.to(inp, D), R.to(inp, S32)
    sums = R.case_sums(case, mode, d64)
    r64, m32 = R.case_ref(case, mode, d64, sums), R.case_ref(case, mode, d32, sums, dot=R.seq_dot, kernel_order=True)
    dz = m32["dz"][0]
    assert worst("dx", R.seq_dot(dz[:, :-4].contiguous(), d32["wt"][:, :-4].contiguous()), r64["dx"]) > 1
    assert worst("dsum", m32["dgamma"][0] + sums[case["N"]:].float(), r64["dgamma"]) > 1
    off = {k: (torch.roll(v, 1) if k in ("scale", "shift", "mean", "invstd") else v) for k, v in d32.items()}
    dz_off = dz.clone()
    dz_off[:, -4:] = R.case_ref(case, mode, off, sums, kernel_order=True)["dz"][0][:, -4:]
    assert worst("dz", dz_off, r64["dz"]) > 1 and worst("dx", R.seq_dot(dz_off, d32["wt"]), r64["dx"]) > 1
    assert float((dz_off - dz).abs().max()) > 0
    case, mode = R.CASE["sk_p5"], R.SP
    inp = R.case_inputs(case)
    d64, d32 = R.to(inp, D), R.to(inp, S32)
    sums = R.case_sums(case, mode, d64)
    r64, m32 = R.case_ref(case, mode, d64, sums), R.case_ref(case, mode, d32, sums, dot=R.seq_dot, kernel_order=True)
    dx, A = m32["dx"]
    p5 = {"z": torch.roll(d32["p5_z"], 32, 0), "scale": d32["p5_scale"], "shift": d32["p5_shift"], "mean": d32["p5_mean"], "invstd": d32["p5_invstd"],
          "out0": d32["p5_0"], "B": case["B"]}
    assert worst("p5", R.p5_ref(torch.roll(dx, 32, 0), A, p5)[0], r64["p5"]) > 1
    assert worst("p5", m32["p5"][0], r64["p5"]) <= 0.25


# ------------------------------------------------------------------------------------------------ 3. coverage
DISPATCH_ENV = ["MMD_SKINNY_K", "MMD_STREAM", "MMD_SKINNY_TILES", "MMD_SQ_TILES", "MMD_SQ_MIN", "MMD_BN32_GAIN", "MMD_NO_LEAN", "MMD_SK_PF2",
                "MMD_SK_BQ_LDS", "MMD_NO_BQ_LDS", "MMD_BQ_LDS_CAP_KB", "MMD_NO_SLAB", "MMD_SLAB_BLOCKS", "MMD_NO_LONGK", "MMD_NO_ROWS"]


def test_no_dispatch_override_in_the_environment():
    """the variables pw_dispatch, pw_bq_lds, slab_plan and pw_slab_try read; MMD_MFMA_F32 is the one exception - the GPU test passes it on"""
    assert not [k for k in DISPATCH_ENV if k in os.environ]


def _recs():
    return [(c, m, f, R.route_mode(c, m, f)) for c in R.BD_CASES for m, f in R.runs(c)]


def test_cases_are_legal():
    for c in R.BD_CASES:
        assert c["K"] % 4 == 0 and c["N"] % 4 == 0 and c["M"] % c["B"] == 0 and (c["Kg"], c["Ng"]) == (c["N"], c["K"]) and c["why"]
        assert R.runs(c) and all(f in R.FORMS for f in c["forms"])
        for m in c["modes"]:
            f = R.flags(m)
            assert not (f["p5"] and (f["res"] or f["xs"])), "p5 goes with neither a residual nor upstream sums"
            assert not f["ws"] or f["xs"], "a slot workspace belongs to upstream sums"


def test_cases_reach_every_branch():
    recs = _recs()
    missing = []

    def need(what, form=None, mode=None, case=None, **want):
        for c, m, f, r in recs:
            if form and f not in form:
                continue
            if mode and not mode(R.flags(m)):
                continue
            if case and not case(c):
                continue
            if all((v(r.get(k)) if callable(v) else r.get(k) == v) for k, v in want.items()):
                return
        missing.append(what)

    # ---- every (kernel, nkl, half group, MFMA form) of the LDS-tiled <PRO 1> kernels
    for nkl in (1, 2, 3, 4):
        for half in (False, True):
            for mfma, form in (("f32", ("f2", "f2n")), ("bf16", ("bf16",))):
                need("128x32 nkl %d half %d %s" % (nkl, half, mfma), form=form, family="tiled", bm=128, nkl=nkl, half_group=half, mfma=mfma, ntm=1)
            for mfma, form in (("f32", ("f2n",)), ("split", ("f2",)), ("bf16", ("bf16",))):
                need("64x64 nkl %d half %d %s" % (nkl, half, mfma), form=form, family="tiled", bm=64, nkl=nkl, half_group=half, mfma=mfma)
                need("64x64 nkl %d half %d %s, Ng = 52" % (nkl, half, mfma), form=form, family="tiled", bm=64, nkl=nkl, half_group=half, mfma=mfma,
                     case=lambda c: c["Ng"] == 52 and 68 <= c["Kg"] <= 96)
        need("64x64 split nkl %d on two column tiles with Ng %% 64 = 4" % nkl, form=("f2",), family="tiled", bm=64, nkl=nkl, mfma="split", ntn=2, col_tail=4)
    for Kg, Ng, mfma in ((60, 52, "f32"), (64, 48, "f32"), (64, 52, "split")):
        need("split switch Kg %d Ng %d" % (Kg, Ng), form=("f2",), family="tiled", mfma=mfma, case=lambda c: (c["Kg"], c["Ng"]) == (Kg, Ng))
    need("128x32 for 16 < Ng <= 32 at big_tiles 160", family="tiled", bm=128, big_tiles=160, case=lambda c: c["Ng"] == 32)
    need("skinny for 16 < Ng <= 32 at big_tiles 159", family="skinny", big_tiles=159, case=lambda c: c["Ng"] == 32)
    need("128x32 more than one row block", family="tiled", bm=128, ntm=lambda n: n > 1)
    for M in (1, 33):
        for fam in ("tiled", "skinny"):
            need("%s M %d" % (fam, M), family=fam, case=lambda c: c["M"] == M)
    need("128x32 Ng 4", family="tiled", bm=128, case=lambda c: c["Ng"] == 4)
    # ---- the coefficient table
    for Kg, form, mfma, table in ((1024, ("f2",), "f32", True), (1028, ("f2",), "f32", False), (1024, ("bf16",), "bf16", True), (1028, ("bf16",), "bf16", False),
                                  (560, ("f2",), "split", True), (564, ("f2",), "split", False), (564, ("f2n",), "f32", True), (564, ("bf16",), "bf16", True)):
        need("table %s at Kg %d (%s)" % ("on" if table else "off", Kg, mfma), form=form, family="tiled", mfma=mfma, table=table, case=lambda c: c["Kg"] == Kg)
    need("table on the 64x64 kernel", family="tiled", bm=64, table=True)
    need("table on the 128x32 kernel", family="tiled", bm=128, table=True)
    assert not any(r.get("table") for c, m, f, r in recs if r.get("family") == "skinny"), "never on the skinny kernel"
    # ---- the skinny <PRO 1> kernel
    have = {c["Kg"] % 32 for c, m, f, r in recs if r.get("family") == "skinny" and c["M"] == 300}
    missing += ["skinny Kg %% 32 = %d" % k for k in (4, 8, 12, 16, 20, 24, 28, 0) if k not in have]
    for Kg in (4, 32, 132, 160, 260):
        need("skinny Kg %d" % Kg, family="skinny", short_k=Kg < 128, case=lambda c: c["Kg"] == Kg)
    for mfma, form in (("f32", ("f2", "f2n", "bn", "bn2")), ("bf16", ("bf16", "bn_bf16"))):
        need("skinny %s" % mfma, form=form, family="skinny", mfma=mfma)
    need("skinny Ng 68: two column tiles, Ng % 64 = 4", family="skinny", ntn=2, col_tail=4)
    need("skinny row tail 12, col tail 40", family="skinny", row_tail=12, col_tail=40)
    # ---- the slab kernel
    for nt in range(2, 8):
        need("slab nt32 %d" % nt, family="slab", nt32=nt, nchunk=1)
    need("slab two chunks", family="slab", nchunk=2)
    for dzk in (1, 2):
        need("slab DZK %d" % dzk, family="slab", dzk=dzk)
    need("slab DZK 2 by a null dz_out", family="slab", dzk=2, row_tail=0, mode=lambda f: not f["dz"])
    need("slab DZK 2 by a ragged last slab", family="slab", dzk=2, row_tail=lambda t: t != 0, mode=lambda f: f["dz"])
    for lg in (4, 5, 6):
        need("slab sliced, combine lg %d" % lg, family="slab", lg=lg, nslice=lambda n: n > 1)
    for ns in (2, 3, 5, 8):
        need("slab %d slices" % ns, family="slab", nslice=ns)
    need("slab unsliced", family="slab", nslice=1, comb=None)
    need("slab by the auto form without a workspace (unsliced)", form=("bn2",), family="slab", nslice=1)
    need("slab by the auto form with a workspace", form=("f0w",), family="slab", nslice=lambda n: n > 1)
    need("auto form on a sliced shape without a workspace keeps the LDS kernels", form=("f0",), family="skinny", case=lambda c: c["name"] == "sl_auto")
    need("slab with the pool as its own launch", family="slab", p5="standalone")
    need("a pool in the epilogue keeps the slab kernel out, also forced", form=("f4",), family="skinny", p5="epilogue")
    c = R.CASE["sl_refused"]
    assert R.slab_refusal(c["M"], c["Kg"], c["Ng"]) and all(R.route_mode(c, m, f)["family"] == "skinny" for m, f in R.runs(c)), "the :463 refusal"
    assert R.route(4, 0, 0, 32, 512, 64, slab_ws=False) == {"rc": -22}, "form 4 on a sliced shape without a workspace"
    # ---- slots and pools, modes
    for fam, bm in (("skinny", 32), ("tiled", 64)):
        need("%s slotted" % fam, family=fam, bm=bm, slotted=True)
        need("%s pool in the epilogue" % fam, family=fam, bm=bm, p5="epilogue")
        need("%s pool stand-alone" % fam, family=fam, bm=bm, p5="standalone")
    need("128x32 pool in the epilogue", family="tiled", bm=128, p5="epilogue")
    need("128x32 pool stand-alone", family="tiled", bm=128, p5="standalone")
    for c, m, f, r in recs:
        if R.flags(m)["ws"]:
            assert r["slotted"] and not R.route_mode(c, m, f, ws_slots=0)["slotted"], (c["name"], m, f)
    for fam, pred in (("128x32", lambda r: r.get("bm") == 128), ("64x64", lambda r: r.get("bm") == 64), ("skinny", lambda r: r.get("family") == "skinny"),
                      ("slab", lambda r: r.get("family") == "slab")):
        got = [R.flags(m) for c, m, f, r in recs if pred(r)]
        for what, p in (("act 0", lambda f: not f["act"]), ("act 1", lambda f: f["act"]), ("mul_b", lambda f: f["mulb"]), ("no mul_b", lambda f: not f["mulb"]),
                        ("dz_out null", lambda f: not f["dz"]), ("dz_out", lambda f: f["dz"]), ("dgamma null", lambda f: not f["dsum"]),
                        ("dgamma", lambda f: f["dsum"]), ("no residual", lambda f: not f["res"]), ("residual aliasing dx", lambda f: f["res"] == "alias"),
                        ("xs with xs_mul_b", lambda f: f["xs"] == "xsm")):
            if not any(p(f) for f in got):
                missing.append("%s: %s" % (fam, what))
    for what, p in (("separate residual", lambda f: f["res"] == "res"), ("xs without xs_mul_b", lambda f: f["xs"] == "xs")):
        for fam in ("tiled", "skinny"):
            need("%s: %s" % (fam, what), family=fam, mode=p)
    assert not missing, missing
    # every launch lands in the family its case names; a forced slab launch that is legal never returns an error; a workspace is passed
    # exactly where slices need one
    for c, m, f, r in recs:
        assert r.get("family") == R.expected_family(c, f), (c["name"], m, f, r)
        if r["family"] == "slab":
            assert bool(R.FORMS[f][3]) == (r["nslice"] > 1), (c["name"], f)
    # the plain entry points: one case per kernel family, by pw_ref's copy of the forward dispatch
    fams = set()
    for name, fam in R.PLAIN_CASES:
        pc = pw_ref.CASE[name]
        for acc in (False, True):
            r = pw_ref.route(0, 0, 0, pc["M"], pc["K"], pc["N"], residual=acc)
            assert r["family"] == fam, (name, r)
            fams.add((r["family"], r.get("variant")))
            assert pw_ref.route(0, 0, 1, pc["M"], pc["K"], pc["N"], residual=acc)["family"] == R.PLAIN_BF16_FAMILY.get(name, fam)
    assert fams == {("tiled", 1), ("skinny", 0), ("tiled", 2), ("tiled", 3), ("longk", 0)}


def test_route_matches_hand_values():
    """worked out by hand from pw_dispatch, pw_bq_lds and slab_plan"""
    r = R.route(0, 0, 0, 100, 12, 16)
    assert (r["family"], r["bm"], r["bn"], r["nkl"], r["half_group"], r["mfma"], r["table"], r["pro"]) == ("tiled", 128, 32, 2, True, "f32", True, 1)
    assert R.route(0, 0, 0, 20352, 40, 32)["family"] == "skinny" and R.route(0, 0, 0, 20353, 40, 32)["bm"] == 128
    assert R.route(0, 0, 0, 10 ** 6, 40, 16)["bm"] == 128 and R.route(0, 0, 0, 20353, 40, 36)["bm"] == 64
    r = R.route(0, 0, 0, 10 ** 6, 96, 576)          # a forward launch of this shape takes 128x64 tiles; a BatchNorm-operand launch never does
    assert (r["bm"], r["bn"], r["mfma"]) == (64, 64, "split")
    assert [R.route(0, 0, 0, 20400, Kg, Ng)["mfma"] for Kg, Ng in ((60, 52), (64, 48), (64, 52))] == ["f32", "f32", "split"]
    assert R.route(0, 1, 0, 20400, 96, 52)["mfma"] == "f32" and R.route(0, 0, 0, 20400, 96, 52, split_default=False)["mfma"] == "f32"
    assert [R.route(0, 0, b, 100, Kg, 16)["table"] for Kg, b in ((1024, 0), (1028, 0), (1024, 1), (1028, 1))] == [True, False, True, False]
    assert [R.route(0, n, 0, 20400, Kg, 52)["table"] for Kg, n in ((560, 0), (564, 0), (564, 1), (1028, 1))] == [True, False, True, False]
    # headline launches of test_pwconv_slab_bn_operand: (M, K, N) = (2048, 208, 1248) is cut along K, (8192, 120, 720) is not
    p = R.slab_plan(2048, 1248, 208)
    assert (p["nt32"], p["nchunk"], p["nslab"], p["nslice"], p["gran"], p["lg"]) == (7, 1, 64, 4, 10, 6) and p["part_floats"] == 4 * 64 * 32 * 224
    p = R.slab_plan(8192, 720, 120)
    assert (p["nt32"], p["nslice"], p["part_floats"], p["lg"]) == (4, 1, 0, 5)
    p = R.slab_plan(2048, 2112, 352)                # two column chunks x two K slices
    assert (p["nchunk"], p["nt32"], p["nslice"]) == (2, 6, 2)
    p = R.slab_plan(96, 260, 36)                    # nine granules: gtot / 8 = 1 allows no second slice
    assert (p["nt32"], p["nslice"], p["gran"], p["lg"]) == (2, 1, 9, 4)
    assert R.slab_plan(64, 124, 100) is None and R.slab_plan(64, 256, 32) is None and R.slab_plan(64, 256, 36) is not None
    assert R.slab_plan(32, 288, 68) is None and R.slab_plan(64, 288, 68) is not None and R.slab_plan(32, 288, 68, pro=0) is not None
    assert R.route(0, 0, 0, 2048, 1248, 208, slab_ws=True)["family"] == "slab" and R.route(0, 0, 0, 2048, 1248, 208)["family"] == "skinny"
    assert R.route(0, 0, 0, 8192, 720, 120)["family"] == "slab" and R.route(2, 0, 0, 8192, 720, 120)["family"] == "skinny"
    assert R.route(0, 0, 1, 8192, 720, 120)["family"] == "skinny" and R.route(0, 0, 0, 8192, 720, 120, p5_B=8)["family"] == "skinny"
    assert R.route(0, 0, 0, 8192, 720, 64)["family"] == "skinny" and R.route(4, 0, 0, 8192, 720, 64)["family"] == "slab"
    assert (R.route(4, 0, 0, 64, 256, 100)["dzk"], R.route(4, 0, 0, 64, 256, 100, dz_out=False)["dzk"], R.route(4, 0, 0, 40, 256, 100)["dzk"]) == (1, 2, 2)
    # slots: cdiv(M, 64) > 128 with a workspace; the slab kernel leaves a slotted launch to the LDS kernels
    assert R.route(0, 0, 0, 8193, 24, 40, xs=True, ws_slots=64)["slotted"] and not R.route(0, 0, 0, 8192, 24, 40, xs=True, ws_slots=64)["slotted"]
    assert not R.route(0, 0, 0, 8193, 24, 40, xs=True)["slotted"] and not R.route(0, 0, 0, 8193, 24, 40, ws_slots=64)["slotted"]
    assert R.route(0, 0, 0, 8200, 256, 68, xs=True, ws_slots=64)["family"] == "skinny" and R.route(0, 0, 0, 8200, 256, 68, xs=True)["family"] == "slab"
    assert (R.route(0, 0, 0, 256, 24, 40, p5_B=2)["p5"], R.route(0, 0, 0, 300, 24, 40, p5_B=4)["p5"], R.route(0, 0, 0, 256, 24, 40)["p5"]) == ("epilogue", "standalone", None)
