"""CPU checks of tests/pw_ref.py, the float64 reference of the forward 1x1-conv GEMM entry points (csrc/pw_gemm.hip, pw_rows.hip,
pw_longk.hip):
  1. the reference against a naive formula written independently with explicit loops over the images, and its live coefficients against
     the formula of test_gpu_kernels.py::test_live_bn_matches_finalized / elt_ref.bn_finalize;
  2. the tolerance constants K of pw_ref are calibrated here, on the CPU models its docstring describes, on every (case, mode) the GPU test
     runs: the stored K32 is the measured one and K = max(8, 4 * K32);
  3. PW_CASES reaches, by the copy of the host dispatch in pw_ref.route, every branch the GPU test exists for, and route reproduces values
     worked out by hand from the source."""
import functools
import os

import pytest
import torch

import pw_ref as R
from elt_ref import bn_finalize, swish, ratio, U, EPS      # EPS: 1e-3 as a C float, what mmd_make_bn stores

D, S32 = torch.float64, torch.float32
FORCED = ("f1", "f1n", "f2", "f2n", "f3", "f3n", "bf16")


# ------------------------------------------------------------------------------------------------ 1. the reference
def _act(t, act):
    return t if act == 0 else (swish(t) if act == 1 else torch.sigmoid(t))


@pytest.mark.parametrize("pro,gate,epi", [("plain", False, "0"), ("given", True, "full"), ("live", False, "s"), ("affine", True, "sig"),
                                          ("swish", False, "osc"), ("plain", True, "remap")])
def test_reference_matches_a_naive_formula(pro, gate, epi):
    case = R._c("naive", 21, 12, 8, 3, ["f2"], None, [(pro, gate, epi)], "")
    inp = R.case_inputs(case)
    d = R._to(inp, D, "cpu")
    got = R.case_ref(case, (pro, gate, epi), inp, D)
    aff, act = R.PRO_KINDS[pro]
    e = R.EPI[epi]
    M, K, N, rpi = 21, 12, 8, 7
    if aff == "live":
        mean = d["in_stats"][:K] / d["in_count"]
        var = d["in_stats"][K:] / d["in_count"] - mean * mean
        sc = d["gamma"] / torch.sqrt(var + EPS)
        sh = d["beta"] - mean * sc
    elif aff == "given":
        sc, sh = d["scale"], d["shift"]
    y = torch.zeros(M, N, dtype=D)
    s, q = d["stats0"][:N].clone(), d["stats0"][N:].clone()
    for b in range(case["B"]):
        for i in range(rpi):
            m = b * rpi + i
            for n in range(N):
                raw = d["bias"][n] if e.get("bias") else torch.zeros((), dtype=D)
                for k in range(K):
                    a = d["x"][m, k]
                    if aff:
                        a = a * sc[k] + sh[k]
                    a = _act(a, act)
                    if gate:
                        a = a * d["gate"][b, k]
                    raw = raw + a * d["w"][n, k]
                s[n] += raw
                q[n] += raw * raw
                t = raw * d["osc"][n] + d["osh"][n] if e.get("osc") else raw
                t = _act(t, e.get("act", 0))
                y[m, n] = t + (d["res"][m, n] if e.get("res") else 0)
    yv, yA = got["y"]
    assert float((yv - y).abs().max()) <= 1e-13 * float(yA.max())
    assert bool((yA >= yv.abs() * (1 - 1e-12)).all()) and bool((yA > 0).all())
    if e.get("stats"):
        assert float((got["sum"][0] - s).abs().max()) <= 1e-13 * float(got["sum"][1].max())
        assert float((got["sumsq"][0] - q).abs().max()) <= 1e-13 * float(got["sumsq"][1].max())
    else:
        assert "sum" not in got
    # the remap: image b's rows start y_offset floats into a destination image of y_batch_stride floats
    idx = R.remap_index(M, N, rpi, rpi * N + R.REMAP_SLACK, R.REMAP_OFFSET)
    assert idx[0, 0] == R.REMAP_OFFSET and idx[rpi, 0] == rpi * N + R.REMAP_SLACK + R.REMAP_OFFSET and idx[rpi - 1, N - 1] == R.REMAP_OFFSET + rpi * N - 1
    assert idx.unique().numel() == M * N


def test_live_coefficients_are_the_finalize_formulas():
    g = R.rng(41)
    z = torch.randn(300, 16, generator=g, dtype=D) * 1.7 + 0.3
    gamma, beta = torch.rand(16, generator=g, dtype=D) + 0.5, torch.randn(16, generator=g, dtype=D) * 0.2
    st = torch.cat([z.sum(0), (z * z).sum(0)])
    sc, sh, Ash = R.live_coef(st, 300, gamma, beta)
    v, _ = bn_finalize(st, 300, gamma, beta)
    assert torch.equal(sc, v["scale"]) and torch.equal(sh, v["shift"])
    mean, var = z.mean(0), z.var(0, unbiased=False)
    want = gamma / torch.sqrt(var + EPS)
    assert float((sc - want).abs().max()) <= 1e-12 and float((sh - (beta - mean * want)).abs().max()) <= 1e-12
    assert bool((Ash >= sh.abs()).all())


def test_sequential_chain_is_a_dot_product():
    g = R.rng(42)
    a, w = torch.randn(7, 13, generator=g, dtype=D), torch.randn(5, 13, generator=g, dtype=D)
    assert float((R.seq_dot(a, w) - a @ w.t()).abs().max()) <= 1e-13
    a32, w32 = a.float(), w.float()
    acc = torch.zeros((), dtype=S32)
    for k in range(13):
        acc = acc + a32[3, k] * w32[2, k]
    assert float(R.seq_dot(a32, w32)[3, 2]) == float(acc)


# ------------------------------------------------------------------------------------------------ 2. calibration of K
@functools.lru_cache(maxsize=None)
def _k32():
    """K32 per family over every (case, mode) of PW_CASES, where each family's worst sits, and the smallest A met"""
    k32 = {f: (0.0, "") for f in R.K_BY_FAMILY}
    a_min, op_max = float("inf"), 0.0
    for case in R.PW_CASES:
        for mode in case["modes"]:
            inp = R.inputs_of(case, mode)
            r64 = R.case_ref(case, mode, inp, D)
            a_min = min(a_min, *(float(A.min()) for _, A in r64.values()))
            if mode[0] != "wide":
                op_max = max(op_max, float(inp["x"].abs().max()), float(inp["w"].abs().max()))
            models = [("", R.case_ref(case, mode, inp, S32, dot=R.seq_dot), U)]
            if "bf16" in case["forms"]:
                models.append(("_bf16", R.case_ref(case, mode, inp, S32, bf16=True), R.UB))
            for sfx, r32, unit in models:
                for out in r64:
                    r = ratio(r32[out][0], r64[out][0], r64[out][1]) * (U / unit)
                    if r > k32[out + sfx][0]:
                        k32[out + sfx] = (r, "%s %s" % (case["name"], R.mode_label(mode)))
    return k32, a_min, op_max


@pytest.mark.parametrize("family", sorted(R.K_BY_FAMILY))
def test_stored_constant_is_the_calibrated_one(family):
    """K = max(8, 4 * K32), K32 measured here on the CPU models; nothing of it comes from the kernels"""
    k32, where = _k32()[0][family]
    K = R.K_BY_FAMILY[family]
    print("PW K32 %-10s %.3f  (K %.1f, unit 2^%d)  worst at %s" % (family, k32, K, -9 if family.endswith("bf16") else -24, where))
    if max(k32, R.K32[family]) >= 2.0:          # (below 2 the floor K = 8 decides, and the last digits of K32 - one ulp of the CPU's fp32 sigmoid - do not matter)
        assert abs(R.K32[family] - k32) <= 0.05 * k32 + 0.01, "the K32 recorded in pw_ref.py is not the one measured"
    assert K == max(8.0, float(-(-4 * R.K32[family] // 1))), "K is not max(8, ceil(4 * K32))"
    assert k32 <= K / 4 or K == 8.0 and k32 <= 2.0


def test_inputs_are_well_conditioned():
    """no output element with A == 0; operands of order 1 (outside the eight-decades modes, of which there are two)"""
    _, a_min, op_max = _k32()
    assert a_min > 0 and op_max < 16
    wide = [(c["name"], m) for c in R.PW_CASES for m in c["modes"] if m[0] == "wide"]
    assert len(wide) == 2
    for name, m in wide:
        inp = R.inputs_of(R.CASE[name], m)
        assert float(inp["x"].abs().max() / inp["x"].abs().min()) > 1e8


# ------------------------------------------------------------------------------------------------ 3. coverage
DISPATCH_ENV = ["MMD_SKINNY_K", "MMD_STREAM", "MMD_SKINNY_TILES", "MMD_SQ_TILES", "MMD_SQ_MIN", "MMD_BN32_GAIN", "MMD_NO_LEAN", "MMD_SK_PF2",
                "MMD_SK_BQ_LDS", "MMD_NO_BQ_LDS", "MMD_BQ_LDS_CAP_KB", "MMD_NO_ROWS", "MMD_ROWS_LDS", "MMD_ROWS_ALL", "MMD_ROWS_SMALL",
                "MMD_ROWS_BLK", "MMD_ROWS_ABL", "MMD_NO_LONGK", "MMD_NO_SLAB"]


def test_no_dispatch_override_in_the_environment():
    """the variables pw_dispatch, pw_rows_try, pw_longk_try (and pw_slab_try's switch) read; MMD_MFMA_F32 is the one exception - the GPU test
    passes it on to route"""
    assert not [k for k in DISPATCH_ENV if k in os.environ]


def _recs():
    return [(c, m, f, R.route_mode(c, m, f)) for c in R.PW_CASES for m in c["modes"] for f in c["forms"]]


def test_cases_reach_every_branch():
    recs = _recs()
    missing = []

    def need(what, form=None, mode=None, **want):
        for c, m, f, r in recs:
            if form and f not in form:
                continue
            if mode and not mode(m):
                continue
            if all((v(r.get(k)) if callable(v) else r.get(k) == v) for k, v in want.items()):
                return
        missing.append(what)

    # every (family, variant, nkl, mfma, pro) the three entry points reach
    for variant in (1, 2, 3):
        for nkl in (1, 2, 3, 4):
            for mfma, form in (("f32", ("f2n",)), ("split", ("f2",)), ("bf16", ("bf16",))):
                for pro in (0, 3, 4):
                    need("tiled v%d nkl %d %s PRO %d" % (variant, nkl, mfma, pro), form=form, family="tiled", variant=variant, nkl=nkl, mfma=mfma, pro=pro)
    for variant in (1, 2, 3):
        need("tiled v%d split form with a half-populated 8-wide group" % variant, form=("f2",), family="tiled", variant=variant, mfma="split", half_group=True)
    need("tiled fp32 MFMA without `native` (K < 64)", form=("f2",), family="tiled", mfma="f32")
    for mfma, form in (("f32", ("f2", "f2n")), ("bf16", ("bf16",))):
        for pro in (0, 3, 4):
            need("skinny %s PRO %d" % (mfma, pro), form=form, family="skinny", mfma=mfma, pro=pro)
    for C in (7, 4, 3, 1):
        for nkk in R.ROWS_NKK:
            need("rows <%d,%d>" % (nkk, C), form=("f1",), family="rows", C=C, nkl=nkk, small_slabs=False)
        need("rows C %d with a partial slab" % C, family="rows", C=C, row_tail=lambda t: t != 0)
    for bits in (R.RW_AFF, R.RW_SWISH, R.RW_GATE):
        need("rows mode bit %d" % bits, family="rows", pro=lambda p: p & bits)
    need("rows plain", family="rows", pro=0)
    need("rows small_slabs override", family="rows", small_slabs=True, C=1)
    need("rows more than one panel", family="rows", npanels=lambda n: n > 1)
    need("rows several chunks per panel", family="rows", cpp=lambda n: n > 1)
    need("rows K 16", family="rows", nkl=2)
    need("rows K 128", family="rows", nkl=16)
    need("rows slotted", family="rows", slotted=True)
    need("rows taken by the auto form", form=("auto",), family="rows")
    for pro in (3, 4):
        need("longk PRO %d" % pro, form=("f3",), family="longk", pro=pro)
    for tail in (0, 16, 80):
        need("longk K tail %d" % tail, family="longk", k_tail=tail)
    need("longk K % 8 == 4", family="longk", half_group=True)
    need("longk N 4", family="longk", col_tail=4, nblk=lambda n: n == 3)
    need("longk statistics", family="longk", mode=lambda m: m[2] == "s")
    need("longk taken by the auto form", form=("auto",), family="longk")
    # K % 32 on the tiled and on the skinny kernel; K shorter than the skinny kernel's K split
    for fam in ("tiled", "skinny"):
        have = {c["K"] % 32 for c, m, f, r in recs if r["family"] == fam}
        missing += ["%s K %% 32 = %d" % (fam, k) for k in (4, 8, 12, 16, 20, 24, 28, 0) if k not in have]
    for K in (4, 8):
        if not any(c["K"] == K and r["family"] == "skinny" for c, m, f, r in recs):
            missing.append("skinny K %d" % K)
    # tails, M = 1 and 33
    need("tiled row tail", family="tiled", row_tail=lambda t: t != 0, ntm=lambda n: n > 1)
    need("tiled 128x32 col tail 24", family="tiled", bn=32, col_tail=24)
    need("tiled N % 32 = 4", family="tiled", bn=32, col_tail=4)
    need("tiled N % 64 = 4", family="tiled", bn=64, col_tail=4)
    need("skinny N % 64 = 4", family="skinny", col_tail=4, ntn=2)
    need("skinny row tail 12, col tail 40", family="skinny", row_tail=12, col_tail=40, nblk=10)
    for fam in ("tiled", "skinny"):
        for M in (1, 33):
            if not any(c["M"] == M and r["family"] == fam for c, m, f, r in recs):
                missing.append("%s M %d" % (fam, M))
    # statistics: slotted and direct on one shape
    need("tiled slotted", family="tiled", slotted=True, mode=lambda m: m[2] == "sw")
    need("tiled slotted, whole epilogue", family="tiled", slotted=True, mode=lambda m: m[2] == "fullw")
    if not any(c["name"] == "t2_k96" and m[2] == "s" and not r["slotted"] for c, m, f, r in recs):
        missing.append("direct sums on the slotted shape")
    # non-lean kinds, remap, aliasing
    for kind in ("affine", "live", "swish", "given"):
        for fam in ("tiled", "skinny"):
            need("%s non-lean %s" % (fam, kind), family=fam, pro=0, mode=lambda m, k=kind: m[0] == k)
    for fam in ("tiled", "skinny", "rows"):
        need("%s remap" % fam, family=fam, mode=lambda m: m[2] == "remap")
    for fam in ("tiled", "skinny", "rows", "longk"):
        need("%s output aliasing the residual" % fam, family=fam, mode=lambda m: m[2] == "acc")
    # the split-form switch
    for K, N, mfma in ((60, 64, "f32"), (64, 48, "f32"), (64, 52, "split")):
        if not any(c["K"] == K and c["N"] == N and f == "f2" and r["mfma"] == mfma and r["family"] == "tiled" for c, m, f, r in recs):
            missing.append("split switch K %d N %d" % (K, N))
    # refused launches
    for name, fam in (("rows_refused_k132", "skinny"), ("rows_refused_gate", "skinny"), ("rows_refused_k40", "tiled"), ("lk_refused_k252", "skinny")):
        c = R.CASE[name]
        if any(R.route_mode(c, m, f)["family"] != fam for m in c["modes"] for f in c["forms"]):
            missing.append(name)
    assert not missing, missing
    # every forced form names its family (or, refused, the family it falls through to); nothing lands on the slab kernel; a workspace is
    # passed exactly where it is used
    for c, m, f, r in recs:
        assert r["family"] != "slab", (c["name"], m, f)
        if f in FORCED:
            assert r["family"] == c["fam"], (c["name"], m, f, r)
        assert bool(R.EPI[m[2]].get("ws")) == bool(r["slotted"]), (c["name"], m, f, r)
        assert not (m[1] and r["family"] == "rows" and c["rpi"] % 16) and c["M"] % c["B"] == 0


def test_route_matches_hand_values():
    """the table of the issue (worked out by hand from the source with form 2) and shapes of the existing tests"""
    r = R.route(2, 0, 0, 100, 12, 16)
    assert (r["family"], r["bm"], r["bn"], r["nkl"], r["half_group"], r["mfma"], r["pro"], r["nblk"], r["row_tail"]) == ("tiled", 128, 32, 2, True, "f32", 3, 1, 100)
    r = R.route(2, 0, 0, 300, 24, 40)
    assert (r["family"], r["nblk"], r["row_tail"], r["col_tail"]) == ("skinny", 10, 12, 40)
    r159, r160 = R.route(2, 0, 0, 20352, 32, 64), R.route(2, 0, 0, 20480, 32, 64)
    assert (r159["big_tiles"], r159["family"], r160["big_tiles"], r160["family"], r160["bm"], r160["bn"]) == (159, "skinny", 160, "tiled", 64, 64)
    r = R.route(2, 0, 0, 20480, 96, 64)
    assert (r["bm"], r["bn"], r["nkl"], r["mfma"]) == (64, 64, 4, "split")
    assert R.route(2, 1, 0, 20480, 96, 64)["mfma"] == "f32" and R.route(2, 0, 0, 20480, 96, 64, split_default=False)["mfma"] == "f32"
    r, rb = R.route(2, 0, 0, 25500, 40, 208), R.route(0, 0, 1, 25500, 40, 208)
    assert (r["big_tiles"], r["bm"], r["bn"], rb["bm"], rb["bn"], rb["mfma"]) == (800, 128, 32, 128, 64, "bf16")
    r = R.route(2, 0, 0, 34100, 64, 192)
    assert (r["big_tiles"], r["bm"], r["bn"], r["row_tail"], r["mfma"]) == (801, 128, 64, 52, "split")
    r = R.route(2, 0, 0, 51100, 40, 88)
    assert (r["bm"], r["bn"], r["col_tail"]) == (128, 32, 24)
    assert [R.route(2, 0, 0, 20480, K, N)["mfma"] for K, N in ((60, 64), (64, 48), (64, 52))] == ["f32", "f32", "split"]
    assert [R.route(2, 0, 0, 100, 12, 16, pro=p, gate=g)["pro"] for p, g in (("plain", 0), ("plain", 1), ("affine", 0), ("live", 1), ("swish", 0))] == [3, 4, 0, 0, 0]
    assert R.route(2, 0, 0, 20480, 96, 64, stats=True, ws_slots=64)["slotted"] and not R.route(2, 0, 0, 16384, 96, 64, stats=True, ws_slots=64)["slotted"]
    # test_pwconv_rows_kernel (form 1): every shape of its list is taken by the row-slab kernel
    rows = [(8192, 88, 528, 8, "given", 1, 1, 0), (8192, 120, 720, 8, "plain", 1, 1, 0), (32768, 112, 112, 8, "given", 0, 1, 64),
            (20008, 112, 112, 1, "live", 0, 1, 64), (131072, 24, 144, 8, "plain", 0, 0, 0), (65536, 16, 96, 4, "live", 0, 1, 64),
            (40960, 32, 16, 4, "plain", 0, 0, 0), (2048, 112, 112, 8, "plain", 0, 1, 0), (48, 112, 36, 1, "plain", 0, 0, 0),
            (512, 112, 180, 2, "plain", 0, 0, 0), (1000, 48, 288, 1, "affine", 0, 0, 0), (4096, 96, 24, 4, "plain", 1, 0, 0),
            (2048, 128, 352, 8, "plain", 0, 0, 0), (777, 16, 16, 1, "plain", 0, 1, 0)]
    got = [R.route(1, 0, 0, M, K, N, pro=p, gate=bool(g), stats=bool(s), ws_slots=ws, rpi=M // B) for M, K, N, B, p, g, s, ws in rows]
    assert [r["family"] for r in got] == ["rows"] * len(rows)
    assert (got[8]["C"], got[8]["small_slabs"]) == (1, True) and got[2]["C"] == 7 and got[2]["slotted"] and (got[0]["C"], got[0]["cpp"], got[0]["npanels"]) == (3, 6, 2)
    # test_pwconv_longk_kernel (form 3): every shape is taken by the long-K kernel
    lk = [(2048, 1248, 208, 8, 1, 0), (2048, 2112, 352, 8, 1, 0), (8192, 528, 88, 8, 1, 0), (8192, 720, 120, 8, 1, 0), (2048, 1248, 208, 8, 0, 0),
          (2048, 720, 208, 1, 0, 1), (100, 260, 36, 1, 0, 0), (2048, 256, 64, 8, 1, 0), (96, 388, 4, 1, 0, 0)]
    got = [R.route(3, 0, 0, M, K, N, gate=bool(g), stats=bool(s), rpi=M // B) for M, K, N, B, g, s in lk]
    assert [r["family"] for r in got] == ["longk"] * len(lk)
    assert [r["k_tail"] for r in got[2:4]] == [16, 80] and got[6]["half_group"] and got[8]["half_group"]
    # the auto form's filters
    assert R.route(0, 0, 0, 43648, 112, 112)["family"] == "rows" and R.route(0, 0, 0, 43648, 112, 112, stats=True)["family"] == "tiled"
    assert R.route(0, 0, 0, 2048, 1248, 208, gate=True, rpi=256)["family"] == "longk" and R.route(0, 0, 0, 8192, 528, 88)["family"] == "skinny"
    assert R.route(0, 0, 0, 2048, 1248, 352, pro="given")["family"] == "slab"
