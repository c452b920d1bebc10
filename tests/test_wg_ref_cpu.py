"""CPU checks of tests/wg_ref.py, the float64 reference of the 1x1-conv weight-gradient kernels (csrc/pw_wgrad_grouped.hip, pw_wgrad_kernel in
pw_gemm.hip):
  1. the reference against a naive formula written independently with explicit Python loops, in every prologue and BatchNorm-operand mode;
  2. the tolerance constants K of wg_ref are calibrated here, on the CPU models its docstring describes, on every layer and case the GPU test
     runs: the stored K32 is the measured one to within 5 % + 0.01 (not compared below 2, where the floor K = 8 decides), no model exceeds
     K / 4, and K = max(8, ceil(4 * K32));
  3. through the copies of the two host planners (wg_ref.plan / describe, per_layer_plan) the tables reach every branch the GPU test exists
     for, and the copies reproduce values worked out by hand from the source."""
import functools
import math

import pytest
import torch

import wg_ref as W
from elt_ref import ratio, U

D, S32 = torch.float64, torch.float32


# ------------------------------------------------------------------------------------------------ 1. the reference
def _sig(u):
    return 1.0 / (1.0 + math.exp(-u))


NAIVE = (21, 12, 8, "", 3)          # three images of 7 rows (BN_RPI = 7 as well)


@pytest.mark.parametrize("flags", W.PL_MODES)
@pytest.mark.parametrize("bn_mode", [None] + W.BN_MODES)
def test_reference_matches_a_naive_formula(flags, bn_mode):
    M, K, N, _, B = NAIVE
    rpi = M // B
    inp = W.to(W.layer_inputs(0, *NAIVE), D)
    bn = W.to(W.bn_layer_inputs(M, N), D) if bn_mode else None
    got = W.layer_ref(NAIVE, inp, bn=bn, bn_mode=bn_mode, flags=flags, with_dw0=True)
    L = {k: v.tolist() for k, v in inp.items()}
    a = [[0.0] * K for _ in range(M)]
    for m in range(M):
        for k in range(K):
            v = L["x"][m][k]
            if "aff" in flags:
                v = v * L["scale"][k] + L["shift"][k]
                v = v * _sig(v)
            if "gate" in flags:
                v = v * L["gate"][m // rpi][k]
            a[m][k] = v
    d = L["dy"]
    if bn_mode:
        act, mul_b, dsum = bn_mode
        Bn = {k: (v.tolist() if isinstance(v, torch.Tensor) else v) for k, v in bn.items()}
        d = [[0.0] * N for _ in range(M)]
        for m in range(M):
            for n in range(N):
                gp = L["dy"][m][n] * (Bn["mul_b"][m // W.BN_RPI] if mul_b else 1.0)
                if act:
                    u = Bn["z"][m][n] * Bn["scale"][n] + Bn["shift"][n]
                    s = _sig(u)
                    gp = gp * s * (1 + u * (1 - s))
                xhat = (Bn["z"][m][n] - Bn["mean"][n]) * Bn["invstd"][n]
                d[m][n] = Bn["scale"][n] * (gp - Bn["sums"][n] / Bn["count"] - xhat * Bn["sums"][N + n] / Bn["count"])
    want = torch.zeros(N, K, dtype=D)
    for n in range(N):
        for k in range(K):
            s = 0.0
            for m in range(M):
                s += d[m][n] * a[m][k]
            want[n, k] = L["dw0"][n][k] + s
    v, A = got["dw"]
    assert float((v - want).abs().max()) <= 1e-13 * float(A.max())
    assert bool((A >= v.abs() * (1 - 1e-12)).all()) and bool((A > 0).all())
    if bn_mode and bn_mode[2]:
        for out, off, d0 in (("dgamma", N, "dgamma0"), ("dbeta", 0, "dbeta0")):
            v, A = got[out]
            want = torch.tensor([Bn[d0][n] + Bn["sums"][off + n] for n in range(N)], dtype=D)
            assert float((v - want).abs().max()) <= 1e-13 * float(A.max())
            assert bool((A >= v.abs() * (1 - 1e-12)).all()) and bool((A > 0).all())
    else:
        assert set(got) == {"dw"}


def test_kernel_order_is_the_same_function():
    """a1*g' + a2*(z - mu) + a3 with a2 = -a1*invstd*m2, a3 = -a1*m1 is scale*(g' - m1 - xhat*m2)"""
    M, K, N, _, B = NAIVE
    inp, bn = W.to(W.layer_inputs(0, *NAIVE), D), W.to(W.bn_layer_inputs(M, N), D)
    for mode in W.BN_MODES:
        (a, A), (b, _) = (W.layer_ref(NAIVE, inp, bn=bn, bn_mode=mode, kernel_order=o)["dw"] for o in (False, True))
        assert float(((a - b).abs() / A).max()) <= 1e-14


def test_sequential_chain_over_rows():
    g = W.rng(43)
    d, a = torch.randn(13, 5, generator=g), torch.randn(13, 7, generator=g)
    acc = torch.zeros((), dtype=S32)
    for m in range(13):
        acc = acc + d[m, 2] * a[m, 3]
    assert float(W.seq_rows(d, a)[2, 3]) == float(acc)
    assert float((W.seq_rows(d.double(), a.double()) - d.double().t() @ a.double()).abs().max()) <= 1e-13


# ------------------------------------------------------------------------------------------------ 2. calibration of K
def _table_layers():
    for t in W.WG_TABLES:
        for i, layer in enumerate(t["layers"]):
            yield t["name"], i, layer


@functools.lru_cache(maxsize=None)
def _k32():
    """K32 per family over every layer of WG_TABLES and every (case, mode) of PER_LAYER_CASES, where each family's worst sits, and the smallest
    A met"""
    k32 = {f: (0.0, "") for f in W.K_BY_FAMILY}
    a_min = [float("inf")]

    def take(family, where, model, r64, outs):
        for out in outs:
            v, A = r64[out]
            a_min[0] = min(a_min[0], float(A.min()))
            r = ratio(model[out][0], v, A) * (U / W.UNIT[family])
            if r > k32[family][0]:
                k32[family] = (r, where)

    for name, i, layer in _table_layers():
        inp = W.layer_inputs(i, *layer)
        d64, d32 = W.to(inp, D), W.to(inp, S32)
        r64 = W.layer_ref(layer, d64)
        where = "%s[%d] %s" % (name, i, layer[:4])
        take("dw", where, W.layer_ref(layer, d32, dot=W.seq_rows), r64, ["dw"])
        take("dw_bf16", where, W.layer_ref(layer, d32, bf16=True), r64, ["dw"])
    for ci, case in enumerate(W.PER_LAYER_CASES):
        M, K, N, B = case
        layer = (M, K, N, "", B)
        inp, bn = W.layer_inputs(ci, *layer), W.bn_layer_inputs(M, N)
        d64, d32, b64, b32 = W.to(inp, D), W.to(inp, S32), W.to(bn, D), W.to(bn, S32)
        plain, bnm = W.per_layer_modes()
        for flags in plain:
            r64 = W.layer_ref(layer, d64, flags=flags, with_dw0=True)
            where = "per-layer %s [%s]" % (case, flags)
            take("dw", where, W.layer_ref(layer, d32, flags=flags, with_dw0=True, dot=W.seq_rows), r64, ["dw"])
            take("dw_bf16", where, W.layer_ref(layer, d32, flags=flags, with_dw0=True, bf16=True), r64, ["dw"])
        for flags, mode in bnm:
            r64 = W.layer_ref(layer, d64, bn=b64, bn_mode=mode, flags=flags, with_dw0=True)
            where = "per-layer bn %s [%s] %s" % (case, flags, mode)
            m32 = W.layer_ref(layer, d32, bn=b32, bn_mode=mode, flags=flags, with_dw0=True, dot=W.seq_rows, kernel_order=True)
            take("dw_bn", where, m32, r64, ["dw"])
            take("dw_bn_bf16", where, W.layer_ref(layer, d32, bn=b32, bn_mode=mode, flags=flags, with_dw0=True, bf16=True, kernel_order=True), r64, ["dw"])
            if mode[2]:
                take("dsum", where, m32, r64, ["dgamma", "dbeta"])
    return k32, a_min[0]


@pytest.mark.parametrize("family", sorted(W.K_BY_FAMILY))
def test_stored_constant_is_the_calibrated_one(family):
    """K = max(8, ceil(4 * K32)), K32 measured here on the CPU models; nothing of it comes from the kernels"""
    k32, where = _k32()[0][family]
    K = W.K_BY_FAMILY[family]
    print("WG K32 %-10s %.3f  (K %.1f, unit 2^%d)  worst at %s" % (family, k32, K, -9 if family.endswith("bf16") else -24, where))
    if max(k32, W.K32[family]) >= 2.0:          # (below 2 the floor K = 8 decides, and the last digits of K32 - one ulp of the CPU's fp32 sigmoid - do not matter)
        assert abs(W.K32[family] - k32) <= 0.05 * k32 + 0.01, "the K32 recorded in wg_ref.py is not the one measured"
    assert K == max(8.0, float(-(-4 * W.K32[family] // 1))), "K is not max(8, ceil(4 * K32))"
    assert k32 <= K / 4 or K == 8.0 and k32 <= 2.0


def test_inputs_are_well_conditioned():
    """no output element with A == 0; exactly one eight-decade layer per table that has one"""
    assert _k32()[1] > 0
    for name in ("tails", "rows32"):
        wide = [(i, l) for i, l in enumerate(W.TABLE[name]["layers"]) if "wide" in l[3]]
        assert len(wide) == 1
        inp = W.layer_inputs(wide[0][0], *wide[0][1])          # the tensors the GPU test uses: drawn with the layer's own index
        assert float(inp["x"].abs().max() / inp["x"].abs().min()) > 1e8 and float(inp["dy"].abs().max() / inp["dy"].abs().min()) > 1e8


# ------------------------------------------------------------------------------------------------ 3. coverage
def _described():
    out = []
    for t in W.WG_TABLES:
        lps = W.plan(t["layers"], t["rows_per_item"])[0]
        out += [(t, lp, W.describe(lp)) for lp in lps]
    return out


def test_tables_are_legal():
    for t in W.WG_TABLES:
        assert t["grids"] == (1, 7, 64, 100, 0)
        for M, K, N, flags, B in t["layers"]:
            assert K % 4 == 0 and N % 4 == 0 and M > 0 and B == W.cdiv(M, W.cdiv(M, B))
            assert 1 not in t["rows32"] or M % 32 == 0, "a rows32 launch promises that every M is a multiple of 32"
        assert all(0 < p <= len(t["layers"]) <= W.GW_MAXL for p in t["prefixes"])
    assert W.TABLE["tails"]["rows32"] == (0,) and any(l[0] % 32 for l in W.TABLE["tails"]["layers"])
    assert W.TABLE["many"]["prefixes"] == (255, 256, 512) and len(W.TABLE["many"]["layers"]) == 512


def test_tables_reach_every_branch():
    recs = _described()
    missing = []

    def need(what, pred):
        if not any(pred(t, lp, d) for t, lp, d in recs):
            missing.append(what)

    need("thin tile", lambda t, lp, d: not d["wide"])
    need("wide tile", lambda t, lp, d: d["wide"])
    for nu in (0, 1, 2):
        for nv in (0, 1):
            need("row loop of a wave with (nu, nv) = (%d, %d)" % (nu, nv), lambda t, lp, d: (nu, nv) in d["insts"])
            for r32 in (0, 1):
                need("(nu, nv) = (%d, %d) with rows32 = %d" % (nu, nv, r32), lambda t, lp, d: (nu, nv) in d["insts"] and r32 in t["rows32"])
    need("a block mixing a zero-sub-tile wave with a two-sub-tile wave", lambda t, lp, d: d["mixed_0_2"])
    need("a last N tile of 4 columns on a wide layer", lambda t, lp, d: d["wide"] and lp["N"] % 128 == 4)
    need("a thin tile whose second sub-tile has 4 live columns", lambda t, lp, d: not d["wide"] and lp["N"] == 36)
    need("N in 65..96", lambda t, lp, d: 65 <= lp["N"] <= 96)
    need("K <= 32 with N > 64", lambda t, lp, d: lp["K"] <= 32 and lp["N"] > 64)
    need("nsplit 1", lambda t, lp, d: lp["nsplit"] == 1)
    need("nsplit 8", lambda t, lp, d: lp["nsplit"] == 8)
    need("nsplit 8n + r", lambda t, lp, d: d["rounds8"] >= 1 and d["rem8"] > 0)
    need("two fold rounds of 8 and a remainder", lambda t, lp, d: d["rounds8"] == 2 and d["rem8"] > 0)
    need("the fold's second half with a remainder round", lambda t, lp, d: d["second_half"] and d["rounds8"] >= 1 and d["rem8"] > 0)
    need("the fold's second half without a remainder round", lambda t, lp, d: d["second_half"] and d["rounds8"] >= 1 and d["rem8"] == 0)
    need("the fold's first half alone, rounds and remainder", lambda t, lp, d: not d["second_half"] and d["rounds8"] >= 1 and d["rem8"] > 0)
    need("a row tail on the last split", lambda t, lp, d: d["row_tail"] != 0 and lp["nsplit"] > 1)
    need("a row tail of 1", lambda t, lp, d: d["row_tail"] == 1)
    need("gate boundaries inside a step, masked path", lambda t, lp, d: d["inside_step"] > 0 and 0 in t["rows32"] and lp["rpi"] >= 32)
    need("gate boundaries inside a step, R32 path", lambda t, lp, d: d["inside_step"] > 0 and 1 in t["rows32"] and lp["rpi"] >= 32)
    need("rows_per_image < 32, masked path", lambda t, lp, d: lp["gate"] and lp["rpi"] < 32 and 0 in t["rows32"])
    need("rows_per_image < 32, R32 path", lambda t, lp, d: lp["gate"] and lp["rpi"] < 32 and 1 in t["rows32"])
    for r32 in (0, 1):
        for w in (False, True):
            need("a carried gate image index, rows32 = %d, wide %d" % (r32, w), lambda t, lp, d: d["carried"] > 0 and d["wide"] == w and r32 in t["rows32"])
        need("a gate image index carried over two images in one step, rows32 = %d" % r32, lambda t, lp, d: d["carried2"] > 0 and r32 in t["rows32"])
    need("a ragged last image", lambda t, lp, d: lp["gate"] and lp["M"] % lp["rpi"])
    need("a gated layer with a prologue", lambda t, lp, d: lp["gate"] and any(l[3] == "aff gate" and l[:3] == (lp["M"], lp["K"], lp["N"]) for l in t["layers"]))
    assert not missing, missing
    # the layer-count limits: the split kernel's (255) on both sides, the planner's (512) reached
    assert W.GW_MAXL3 in W.TABLE["many"]["prefixes"] and W.GW_MAXL3 + 1 in W.TABLE["many"]["prefixes"] and W.GW_MAXL in W.TABLE["many"]["prefixes"]
    # grid sizes: one persistent block, fewer blocks than an XCD group, exactly one group of 64, a group and a trailing partial one, the default
    for t in W.WG_TABLES:
        n_items = W.plan(t["layers"][:min(t["prefixes"])], t["rows_per_item"])[1]
        # every grid of GRIDS is below n_items, none is clamped but the default (the small `steps` table: 7 < n_items < 64)
        assert n_items > (7 if t["name"] == "steps" else 100), (t["name"], n_items)


def test_plan_matches_hand_values():
    """worked out by hand from mmd_wgrad_plan"""
    lps, items, tiles, ws = W.plan([(608, 24, 144, "gate", 87), (33, 68, 36, "", 1)], 32)
    a, b = lps
    # N = 144 > 64: 128-wide tiles, 2 x 1 of them; rows per item max(32 / 2, 32) = 32 -> 19 splits of 32 rows; 38 items of 128 * 64 floats
    assert [a[f] for f in W.PLAN_FIELDS] == [128, 2, 1, 32, 19, 0, 0, 0]
    # N = 36: 64-wide, 1 x 2 tiles; cdiv(33, 32) = 2 splits -> mchunk = cdiv(17, 32) * 32 = 32, nsplit 2; behind layer 0's 38 items / 2 tiles
    assert [b[f] for f in W.PLAN_FIELDS] == [64, 1, 2, 32, 2, 38, 2, 38 * 8192]
    assert (items, tiles, ws) == (38 + 4, 2 + 2, 38 * 8192 + 4 * 4096)
    # the engine's rows per item on a layer of test_wgrad_grouped_matches_torch_and_is_deterministic: 2048 rows per wide item -> 20 splits,
    # mchunk = cdiv(2000, 32) * 32 = 2016
    (c,), items, tiles, ws = W.plan([(40000, 24, 144, "", 2)], 4096)
    assert (c["pad_"], c["mchunk"], c["nsplit"], items, tiles, ws) == (128, 2016, 20, 40, 2, 40 * 8192)
    # rows_per_item below a step is raised to 32
    assert W.plan([(100, 8, 8, "", 1)], 1)[0][0]["mchunk"] == 32
    # (96, 40, 24) in images of 16 rows at 64 rows per item: items of 64 and 32 rows; the one second step carries rows 32.. from image 0 / 1 to 2 / 3
    e = W.describe(W.plan([(96, 40, 24, "gate", 6)], 64)[0][0])
    assert (e["carried"], e["carried2"], e["inside_step"]) == (1, 1, 3)
    assert W.describe(a)["carried"] == 0          # one-step items: nothing is carried
    d = W.describe(a)
    assert d["wide"] and (d["rounds8"], d["rem8"]) == (2, 3) and d["inside_step"] == sum(1 for r in range(7, 608, 7) if r % 32)
    # N = 144: tile 0 has two live sub-tiles in both wave rows; tile 1 (columns 128..143) one in wn = 0, none in wn = 1; K = 24: wk = 1 idle
    assert d["tiles"] == [((2, 1), (2, 0), (2, 1), (2, 0)), ((1, 1), (1, 0), (0, 1), (0, 0))] and d["mixed_0_2"]
    d = W.describe(b)
    assert d["tiles"] == [((1, 1), (1, 1), (1, 1), (1, 1)), ((1, 1), (1, 0), (1, 1), (1, 0))] and (d["row_tail"], d["last_rows"]) == (1, 1)


def test_per_layer_plan():
    """both sides of M = 8192, a padded grid, idle waves (worked out by hand from pw_wgrad_impl)"""
    p = W.per_layer_plan(8192, 8, 8)
    assert (p["mchunk"], p["splits"], p["nblk"], p["grid"]) == (64, 128, 128, 128)
    p = W.per_layer_plan(8224, 8, 8)          # cdiv(8224, 256) = 33 splits -> mchunk = cdiv(250, 32) * 32 = 256
    assert (p["mchunk"], p["splits"], p["nblk"], p["grid"]) == (256, 33, 33, 40)
    p = W.per_layer_plan(200, 8, 8)
    assert (p["mchunk"], p["splits"]) == (64, 4)
    p = W.per_layer_plan(100, 68, 132)        # 3 x 2 tiles, 2 splits of 64 rows
    assert (p["ntn"], p["ntk"], p["splits"], p["nblk"], p["grid"]) == (3, 2, 2, 12, 16)
    p = W.per_layer_plan(300, 32, 100)
    assert p["idle_waves"] == {(0, 1), (1, 1)} and p["row_tail"] == 12
    plans = [W.per_layer_plan(M, K, N) for M, K, N, _ in W.PER_LAYER_CASES]
    assert any(q["nblk"] % 8 for q in plans) and any(q["nblk"] % 8 == 0 for q in plans) and any(q["nblk"] == 1 for q in plans)
    assert any(q["idle_waves"] for q in plans) and any(q["row_tail"] == 1 for q in plans) and any(q["splits"] == 4 for q in plans)
    for M, K, N, B in W.PER_LAYER_CASES:
        assert K % 4 == 0 and N % 4 == 0 and B == W.cdiv(M, W.cdiv(M, B))
    plain, bnm = W.per_layer_modes()          # every case runs the full set: four prologues; each crossed with act x mul_b x dgamma / dbeta
    assert plain == ("", "aff", "gate", "aff gate") and len(bnm) == 32 and len(set(bnm)) == 32
    assert {(f, a, m, s) for f, (a, m, s) in bnm} == {(f, a, m, s) for f in plain for a in (0, 1) for m in (False, True) for s in (False, True)}
    assert W.BN_RPI % 32 and 32 % W.BN_RPI
