"""CPU checks of tests/kd_ref.py, the float64 references of the knowledge-distillation kernels (csrc/loss.hip):
  1. every reference against an independently written torch composite in float64 (F.normalize, F.softmax, torch.xlogy, autograd for every
     gradient) on every case of KD_CASES, and against the reference project's own numbers in tests/golden/loss_mta_* / loss_at_*;
  2. kd_ref.route_* over KD_CASES reaches every branch: cached / generic body, 1 - 16 register slots, 1 - 3 AttentionLoss chunks, store /
     atomic, one and two float4 trips of the attention loop with full and partial waves;
  3. the conditions on the inputs (zero maps, spikes, signed teachers, exact zeros under powf(., 0));
  4. the tolerance constants K are calibrated here: the same formulas in fp32 on the CPU stay within K / 4 (K = max(8, 4 * K32))."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kd_ref as R

D, S32 = torch.float64, torch.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def within(got, ref, A, name, rtol=1e-11):
    got, ref, A = got.detach().double(), ref.detach().double(), A.detach().double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(((got - ref).abs() <= rtol * A + 1e-300).all()), "%s: worst %.3e of A" % (name, float(((got - ref).abs() / A.clamp_min(1e-300)).max()))
    assert bool((A >= got.abs() * (1 - 1e-9)).all()), name + ": A below |value|"


# ------------------------------------------------------------------------------------------------ the composite
def mta_composite(a_s, ts, T):
    ah = F.normalize(a_s, dim=1, eps=R.CLAMP)
    if len(ts) == 1:
        th = F.normalize(ts[0], dim=1, eps=R.CLAMP)
    else:
        q = F.normalize(ts[0], dim=1, eps=R.CLAMP)
        for t in ts[1:]:
            q = q * F.normalize(t, dim=1, eps=R.CLAMP)
        th = F.normalize(q, p=1, dim=1, eps=R.CLAMP)
    u, v = F.softmax(ah / T, dim=1), F.softmax(th / T, dim=1)
    return (torch.xlogy(v, v) - v * u).sum() / a_s.shape[0]


def at_composite(a_s, t):
    d = F.normalize(a_s, dim=1, eps=R.CLAMP) - F.normalize(t, dim=1, eps=R.CLAMP)
    return (d * d).mean(), (d * d).sum(1)


# ------------------------------------------------------------------------------------------------ 1. references against torch
@pytest.mark.parametrize("name", R.cases_of("att"))
def test_attention_references_match_autograd(name):
    case = R.CASE[name]
    d = R.to(R.case_inputs(case), D)
    ref = R.case_ref(case, R.case_inputs(case), D)
    f = d["f"].clone().requires_grad_(True)
    a = f.pow(case["p"]).mean(1)
    a.backward(d["da"])
    within(ref["a"][0], a, ref["a"][1], name + " a")
    within(ref["df"][0], f.grad, ref["df"][1], name + " df")
    within(ref["df_acc"][0], d["df0"] + f.grad, ref["df_acc"][1], name + " df_acc")
    zero_rows = d["da"] == 0
    assert bool(zero_rows.any()) and bool((ref["df"][0][zero_rows] == 0).all()) and bool((ref["df"][1][zero_rows] == 0).all())


@pytest.mark.parametrize("name", R.cases_of("kl", "multi"))
@pytest.mark.parametrize("start", [None, "da0"])
def test_mta_references_match_autograd(name, start):
    case = R.CASE[name]
    inp = R.case_inputs(case)
    d = R.to(inp, D)
    ref = R.case_ref(case, inp, D, start=start)
    nlev, nt, T, gs = len(case["levels"]), case["nt"], R.f32(case["T"]), R.f32(case["gscale"])
    listed = case["list"] or case["entry"] == "kl"
    das = ref["da"] if case["entry"] == "multi" else [ref["da"]]
    for l in range(nlev):
        a = d["a_s"][l].clone().requires_grad_(True)
        groups = [[d["a_t"][k][l] for k in range(nt)]] if listed else [[d["a_t"][k][l]] for k in range(nt)]
        losses = [mta_composite(a, ts, T) for ts in groups]
        (sum(losses) * gs).backward()
        want = a.grad if (start is None or (case["list"] and case["entry"] == "multi")) else d["da0"][l] + a.grad
        within(das[l][0], want, das[l][1], "%s da[%d]" % (name, l))
        for t, ls in enumerate(losses):
            i = t * nlev + l
            lv, lA = (ref["loss"][0][i], ref["loss"][1][i]) if case["entry"] == "multi" else ref["loss"]
            within(lv, d["loss0"][i] + ls, lA, "%s loss[%d]" % (name, i))


@pytest.mark.parametrize("name", R.cases_of("at"))
def test_at_reference_matches_autograd(name):
    case = R.CASE[name]
    inp = R.case_inputs(case)
    d = R.to(inp, D)
    ref = R.case_ref(case, inp, D)
    nlev, nt, B, gs = len(case["levels"]), case["nt"], case["B"], R.f32(case["gscale"])
    for l in range(nlev):
        a = d["a_s"][l].clone().requires_grad_(True)
        tot = 0
        for k in range(nt):
            loss, part = at_composite(a, d["a_t"][k][l])
            i = k * nlev + l
            within(ref["loss"][0][i], loss, ref["loss"][1][i], "%s loss[%d]" % (name, i))
            within(ref["part"][0][i * B:(i + 1) * B], part, ref["part"][1][i * B:(i + 1) * B], "%s part[%d]" % (name, i))
            tot = tot + loss
        (tot * gs).backward()
        within(ref["da"][l][0], a.grad, ref["da"][l][1], "%s da[%d]" % (name, l))


def rows(f):
    return f.permute(0, 2, 3, 1).reshape(-1, f.shape[1]).double()


def unrows(df, f):
    B, C, H, W = f.shape
    return df.view(B, H, W, C).permute(0, 3, 1, 2)


def close_to_golden(got, gold, name):
    """the fixtures are the reference project's fp32 results: the float64 reference agrees to fp32 accuracy"""
    got, gold = got.detach().double().numpy(), np.asarray(gold, dtype=np.float64)
    assert got.shape == gold.shape, name
    assert (np.abs(got - gold) <= 5e-5 * np.abs(gold) + 2e-6 * np.abs(gold).max() + 1e-12).all(), (name, float(np.abs(got - gold).max()))


@pytest.mark.parametrize("name", ["stock", "peaky"])
def test_mta_references_match_the_golden_fixtures(name):
    gold = np.load(os.path.join(GOLDEN, "loss_mta_%s.npz" % name))
    T = float(gold["T"])
    for key, nt in (("pair", 1), ("list", 3)):
        for l in range(5):
            fs = torch.from_numpy(gold["fs%d" % l])
            B = fs.shape[0]
            a_s = R.attention(rows(fs), 2.0)[0].view(B, -1)
            ts = [R.attention(rows(torch.from_numpy(gold["ft%d_%d" % (k, l)])), 2.0)[0].view(B, -1) for k in range(nt)]
            o = R.mta_kl(a_s, ts, T, 1.0, torch.zeros((), dtype=D))
            close_to_golden(o["loss"][0], gold[key][l], "%s %s loss %d" % (name, key, l))
            df = R.attention_bwd(rows(fs), o["da"][0].reshape(-1), 2.0)[0]
            close_to_golden(unrows(df, fs), gold["%s_dfs%d" % (key, l)], "%s %s dfs%d" % (name, key, l))


@pytest.mark.parametrize("name", ["stock", "zero"])
def test_at_reference_matches_the_golden_fixtures(name):
    gold = np.load(os.path.join(GOLDEN, "loss_at_%s.npz" % name))
    fs = [torch.from_numpy(gold["fs%d" % l]) for l in range(5)]
    B = fs[0].shape[0]
    a_s = [R.attention(rows(f), 2.0)[0].view(B, -1) for f in fs]
    a_t = [[R.attention(rows(torch.from_numpy(gold["ft%d_%d" % (k, l)])), 2.0)[0].view(B, -1) for l in range(5)] for k in range(3)]
    o = R.at_multi(a_s, a_t, 1.0)
    close_to_golden(o["loss"][0].view(3, 5), gold["loss"], name + " loss")
    for l in range(5):
        df = R.attention_bwd(rows(fs[l]), o["da"][l][0].reshape(-1), 2.0)[0]
        close_to_golden(unrows(df, fs[l]), gold["dfs%d" % l], "%s dfs%d" % (name, l))


# ------------------------------------------------------------------------------------------------ 2. route coverage
def test_cases_reach_every_branch():
    att = {R.route_att(c["rows"], c["C"]) for c in map(R.CASE.get, R.cases_of("att"))}
    assert {r[2] for r in att} == {1, 2}                                                   # float4 trips
    assert {r[3] for r in att if r[2] == 1} >= {1, 3, 16, 63, 64} and {r[3] for r in att if r[2] == 2} >= {1, 8, 32}      # lanes in the last trip
    assert {r[1] for r in att} >= {1, 4} and max(r[0] for r in att) == 258              # a partly filled last block behind full ones
    assert {c["C"] for c in map(R.CASE.get, R.cases_of("att"))} == {4, 12, 64, 252, 256, 260, 288, 384}
    assert {c["p"] for c in map(R.CASE.get, R.cases_of("att"))} == {1.0, 2.0, 2.5, 3.0}
    bwd = {R.route_att_bwd(c["rows"], c["C"]) for c in map(R.CASE.get, R.cases_of("att"))}
    assert any(b > 1 and last != 256 for b, last in bwd)
    assert R.route_att(5, 6) is None and R.route_att_bwd(5, 6) is None
    pair, lst = set(), set()
    for c in map(R.CASE.get, R.cases_of("multi")):
        assert not R.refused_multi(len(c["levels"]), c["nt"], c["T"], c["B"])
        for HW in c["levels"]:
            (lst if c["list"] else pair).add((HW,) + R.route_kl(c["list"], HW, c["nt"]))
    assert {r[0] for r in pair} == {1, 255, 256, 257, 1024, 4095, 4096, 4097, 4352}
    for how in ("store", "atomic"):
        got = {r[1:3] for r in pair if r[3] == how}
        assert got >= {("cached", 1), ("cached", 2), ("cached", 16), ("generic", 0)}, (how, got)
    assert ("cached", 4, "atomic") in {r[1:] for r in pair} and (4096, "cached", 16, "store") in pair and (4097, "generic", 0, "atomic") in pair
    assert {r[1:] for r in lst} == {("generic", 0, "store")}
    multi = list(map(R.CASE.get, R.cases_of("multi")))
    assert {c["nt"] for c in multi if c["list"]} == {1, 2, 3, 4} and {c["nt"] for c in multi if not c["list"]} == {1, 2, 3}
    assert {len(c["levels"]) for c in multi if not c["list"]} == {1, 2, 3, 5}
    for mode in (True, False):
        assert {c["T"] for c in multi if c["list"] == mode} == {9.0, 1.0, 0.05}
        assert any(set(c["flags"]) == set(R.SPECIAL) for c in multi if c["list"] == mode)
    assert any(c["signed"] and c["list"] for c in multi)
    kl = list(map(R.CASE.get, R.cases_of("kl")))
    assert {(c["levels"][0], c["B"]) for c in kl} >= {(HW, B) for HW in (1, 2, 63, 256, 257, 1000) for B in (1, 3)}
    assert {c["nt"] for c in kl} == {1, 2, 3}
    at = list(map(R.CASE.get, R.cases_of("at")))
    assert {HW for c in at for HW in c["levels"]} == {1, 255, 4096, 4097, 8193}
    assert {R.route_at(HW) for c in at for HW in c["levels"]} == {(1, 1), (1, 16), (2, 1), (3, 1)}
    assert {c["nt"] for c in at} == {1, 2, 3, 4} and {len(c["levels"]) for c in at} == {1, 5}
    assert R.route_at(4096) == (1, 16) and R.route_at(4097) == (2, 1) and R.route_kl(False, 4096, 1)[0] == "cached"
    for nlev, nt, T in ((0, 1, 1.0), (6, 1, 1.0), (1, 0, 1.0), (1, 5, 1.0), (1, 1, 0.0), (1, 1, -1.0)):
        assert R.refused_multi(nlev, nt, T)


# ------------------------------------------------------------------------------------------------ 3. conditions on the inputs
def test_special_images_are_what_they_say():
    n = 0
    for c in R.KD_CASES:
        if c["entry"] == "att":
            f = R.case_inputs(c)["f"]
            if c["kind"] == "positive":
                assert bool((f > 0).all())
            else:
                assert bool((f < 0).any())
            if c["kind"] == "zeros":
                assert c["p"] == 1.0 and bool((f == 0).any())
            continue
        if set(c["flags"]) != set(R.SPECIAL):
            continue
        n += 1
        d = R.case_inputs(c)
        B, nt = c["B"], c["nt"]
        assert B == 3
        for l, HW in enumerate(c["levels"]):
            assert bool((d["a_s"][l][0] == 0).all()) and bool((d["a_t"][nt - 1][l][B - 1] == 0).all())
            assert int((d["a_s"][l][1] != 0).sum()) == 1 and int((d["a_t"][0][l][1] != 0).sum()) == 1
        if c["signed"]:
            assert bool((d["a_t"][0][0] < 0).any())
    assert n >= 5
    d = R.case_inputs(R.CASE["list_signed_nt3"])
    assert all(bool((d["a_t"][k][0] < 0).any()) for k in range(3))
    # the zero student's gradient passes the clamp: it is the clamp's reciprocal times an ordinary number, and A follows it
    c = R.CASE["pair_special_nt1"]
    da, A = R.case_ref(c, R.case_inputs(c), D)["da"][0]
    assert float(da[0].abs().max()) > 1e3 * float(da[2].abs().max()) > 0 and bool((A[0] >= da[0].abs()).all())


# ------------------------------------------------------------------------------------------------ 4. calibration of K
@functools.lru_cache(maxsize=None)
def _k32():
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        k32 = {f: (0.0, "") for f in R.K_BY_FAMILY}
        for case in R.KD_CASES:
            inp = R.case_inputs(case)
            for start in ([None] if case["entry"] in ("att", "at") else [None, "da0"]):
                r64, r32 = R.flat(R.case_ref(case, inp, D, start=start)), R.flat(R.case_ref(case, inp, S32, start=start))
                for (k, label, v64, A), (_, _, v32, _) in zip(r64, r32):
                    fam = R.FAMILY[(case["entry"], k)]
                    r = R.ratio(v32, v64, A)
                    if r > k32[fam][0]:
                        k32[fam] = (r, "%s %s %s" % (case["name"], start, label))
        return k32
    finally:
        torch.set_num_threads(threads)


@pytest.mark.parametrize("family", sorted(R.K_BY_FAMILY))
def test_fp32_cpu_evaluation_is_within_a_quarter_of_K(family):
    """K = max(8, 4 * K32): the constant in kd_ref is the one this measurement gives, and the fp32 CPU run stays within K / 4"""
    k32, where = _k32()[family]
    K = R.K_BY_FAMILY[family]
    print("K32 %-10s %.3f  (K %.1f)  worst at %s" % (family, k32, K, where))
    assert k32 <= K / 4
    assert K == 8.0 or K <= 4 * k32 * 1.25 + 1, "K is larger than max(8, 4 * K32) calls for"
    assert abs(R.K32[family] - k32) <= 0.05 * k32 + 0.01, "the K32 recorded in kd_ref.py is not the one measured"
