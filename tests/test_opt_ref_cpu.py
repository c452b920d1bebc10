"""CPU checks of tests/opt_ref.py, the float64 references of the training-state kernels (csrc/optim.hip):
  1. the step references against torch.optim.Adam / AdamW / SGD in float64 on every case of OPT_CASES - carried and resumed state, a
     head parameter without a gradient until it switches on, lr changed between steps, grad_scale - and the clip against
     torch.nn.utils.clip_grad_norm_;
  2. the route_* copies over the case tables reach every branch: one and two grid-stride trips, all three head ranges matched, range
     boundaries on float4s that are not block-aligned, every memset path, the clip's early return and its multi-trip sum;
  3. the conditions on the inputs: exact zeros that make the update exactly 0, gradients near 1e-20 and 1e4 in main and head elements;
  4. the tolerance constants K are calibrated here: the same formulas in fp32 on the CPU stay within K / 4 (K = max(8, 4 * K32))."""
import functools

import pytest
import torch

import opt_ref as R

D, S32 = torch.float64, torch.float32


def same(a, b):
    """bit for bit (NaN included)"""
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def within(got, ref, A, name, rtol=1e-12):
    got, ref, A = got.detach().double(), ref.detach().double(), A.detach().double()
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(ref).all()), name
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(((got - ref).abs() <= rtol * A + 1e-300).all()), "%s: worst %.3e of A" % (name, float(((got - ref).abs() / A.clamp_min(1e-300)).max()))


# ------------------------------------------------------------------------------------------------ 1. references against torch.optim
@pytest.mark.parametrize("name", [c["name"] for c in R.OPT_CASES])
def test_step_references_match_torch_optim(name):
    case = R.CASE[name]
    inp = R.case_inputs(case)
    n, mode = case["n"], case["mode"]
    head = R.head_mask(n, case["ranges"])
    ref = R.run_sequence(case, inp, D)
    par = {"main": torch.nn.Parameter(inp["p0"].double()[~head].clone()), "head": torch.nn.Parameter(inp["p0"].double()[head].clone())}
    h = [R.f32(x) for x in case["steps"][0]["hyper"]]
    groups = [{"params": [par[k]]} for k in ("main", "head")]
    if mode == 0:
        opt = torch.optim.Adam(groups, lr=h[0], betas=(h[1], h[2]), eps=h[3])
    elif mode == 1:
        opt = torch.optim.AdamW(groups, lr=h[0], betas=(h[1], h[2]), eps=h[3], weight_decay=h[4])
    else:
        opt = torch.optim.SGD(groups, lr=h[0], momentum=h[5], weight_decay=h[4])
    for k, t0, sel in (("main", case["step0"], ~head), ("head", case["head_step0"], head)):
        if t0 > 0:                                                           # a resumed state
            if mode == 2:
                opt.state[par[k]] = {"momentum_buffer": inp["m0"].double()[sel].clone()}
            else:
                opt.state[par[k]] = {"step": torch.tensor(float(t0)), "exp_avg": inp["m0"].double()[sel].clone(), "exp_avg_sq": inp["v0"].double()[sel].clone()}
    for s, stp in enumerate(case["steps"]):
        for gr in opt.param_groups:
            gr["lr"] = R.f32(stp["hyper"][0])
        g = inp["g"][s].double() * R.f32(stp["gscale"])
        par["main"].grad = g[~head].clone() if stp["active"] else None
        par["head"].grad = g[head].clone() if stp["active"] and stp["head_active"] else None
        opt.step()
        want = inp["p0"].double().clone()
        want[~head], want[head] = par["main"].detach(), par["head"].detach()
        within(ref[s]["p"][0], want, ref[s]["p"][1], "%s step %d p" % (name, s))
        for k, sel in (("main", ~head), ("head", head)):
            stt = opt.state.get(par[k], {})
            if mode != 2 and "exp_avg" in stt and bool(sel.any()):
                within(ref[s]["m"][0][sel], stt["exp_avg"], ref[s]["m"][1][sel], name + " m")
                within(ref[s]["v"][0][sel], stt["exp_avg_sq"], ref[s]["v"][1][sel], name + " v")
                assert float(stt["step"]) == ref[s][k][0]
            if mode == 2 and stt.get("momentum_buffer") is not None and bool(sel.any()):
                within(ref[s]["m"][0][sel], stt["momentum_buffer"], ref[s]["m"][1][sel], name + " buf")
    # what must not move: a gated-off head, an inactive segment, SGD's v, SGD's m without momentum
    first = ref[0]
    if not case["steps"][0]["active"] or not case["steps"][0]["head_active"]:
        sel = head if case["steps"][0]["active"] else torch.ones(n, dtype=torch.bool)
        for k in ("p", "m"):
            assert same(first[k][0][sel], inp[k + "0"].double()[sel])
    if mode == 2 and case["steps"][0]["hyper"][5] == 0.0:
        assert same(ref[-1]["m"][0], inp["m0"].double())
    if mode == 2:
        assert bool(torch.isnan(ref[-1]["v"][0]).all())
        # the momentum buffer of a state that has never stepped is NaN until its first step, finite on every element from then on
        if case["steps"][0]["hyper"][5] != 0.0:
            for s, stp in enumerate(case["steps"]):
                stepped = (~inp["fresh"]) | (~head if stp["active"] else torch.zeros_like(head)) | (head & bool(any(x["head_active"] for x in case["steps"][:s + 1])))
                assert torch.equal(torch.isfinite(ref[s]["m"][0]), stepped), (name, s)
                assert bool(torch.isfinite(ref[s]["p"][0]).all())


@pytest.mark.parametrize("name", [c["name"] for c in R.OPT_CASES if c["mode"] == 2 and c["steps"][0]["hyper"][5] != 0.0 and
                                  (c["step0"] == 0 or c["head_step0"] == 0)])
def test_sgd_cases_fail_without_the_first_step_rule(name, monkeypatch):
    """every SGD case with momentum and a state that has never stepped holds a state that takes its first step on a NaN buffer: `mom * buf + d` on that step (the rule
    dropped, or `first` read from the other state) leaves NaN in p"""
    case = R.CASE[name]
    inp = R.case_inputs(case)
    assert bool(torch.isnan(inp["m0"][inp["fresh"]]).all()) and bool(inp["fresh"].any())
    real = R.one_step
    monkeypatch.setattr(R, "one_step", lambda mode, X, g, hyper, gscale, step, dt: real(mode, X, g, hyper, gscale, 99, dt))
    broken = R.run_sequence(case, inp, D)
    assert bool(torch.isnan(broken[-1]["p"][0]).any()), name


@pytest.mark.parametrize("n,off,clips", R.CLIP_CASES)
def test_clip_reference_matches_clip_grad_norm(n, off, clips):
    x = R.clip_inputs(n, off, clips)
    S, (y, A), did = R.clip_ref(x, R.CLIP_MAX_NORM, D)
    assert did == clips
    p = torch.nn.Parameter(torch.zeros(n, dtype=D))
    p.grad = x.double().clone()
    tot = torch.nn.utils.clip_grad_norm_([p], R.f32(R.CLIP_MAX_NORM))
    assert abs(float(tot) ** 2 - S) <= 1e-12 * S
    within(y, p.grad, A, "clip", 1e-12)
    if not clips:
        assert torch.equal(y, x.double())
    norm = float(x.double().norm())
    assert (norm > 4 * R.CLIP_MAX_NORM) if clips else (norm < R.CLIP_MAX_NORM / 4)          # far from the coef = 1 boundary


# ------------------------------------------------------------------------------------------------ 2. route coverage
def test_cases_reach_every_branch_of_the_step_kernels():
    trips, matched, unaligned = {"adam": set(), "gated": set()}, [0, 0, 0], 0
    modes, shapes = set(), set()
    for c in R.OPT_CASES:
        r = R.route_step(c["n"], c["ranges"])
        assert r is not None, c["name"]
        blocks, tr, per = r
        trips[c["entry"]].add(tr)
        assert blocks == min(R.cdiv(c["n"] // 4, 256), 2048)
        head = R.head_mask(c["n"], c["ranges"])
        assert int(head.sum()) == 4 * sum(per), c["name"]                       # the ranges of a case never overlap
        for k, (b, e) in enumerate(c["ranges"]):
            matched[k] += per[k] > 0
            assert b % 4 == 0 and e % 4 == 0 and (b % 1024 or b == 0) and (e % 1024 or e == 0)
            unaligned += (b // 4) % 256 != 0 and (e // 4) % 256 != 0
            if c["entry"] == "gated":
                shapes.update([("empty", b == e), ("start0", b == 0 and e > b), ("end_n", e == c["n"] and e > b)])
        if c["entry"] == "gated":
            modes.add((c["mode"], c["steps"][0]["hyper"][5] != 0.0))
            rg = sorted(c["ranges"])
            shapes.add(("adjacent", any(rg[i][1] == rg[i + 1][0] and rg[i][0] < rg[i][1] < rg[i + 1][1] for i in range(2))))
            shapes.add(("disjoint", all(rg[i][1] < rg[i + 1][0] for i in range(2))))
    assert trips == {"adam": {1, 2}, "gated": {1, 2}}
    assert min(matched) >= 5 and unaligned >= 20
    assert modes == {(0, True), (1, True), (2, True), (2, False)}
    assert {k for k, on in shapes if on} == {"empty", "start0", "end_n", "adjacent", "disjoint"}
    # the second trip holds range boundaries: float4s past the first 2048 * 256
    big = R.CASE["gated_big_m0"]
    assert any(b < 2048 * 1024 < e for b, e in big["ranges"]) and R.route_step(big["n"], big["ranges"])[1] == 2
    assert R.route_step(1022) is None and R.route_step(1020, [(2, 8)]) is None and R.route_step(1020, [(4, 10)]) is None
    # sequences: resumed main states (7 and 1000), a head switched on after the main state has stepped, lr changed, grad_scale != 1
    assert {c["step0"] for c in R.OPT_CASES} >= {0, 7, 1000}
    assert any(c["steps"][0]["gscale"] == 0.5 for c in R.OPT_CASES if c["entry"] == "gated") and R.CASE["adam_n1020_resume7"]["steps"][0]["gscale"] == 0.5
    for c in R.OPT_CASES:
        if c["entry"] == "gated" and c["head_step0"] == 0:
            on = [s["head_active"] for s in c["steps"]]
            assert on[0] == 0 and on[-1] == 1 and on == sorted(on), c["name"]
    assert len({s["hyper"][0] for s in R.CASE["gated_disjoint_m0"]["steps"]}) == 2
    assert {c["active_arg"] for c in R.OPT_CASES if c["entry"] == "adam"} == {"null", "one", "zero"}
    # a head state resumed with non-zero moments and stepped; one that is never stepped
    res = [c for c in R.OPT_CASES if c["head_step0"] > 0 and c["steps"][0]["head_active"]]
    assert {c["mode"] for c in res} == {0, 2} and all(c["head_step0"] == 1000 for c in res)
    for c in res:
        inp, head = R.case_inputs(c), R.head_mask(c["n"], c["ranges"])
        assert bool((inp["m0"][head] != 0).any()) and R.run_sequence(c, inp, D)[0]["head"][0] == 1001.0


def test_clip_and_memset_cases_reach_every_path():
    assert {R.route_clip(n) for n, _, _ in R.CLIP_CASES} == {(1, 1), (1, 4), (1024, 5)}      # (blocks, trips)
    assert {(o, c) for _, o, c in R.CLIP_CASES} == {(0, False), (0, True), (1, False), (1, True)}
    paths = {R.route_memset(256 + off, val, nb) for nb, off, val in R.MEMSET_CASES}
    assert ("hip",) in paths
    kern = {p for p in paths if p[0] == "kernel"}
    assert {(p[1] > 0, p[2] > 0) for p in kern} == {(False, True), (True, False), (True, True)}
    assert {p[3] for p in kern} == {1, 2}                                            # the zero-fill kernel's grid-stride second trip
    assert R.route_memset(256 + 4, 0, 64) == ("hip",) and R.route_memset(256, 0x5A, 64) == ("hip",)


# ------------------------------------------------------------------------------------------------ 3. conditions on the inputs
def test_inputs_hold_exact_zero_updates_and_extreme_gradients():
    for c in R.OPT_CASES:
        inp = R.case_inputs(c)
        head = R.head_mask(c["n"], c["ranges"])
        z = inp["zero"]
        g0 = inp["g"][0]
        for sel in (~head, head):
            if int(sel.sum()) >= 1000:
                assert bool((z & sel).any()) and bool(((g0 == 1e-20) & sel).any()) and bool(((g0 == 1e4) & sel).any()), c["name"]
                assert bool(((inp["p0"] == 0) & sel & ~z).any()), c["name"]          # zero parameters that do move: A_p = A_upd
        if c["mode"] == 0:                                                       # (weight decay moves p where the gradient is zero)
            ref = R.run_sequence(c, inp, D)
            assert torch.equal(ref[-1]["p"][0][z], inp["p0"].double()[z]), c["name"]


# ------------------------------------------------------------------------------------------------ 4. calibration of K
@functools.lru_cache(maxsize=None)
def _k32():
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        k32 = {f: (0.0, "") for f in R.K_BY_FAMILY}

        def note(fam, r, where):
            if r > k32[fam][0]:
                k32[fam] = (r, where)
        for case in R.OPT_CASES:
            inp = R.case_inputs(case)
            r64, r32 = R.run_sequence(case, inp, D), R.run_sequence(case, inp, S32)
            for s in range(len(r64)):
                for k in ("p", "m", "v"):
                    if k == "v" and case["mode"] == 2:
                        continue
                    ok = torch.isfinite(r64[s][k][0])                    # (an SGD buffer that has not stepped yet is NaN)
                    note(k, R.ratio(r32[s][k][0][ok], r64[s][k][0][ok], r64[s][k][1][ok]), "%s step %d" % (case["name"], s))
                for st in ("main", "head"):
                    a, b = torch.tensor(r32[s][st][1:], dtype=D), torch.tensor(r64[s][st][1:], dtype=D)
                    note("state", R.ratio(a, b, b.abs()), "%s step %d %s" % (case["name"], s, st))
        for n, off, clips in R.CLIP_CASES:
            x = R.clip_inputs(n, off, clips)
            (y32, _), (y64, A) = R.clip_ref(x, R.CLIP_MAX_NORM, S32)[1], R.clip_ref(x, R.CLIP_MAX_NORM, D)[1]
            note("clip", R.ratio(y32, y64, A), "clip %d %d %d" % (n, off, clips))
        return k32
    finally:
        torch.set_num_threads(threads)


@pytest.mark.parametrize("family", sorted(R.K_BY_FAMILY))
def test_fp32_cpu_evaluation_is_within_a_quarter_of_K(family):
    """K = max(8, 4 * K32): the constant in opt_ref is the one this measurement gives, and the fp32 CPU run stays within K / 4"""
    k32, where = _k32()[family]
    K = R.K_BY_FAMILY[family]
    print("K32 %-10s %.3f  (K %.1f)  worst at %s" % (family, k32, K, where))
    assert k32 <= K / 4
    assert K == 8.0 or K <= 4 * k32 * 1.25 + 1, "K is larger than max(8, 4 * K32) calls for"
    assert abs(R.K32[family] - k32) <= 0.05 * k32 + 0.01, "the K32 recorded in opt_ref.py is not the one measured"


def test_sumsq_bound_is_far_below_fp32():
    for n, _, _ in R.CLIP_CASES:
        assert R.clip_sumsq_bound(n, 1.0) < 2.0 ** -40
