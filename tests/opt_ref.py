"""Helper (not a test): float64 restatement of the training-state kernels of csrc/optim.hip - mmd_adam_step, mmd_adam_step_gated,
mmd_opt_step_gated (Adam, AdamW, SGD), mmd_clip_grad_norm, mmd_memset_async - written from the formulas in the comments of optim.hip and the
definitions of torch.optim.Adam / AdamW / SGD, not from the kernels' loops; a copy of the host dispatch (route_*); and the one case table
(OPT_CASES, CLIP_CASES, MEMSET_CASES) that test_opt_ref_cpu.py and test_gpu_opt_float64.py share.

Conventions are those of elt_ref.py and node_ref.py.  Every reference computes in the dtype of its tensor arguments: float64 is the oracle,
float32 the "plain fp32" evaluation that calibrates K.  A case is a SEQUENCE of steps on carried state; the reference carries (value, A) of
p, m, v from step to step, A_i the magnitude of what was summed or multiplied into element i:
    m' = b1 m + (1 - b1) g s                A_m' = b1 A_m + |(1 - b1) g s|
    v' = b2 v + (1 - b2) (g s)^2            A_v' = b2 A_v + (1 - b2) (g s)^2
    den = sqrt(v') c + eps                  A_den = c (sqrt(v') + A_v' / (2 sqrt(v'))) + eps      (A_v' / 2 sqrt(v') dropped where v' = 0)
    upd = ss m' / den                       A_upd = ss (A_m' + |m'| A_den / den) / den
    p'  = p (1 - lr wd) - upd               A_p'  = A_p + A_upd                                   (1 - lr wd: AdamW only)
    SGD: d = g s + wd p, buf' = d on the first step of that state, else mom buf + d, p' = p - lr buf'
         A_d = |g s| + wd A_p,  A_buf' = mom A_buf + A_d,  A_p' = A_p + lr A_buf'
The bias corrections are held as the kernels hold them: a float step count, ss = lr / (1 - b1^t) and c = 1 / sqrt(1 - b2^t) formed in
double and, in the fp32 evaluation, rounded to float; the float64 reference keeps the exact values.  That difference (one rounding each) is
part of what K covers, and the fp32 evaluation shows it.  lr, betas, eps, weight decay, momentum and grad_scale are the C floats the
kernels receive.

Errors are judged per element: |got - ref64| <= K * 2^-24 * A + tiny, K = max(8, 4 * K32) per family, K32 the largest error of the fp32
CPU evaluation over every case in the same unit (test_opt_ref_cpu.py measures it and asserts K32 <= K / 4).  No constant comes from a GPU
run of the kernels.

mmd_clip_grad_norm: the workspace double is sum x^2, accumulated in float64 from exact products (24 + 24 bits fit 53).  Along any path from
a term to the result there are at most trips (the thread's serial loop) + 6 (wave tree) + 3 (four waves) + blocks (the atomics on one
address) float64 additions, each of relative error 2^-53 on a partial sum <= S: |ws - S| <= (trips + 9 + blocks) 2^-53 S.  The float64
torch sum it is compared with is pairwise: 32 more units for any n < 2^32 (clip_sumsq_bound)."""
import functools
import math

import torch

from elt_ref import ratio, rng, SENTINEL, f32, cdiv, U, TINY                                   # noqa: F401

ADAM_BLOCK_CAP, CLIP_BLOCK_CAP, ZERO_BLOCK_CAP = 2048, 1024, 4096      # block caps of the step, sumsq and zero-fill launches

# K per family = max(8, 4 * K32).  K32 as test_opt_ref_cpu.py measures it (fp32 CPU evaluation of these references on every case):
K32 = {"p": 5.415, "m": 4.135, "v": 5.177, "state": 0.742, "clip": 2.099}
K_BY_FAMILY = {"p": 22.0, "m": 17.0, "v": 21.0, "state": 8.0, "clip": 9.0}


# ------------------------------------------------------------------------------------------------ the dispatch, copied
def route_step(n, ranges=None):
    """-> (blocks, grid-stride trips of the busiest thread, float4s per range).  A COPY of the launch arithmetic of mmd_adam_step /
    mmd_adam_step_gated / mmd_opt_step_gated; None: the host refuses (n % 4, a bound that is no multiple of 4)"""
    if n <= 0 or n & 3 or any((b | e) & 3 for b, e in (ranges or [])):
        return None
    n4 = n // 4
    blocks = min(cdiv(n4, 256), ADAM_BLOCK_CAP)
    return blocks, cdiv(n4, blocks * 256), [max(0, (min(e, n) - max(b, 0)) // 4) for b, e in (ranges or [])]


def head_mask(n, ranges):
    """element i belongs to the head iff the first element e0 = 4 * (i // 4) of its float4 lies in one of the ranges [b, e)"""
    e0 = torch.arange(n) // 4 * 4
    mask = torch.zeros(n, dtype=torch.bool)
    for b, e in ranges:
        mask |= (e0 >= b) & (e0 < e)
    return mask


def route_clip(n):
    """-> (blocks, trips of sumsq_kernel's busiest thread)"""
    blocks = min(cdiv(n, 1024), CLIP_BLOCK_CAP)
    return blocks, cdiv(n, blocks * 256)


def route_memset(addr, value, nbytes):
    """-> ("kernel", float4s, tail bytes, grid-stride trips) | ("hip",): mmd_memset_async -> mmd_zero_bytes"""
    if value != 0 or addr & 15:
        return ("hip",)
    return ("kernel", nbytes // 16, nbytes % 16, cdiv(max(nbytes // 16, 1), min(cdiv(max(nbytes // 16, 1), 256), ZERO_BLOCK_CAP) * 256))


def clip_sumsq_bound(n, S):
    blocks, trips = route_clip(n)
    return (trips + 9 + blocks + 32) * 2.0 ** -53 * S


# ------------------------------------------------------------------------------------------------ references
def bias_corrections(step, lr, b1, b2, dt):
    """(ss, c) = (lr / (1 - b1^t), 1 / sqrt(1 - b2^t)) formed in double; rounded to float for the fp32 evaluation, as the kernels store them"""
    ss = lr / (1.0 - b1 ** step)
    c = 1.0 / math.sqrt(1.0 - b2 ** step)
    return (f32(ss), f32(c)) if dt == torch.float32 else (ss, c)


def one_step(mode, X, g, hyper, gscale, step, dt):
    """one update of the elements X = {"p", "m", "v"} -> each (value, A), `step` = the state's count AFTER this step (1 = its first)"""
    lr, b1, b2, eps, wd, mom = hyper
    (p, Ap), (m, Am), (v, Av) = X["p"], X["m"], X["v"]
    gk = g * gscale
    if mode == 2:
        d, Ad = gk + wd * p, gk.abs() + wd * Ap
        if mom != 0.0:
            m, Am = (d, Ad) if step == 1 else (mom * m + d, mom * Am + Ad)
            d, Ad = m, Am
        return {"p": (p - lr * d, Ap + lr * Ad), "m": (m, Am), "v": (v, Av)}
    ss, c = bias_corrections(step, lr, b1, b2, dt)
    if mode == 1:
        p = p * (1.0 - lr * wd)
    m, Am = b1 * m + (1.0 - b1) * gk, b1 * Am + ((1.0 - b1) * gk).abs()
    v, Av = b2 * v + (1.0 - b2) * gk * gk, b2 * Av + (1.0 - b2) * gk * gk
    sq = torch.sqrt(v)
    den = sq * c + eps
    Aden = c * (sq + torch.where(v > 0, Av / (2 * sq.clamp_min(1e-300)), torch.zeros_like(v))) + eps
    upd, Aupd = ss * (m / den), ss * (Am + m.abs() * Aden / den) / den
    return {"p": (p - upd, Ap + Aupd), "m": (m, Am), "v": (v, Av)}


def run_sequence(case, inp, dt):
    """the whole sequence of a case in dtype dt -> list over steps of {"p", "m", "v": (value, A), "main": [t, ss, c], "head": [t, ss, c]}.
    Elements of the head ranges follow the head state and keep everything while head_active = 0 (whole segment: `active`)"""
    n, mode = case["n"], case["mode"]
    head = head_mask(n, case["ranges"])
    X = {k: (inp[k + "0"].to(dt), inp[k + "0"].to(dt).abs()) for k in ("p", "m", "v")}
    t_main, t_head = case["step0"], case["head_step0"]
    st = {"main": [float(t_main), float(inp["st_main0"][1]), float(inp["st_main0"][2])],
          "head": [float(t_head), float(inp["st_head0"][1]), float(inp["st_head0"][2])]}
    out = []
    for s, stp in enumerate(case["steps"]):
        hyper = [f32(x) for x in stp["hyper"]]
        gs = f32(stp["gscale"])
        g = inp["g"][s].to(dt)
        new = {k: (X[k][0].clone(), X[k][1].clone()) for k in X}
        for name, on, sel in (("main", stp["active"], ~head), ("head", stp["active"] and stp["head_active"], head)):
            if not on:
                continue
            t = (t_main if name == "main" else t_head) + 1
            if name == "main":
                t_main = t
            else:
                t_head = t
            st[name] = [float(t)] + list(bias_corrections(t, hyper[0], hyper[1], hyper[2], dt))
            if bool(sel.any()):
                r = one_step(mode, {k: (X[k][0][sel], X[k][1][sel]) for k in X}, g[sel], hyper, gs, t, dt)
                for k in X:
                    new[k][0][sel], new[k][1][sel] = r[k]
        X = new
        out.append({**{k: (X[k][0].clone(), X[k][1].clone()) for k in X}, "main": list(st["main"]), "head": list(st["head"])})
    return out


def clip_ref(x, max_norm, dt):
    """-> (S = sum x^2 in float64, (x', A) in dtype dt, clipped): norm = float(sqrt(S)), coef = max_norm / (norm + 1e-6), x' = x * coef
    where coef < 1"""
    S = float((x.double() * x.double()).sum())
    norm = f32(math.sqrt(S)) if dt == torch.float32 else math.sqrt(S)
    mx, e = f32(max_norm), f32(1e-6)
    coef = float(torch.tensor(mx, dtype=dt) / (torch.tensor(norm, dtype=dt) + e))
    xd = x.to(dt)
    if coef >= 1.0:
        return S, (xd, xd.abs()), False
    return S, (xd * coef, (xd * coef).abs()), True


# ------------------------------------------------------------------------------------------------ cases
BIG = 2048 * 256 * 4 + 1028            # the grid-stride second trip of the optimizer kernels
H0 = (1e-3, 0.9, 0.999, 1e-8, 1e-2, 0.9)         # lr, beta1, beta2, eps, weight decay, momentum


def _steps(k, head_on_after=None, lr2=None, gscale=1.0, mom=0.9, wd=1e-2, active=1):
    out = []
    for s in range(k):
        h = list(H0)
        h[4], h[5] = wd, mom
        if lr2 is not None and s >= 2:
            h[0] = lr2                                                     # the scheduler changed lr between steps
        out.append({"hyper": tuple(h), "gscale": gscale, "active": active, "head_active": 0 if head_on_after is None else int(s >= head_on_after)})
    return out


def _c(name, entry, n, mode, steps, ranges=(), step0=0, head_step0=0, active_arg="null", why=""):
    return {"name": name, "entry": entry, "n": n, "mode": mode, "steps": steps, "ranges": list(ranges), "step0": step0,
            "head_step0": head_step0, "active_arg": active_arg, "why": why}


R_DISJOINT = [(8, 100), (200, 300), (512, 1000)]
R_ADJACENT = [(40, 120), (120, 360), (360, 364)]
R_EMPTY = [(16, 16), (100, 204), (600, 900)]
R_START0 = [(0, 44), (400, 404), (700, 720)]
R_END_N = [(4, 8), (500, 508), (1012, 1020)]
R_BIG = [(0, 260), (2048 * 1024 - 4, 2048 * 1024 + 36), (BIG - 520, BIG)]      # the second crosses into the grid-stride second trip


def _cases():
    cs = []
    # ---- mmd_adam_step
    cs.append(_c("adam_n4_fresh", "adam", 4, 0, _steps(3, lr2=5e-4), why="one float4, active NULL, fresh state, lr changed at step 3"))
    cs.append(_c("adam_n1020_resume7", "adam", 1020, 0, _steps(3, lr2=5e-4, gscale=0.5), step0=7, active_arg="one",
                 why="active = 1, resumed at step 7 with non-zero moments, grad_scale 0.5, partial last block"))
    cs.append(_c("adam_big_resume1000", "adam", BIG, 0, _steps(3, lr2=2e-3), step0=1000, why="second grid-stride trip, resumed at step 1000"))
    cs.append(_c("adam_n1020_inactive", "adam", 1020, 0, _steps(2, active=0), step0=7, active_arg="zero", why="active = 0: nothing changes"))
    # ---- gated: every range shape x every mode; the head switches on after two steps
    for tag, rg in (("disjoint", R_DISJOINT), ("adjacent", R_ADJACENT), ("empty", R_EMPTY), ("start0", R_START0), ("end_n", R_END_N)):
        for mode in (0, 1, 2):
            cs.append(_c("gated_%s_m%d" % (tag, mode), "gated", 1020, mode, _steps(4, head_on_after=2, lr2=5e-4, gscale=0.5 if tag == "adjacent" else 1.0),
                         rg, step0=7 if tag in ("disjoint", "end_n") else 0, why="ranges %s, mode %d" % (rg, mode)))
    cs.append(_c("gated_sgd_mom0", "gated", 1020, 2, _steps(4, head_on_after=2, mom=0.0, wd=1e-3), R_DISJOINT, why="SGD without momentum: m keeps its bits"))
    cs.append(_c("gated_sgd_resume", "gated", 1020, 2, _steps(3, head_on_after=1, wd=1e-3), R_ADJACENT, step0=7,
                 why="SGD: main resumed (never a first step), the head's first step when it switches on"))
    cs.append(_c("gated_n4_all_head", "gated", 4, 0, _steps(4, head_on_after=2), [(0, 4), (4, 4), (4, 4)], why="n = 4: the only float4 is head"))
    for mode in (0, 2):
        cs.append(_c("gated_big_m%d" % mode, "gated", BIG, mode, _steps(3, head_on_after=1, lr2=5e-4), R_BIG, step0=1000 if mode == 0 else 0,
                     why="second grid-stride trip with range boundaries inside it"))
    for mode in (0, 2):
        cs.append(_c("gated_head_resume_m%d" % mode, "gated", 1020, mode, _steps(3, head_on_after=0, lr2=5e-4), R_DISJOINT, step0=7, head_step0=1000,
                     why="the head state resumed at step 1000 with non-zero moments and active from the first step"))
    cs.append(_c("gated_head_never_on", "gated", 1020, 1, _steps(3), R_DISJOINT, head_step0=5, why="head never active: its state keeps step 5"))
    return cs


OPT_CASES = _cases()
CASE = {c["name"]: c for c in OPT_CASES}
assert len(CASE) == len(OPT_CASES)


def cases_of(*entries):
    return [c["name"] for c in OPT_CASES if c["entry"] in entries]


def _gen(case):
    n, k = case["n"], len(case["steps"])
    gen = rng(61, n, case["mode"], sum(map(ord, case["name"])) % 997)
    rn = lambda *sh: torch.randn(*sh, generator=gen)
    d = {"p0": rn(n), "g": [rn(n) * 0.01 * (s + 1) for s in range(k)]}
    d["m0"], d["v0"] = rn(n) * 0.01, rn(n).abs() * 1e-4                  # the moments of a resumed state
    head = head_mask(n, case["ranges"])
    idx = torch.arange(n)
    # parameters that are exactly zero, in main and head elements: A_p is then the update's own magnitude, and the update is judged at
    # K * 2^-24 of its size instead of against |p| ~ 1
    d["p0"][idx % 5 == 2] = 0.0
    fresh = torch.zeros(n, dtype=torch.bool)                             # elements of a state that has never stepped: no moments
    if case["step0"] == 0:
        fresh |= ~head
    if case["head_step0"] == 0:
        fresh |= head
    d["m0"][fresh], d["v0"][fresh] = 0.0, 0.0
    # exact zeros where m = v = 0 (the update is exactly 0), tiny and large gradients; spread over main and head elements
    zero = idx % 7 == 3
    d["m0"][zero], d["v0"][zero] = 0.0, 0.0
    for s in range(k):
        d["g"][s][idx % 11 == 5] = 1e-20 * (s + 1)
        d["g"][s][idx % 13 == 6] = 1e4 / (s + 1)
        d["g"][s][zero] = 0.0
    d["zero"] = zero
    if case["mode"] == 2:
        d["v0"] = torch.full((n,), float("nan"))                         # SGD never touches v
        # SGD's first-step rule: buf = d on a state's first step whatever the buffer holds.  The buffer of a state that has never stepped
        # is NaN: mom * buf + d there, or `first` read from the other state, gives NaN.  It keeps its bits until that state steps
        d["m0"][fresh] = float("nan")
    d["fresh"] = fresh
    for name, t in (("st_main0", case["step0"]), ("st_head0", case["head_step0"])):
        d[name] = torch.tensor([float(t), 0.123, 4.56, -7.0])            # [1], [2] are rewritten by a step; [3] is never touched
    return d


@functools.lru_cache(maxsize=None)
def _inputs(name):
    return _gen(CASE[name])


def case_inputs(case):
    """fp32 CPU tensors of one case, the same for the CPU calibration and the GPU test; cached - do not modify"""
    return _inputs(case["name"])


CLIP_CASES = [(n, off, clips) for n in (1, 1023, 1024 * 1024 + 1025) for off in (0, 1) for clips in (False, True)]       # (n, offset in floats, norm above max_norm)
CLIP_MAX_NORM = 10.0


def clip_inputs(n, off, clips):
    """x with ||x|| = 5 * max_norm (clips) or max_norm / 5 (does not): far from the coef = 1 boundary on either side"""
    x = torch.randn(n, generator=rng(62, n, off, clips))
    if n == 1:
        x = x.abs() + 0.5
    x = (x * ((CLIP_MAX_NORM * (5.0 if clips else 0.2)) / float(x.double().norm()))).float()
    return x


MEMSET_BYTES = (1, 15, 16, 17, 4101, 16 * 1024 * 1024 + 55)
MEMSET_CASES = [(nb, off, val) for nb in MEMSET_BYTES for off, val in ((0, 0), (4, 0), (0, 0x5A), (4, 0x5A))]      # (bytes, start offset, value)
