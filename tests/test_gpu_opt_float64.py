"""GPU: the training-state kernels of csrc/optim.hip (mmd_adam_step, mmd_adam_step_gated, mmd_opt_step_gated in its three modes,
mmd_clip_grad_norm, mmd_memset_async) against the float64 references of tests/opt_ref.py, through the C ABI, on the case tables
opt_ref.OPT_CASES / CLIP_CASES / MEMSET_CASES (test_opt_ref_cpu.py proves through opt_ref.route_* that every branch is reached, and the
references against torch.optim).

A case is a sequence of steps on carried state; after EVERY step every element of p, m, v and both step states is judged:
|got_i - ref64_i| <= K * 2^-24 * A_i + tiny, A_i the magnitude the reference carries for that element and K the family's constant of
opt_ref (calibrated on the CPU by test_opt_ref_cpu.py, never on these kernels).  What must not move is compared bit for bit: a gated-off
head's p / m / v and step state, an inactive segment, v under SGD (NaN on entry), m under SGD without momentum, a gradient below max_norm,
the bytes around a memset.  Every buffer lies in front of 16 guard rows of a sentinel that must survive; the clip workspace is exactly one
double holding garbage on entry.  Each check prints `OPT64 <family> <case> <worst err / (2^-24 A)> (K)` before it asserts.  The float64
references run in torch (nothing of the library under test).

Float64 suites of this shape: see the list in test_gpu_kd_float64.py."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from mm_distillnet_amd import _lib

import opt_ref as R

call = _lib.call
DEV = "cuda"
D = torch.float64


class Out:
    """a buffer of `shape` followed by 16 guard rows of the sentinel, holding `fill` (a CPU tensor) on entry"""

    def __init__(self, shape, fill, dtype=torch.float32):
        self.n = math.prod(shape)
        self.buf = torch.full((self.n + 16 * shape[-1],), R.SENTINEL, dtype=dtype, device=DEV)
        self.t = self.buf[:self.n].view(shape)
        self.t.copy_(fill.to(dtype).reshape(shape))

    def get(self):
        assert bool((self.buf[self.n:] == R.SENTINEL).all()), "guard rows behind the buffer were written"
        return self.t


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def judge(fam, label, got, value, A):
    K = R.K_BY_FAMILY[fam]
    r = R.ratio(got.reshape(value.shape), value, A)
    print("OPT64 %-6s %-52s %8.3f  (K %.0f)" % (fam, label, r, K))
    assert r <= K, "%s %s: err / (2^-24 A) = %.3f > K = %.1f" % (fam, label, r, K)


class State:
    """p, m, v as [n / 4, 4] buffers (guards: 64 floats), the two step states [4] and the device scalars of one run"""

    def __init__(self, case, inp):
        n = case["n"]
        self.p, self.m, self.v = (Out((n // 4, 4), inp[k]) for k in ("p0", "m0", "v0"))
        self.main, self.head = Out((4,), inp["st_main0"]), Out((4,), inp["st_head0"])
        self.hyper = torch.zeros(6, device=DEV)
        self.act = torch.zeros(1, dtype=torch.int32, device=DEV)

    def snapshot(self):
        return {k: bits(getattr(self, k).get()).clone() for k in ("p", "m", "v", "main", "head")}


def run_step(kind, case, S, stp, g):
    n = case["n"]
    S.hyper.copy_(torch.tensor(stp["hyper"], dtype=torch.float32))
    rg = [x for be in case["ranges"] for x in be]
    if kind == "adam":
        S.act.fill_(stp["active"])
        active = {"null": None, "one": S.act, "zero": S.act}[case["active_arg"]]
        call("mmd_adam_step", S.p.t, g, S.m.t, S.v.t, S.main.t, S.hyper, active, stp["gscale"], n)
        return
    S.act.fill_(stp["head_active"])
    if kind == "adam_gated":
        call("mmd_adam_step_gated", S.p.t, g, S.m.t, S.v.t, S.main.t, S.head.t, S.hyper, S.act, *rg, stp["gscale"], n)
    else:
        call("mmd_opt_step_gated", case["mode"], S.p.t, g, S.m.t, S.v.t, S.main.t, S.head.t, S.hyper, S.act, *rg, stp["gscale"], n)


def check_step(case, S, before, ref, head, stp, label):
    """judge every element of p, m, v and the states against the float64 step; what the step must not touch keeps its bits"""
    n, mode = case["n"], case["mode"]
    now = S.snapshot()
    for k in ("p", "m") + (() if mode == 2 else ("v",)):
        got, ok = getattr(S, k).get().reshape(n), torch.isfinite(ref[k][0]).to(DEV)
        # (an SGD momentum buffer is NaN until its state's first step, which must overwrite it: judged on the elements that have stepped,
        # the others keep their bits)
        assert k == "m" or bool(ok.all())
        assert torch.equal(now[k].reshape(n)[~ok], before[k].reshape(n)[~ok]), "%s %s: an element that has not stepped changed" % (label, k)
        judge(k, "%s %s" % (label, k), got[ok], ref[k][0].to(DEV)[ok], ref[k][1].to(DEV)[ok])
    frozen = torch.zeros(n, dtype=torch.bool)
    if not stp["active"]:
        frozen[:] = True
    elif not stp["head_active"]:
        frozen |= head
    fz = frozen.to(DEV)
    for k in ("p", "m", "v"):
        assert torch.equal(now[k].reshape(n)[fz], before[k].reshape(n)[fz]), "%s %s: a gated-off element changed" % (label, k)
    if mode == 2:
        assert torch.equal(now["v"], before["v"]), label + ": SGD wrote v"
        if stp["hyper"][5] == 0.0:
            assert torch.equal(now["m"], before["m"]), label + ": SGD without momentum wrote m"
    for name, on in (("main", stp["active"]), ("head", stp["active"] and stp["head_active"] and case["entry"] == "gated")):
        st = getattr(S, name).get().cpu()
        if on:
            assert float(st[0]) == ref[name][0], (label, name, float(st[0]), ref[name][0])
            want = torch.tensor(ref[name][1:], dtype=D)
            judge("state", "%s %s" % (label, name), st[1:3], want, want.abs())
            assert float(st[3]) == -7.0
        else:
            assert torch.equal(now[name], before[name]), "%s: the %s state of a gated-off step changed" % (label, name)


@pytest.mark.parametrize("name", R.cases_of("adam"))
def test_adam_step_sequences(name):
    """mmd_adam_step: n = 4, 1020 and the grid-stride second trip; active NULL / 1 / 0 (0: p, m, v and the state keep their bits); three
    steps on carried state from a fresh start and resumed at steps 7 and 1000 with non-zero moments; lr changed between steps;
    grad_scale 0.5; exact-zero, 1e-20 and 1e4 gradients"""
    case = R.CASE[name]
    inp = R.case_inputs(case)
    ref = R.run_sequence(case, inp, D)
    head = R.head_mask(case["n"], case["ranges"])
    S = State(case, inp)
    for s, stp in enumerate(case["steps"]):
        before = S.snapshot()
        run_step("adam", case, S, stp, inp["g"][s].to(DEV))
        check_step(case, S, before, ref[s], head, stp, "%s step %d" % (name, s))
    if case["mode"] == 0:
        z = inp["zero"].to(DEV)
        assert torch.equal(S.p.get().reshape(-1)[z].cpu(), inp["p0"][inp["zero"]]), "an exactly-zero update moved p"


@pytest.mark.parametrize("name", R.cases_of("gated"))
def test_gated_step_sequences(name):
    """mmd_opt_step_gated (Adam / AdamW / SGD with and without momentum) and, in mode 0, mmd_adam_step_gated on the same inputs (bit for
    bit the same): three head ranges - disjoint, adjacent, one empty, one starting at 0, one ending at n, boundaries on float4s that are
    not block-aligned, inside the grid-stride second trip - the head gated off for the first steps (bits kept) and then counting its own
    steps from 1, SGD's first-step rule per state (the momentum buffer of a state that has never stepped is NaN: its first step must
    overwrite it, and it keeps its bits until then), resumed main states, a head state resumed at step 1000 with non-zero moments,
    parameters that are exactly zero (the update judged at its own size), lr changed between steps, grad_scale 0.5"""
    case = R.CASE[name]
    inp = R.case_inputs(case)
    ref = R.run_sequence(case, inp, D)
    head = R.head_mask(case["n"], case["ranges"])
    S = State(case, inp)
    S2 = State(case, inp) if case["mode"] == 0 else None
    for s, stp in enumerate(case["steps"]):
        g = inp["g"][s].to(DEV)
        before = S.snapshot()
        run_step("opt_gated", case, S, stp, g)
        check_step(case, S, before, ref[s], head, stp, "%s step %d" % (name, s))
        if S2 is not None:
            run_step("adam_gated", case, S2, stp, g)
            a, b = S.snapshot(), S2.snapshot()
            for k in a:
                assert torch.equal(a[k], b[k]), "%s step %d: mmd_adam_step_gated and mmd_opt_step_gated mode 0 differ in %s" % (name, s, k)
    if case["mode"] == 0:
        z = inp["zero"].to(DEV)
        assert torch.equal(S.p.get().reshape(-1)[z].cpu(), inp["p0"][inp["zero"]]), "an exactly-zero update moved p"


def test_step_refusals_launch_nothing():
    """n % 4 != 0, a range bound that is no multiple of 4, mode 3: MMD_EINVAL from the host and nothing written"""
    dll = _lib.LIB.load()
    case = R.CASE["gated_disjoint_m0"]
    inp = R.case_inputs(case)
    S = State(case, inp)
    before = S.snapshot()
    g = inp["g"][0].to(DEV)
    S.hyper.copy_(torch.tensor(case["steps"][0]["hyper"], dtype=torch.float32))
    S.act.fill_(1)
    P = lambda o: o.data_ptr()
    base = (P(S.p.t), P(g), P(S.m.t), P(S.v.t), P(S.main.t), P(S.head.t), P(S.hyper), P(S.act))
    ok = (8, 100, 200, 300, 512, 1000)
    assert R.route_step(1018) is None and R.route_step(1020, [(8, 102)]) is None
    assert dll.mmd_adam_step(*base[:5], P(S.hyper), None, 1.0, 1018, None) == -22
    for rg, n, mode in ((ok, 1018, 0), ((8, 102) + ok[2:], 1020, 0), ((6,) + ok[1:], 1020, 1), (ok[:4] + (512, 1001), 1020, 2), (ok, 1020, 3), (ok, 1020, -1)):
        assert dll.mmd_opt_step_gated(mode, *base, *rg, 1.0, n, None) == -22
        if mode in (0, 1, 2):
            assert dll.mmd_adam_step_gated(*base, *rg, 1.0, n, None) == -22
    torch.cuda.synchronize()
    after = S.snapshot()
    assert all(torch.equal(before[k], after[k]) for k in before)


# ------------------------------------------------------------------------------------------------ clip
@pytest.mark.parametrize("n,off,clips", R.CLIP_CASES)
def test_clip_grad_norm(n, off, clips):
    """mmd_clip_grad_norm at n = 1, 1023 and a five-trip sum, on a pointer offset by one float, above max_norm (scaled, judged per element)
    and below it (every bit unchanged); the workspace double - garbage on entry, 8 bytes past a 16-byte boundary when the gradient is
    offset - against the float64 sum of squares within the bound of opt_ref.clip_sumsq_bound"""
    x = R.clip_inputs(n, off, clips)
    S, (want, A), did = R.clip_ref(x, R.CLIP_MAX_NORM, D)
    assert did == clips
    front = torch.full((off,), 3.25)
    gb = Out((n + off, 1), torch.cat([front, x]))
    ws = Out((1 + off,), torch.full((1 + off,), 1e300, dtype=D), D)
    call("mmd_clip_grad_norm", gb.t.reshape(-1)[off:], n, R.CLIP_MAX_NORM, ws.t[off:])
    got, w = gb.get().reshape(-1).cpu(), ws.get().cpu()
    assert bool((got[:off] == 3.25).all()) and bool((w[:off] == 1e300).all()), "written in front of the buffer"
    err, bound = abs(float(w[off]) - S), R.clip_sumsq_bound(n, S)
    print("OPT64 sumsq  n %d off %d: |ws - S| / S = %.3e  (bound %.3e)" % (n, off, err / S, bound / S))
    assert err <= bound
    if clips:
        judge("clip", "n %d off %d" % (n, off), got[off:], want, A)
    else:
        assert torch.equal(bits(got[off:]), bits(x)), "a gradient below max_norm was changed"


# ------------------------------------------------------------------------------------------------ memset
@pytest.mark.parametrize("nbytes,off,value", R.MEMSET_CASES)
def test_memset_async(nbytes, off, value):
    """mmd_memset_async: the zero-fill kernel (16-byte chunks, a byte tail, chunks only, tail only, its grid-stride second trip), the
    hipMemsetAsync path for a start 4 bytes past a 16-byte boundary and for value = 0x5A; every byte inside takes the value, the 64 guard
    bytes on either side keep theirs"""
    buf = torch.full((64 + off + nbytes + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    lo = 64 + off
    buf[lo:lo + nbytes] = 0xFF
    addr = buf.data_ptr() + lo
    assert buf.data_ptr() % 256 == 0
    assert R.route_memset(addr, value, nbytes)[0] == ("kernel" if off == 0 and value == 0 else "hip")
    call("mmd_memset_async", addr, value, nbytes)
    torch.cuda.synchronize()
    assert bool((buf[lo:lo + nbytes] == value).all()), "bytes inside the region were not set"
    assert bool((buf[:lo] == 0xA5).all()) and bool((buf[lo + nbytes:] == 0xA5).all()), "bytes outside the region were written"


def test_memset_refusals():
    dll = _lib.LIB.load()
    buf = torch.zeros(16, dtype=torch.uint8, device=DEV)
    assert dll.mmd_memset_async(None, 0, 16, None) == -22 and dll.mmd_memset_async(buf.data_ptr(), 0, 0, None) == -22
