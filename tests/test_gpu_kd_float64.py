"""GPU: the knowledge-distillation kernels of csrc/loss.hip (mmd_mta_attention, mmd_mta_attention_bwd, mmd_mta_kl, mmd_mta_kl_multi in
pairwise and list mode, mmd_at_loss_multi) against the float64 references of tests/kd_ref.py, through the C ABI, on the case table
kd_ref.KD_CASES - one entry per branch of the host and kernel dispatch (test_kd_ref_cpu.py proves through kd_ref.route_* that every branch is
reached, and the references against torch autograd and the golden fixtures).

Every comparison is per element: |got_i - ref64_i| <= K * 2^-24 * A_i + tiny, A_i the magnitude the reference reports for that element
(the argument-dependent error of __expf included, see kd_ref) and K the family's constant of kd_ref (calibrated on the CPU by
test_kd_ref_cpu.py, never on these kernels).  Every output lies in front of 16 guard rows of a sentinel that must survive; it is pre-filled
with NaN where the kernel must overwrite (a, df with accumulate = 0, da in store mode, the AttentionLoss losses and partials) and with
non-zero values where it must accumulate (the MTA loss slots, da with accumulate = 1 / 2 and the multi-teacher pairwise form, df with
accumulate = 1).  Workspaces get exactly their documented size.  Each check prints `KD64 <family> <case> <worst err / (2^-24 A)> (K)`
before it asserts.  The float64 references run on the GPU in torch (nothing of the library under test).

Float64 suites of this shape: test_gpu_elt_float64, test_gpu_dw_float64, test_gpu_bd_float64, test_gpu_pw_float64, test_gpu_wg_float64,
test_gpu_node_float64, test_gpu_mb_float64, test_gpu_pyr_float64, this one and test_gpu_opt_float64."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from mm_distillnet_amd import _lib

import kd_ref as R

call = _lib.call
DEV = "cuda"
D = torch.float64
NAN = "nan"
VP = ctypes.c_void_p


class Out:
    """an output tensor of `shape` followed by 16 guard rows; fill: NAN (must be overwritten) or a CPU tensor (must be accumulated on)"""

    def __init__(self, shape, fill, dtype=torch.float32):
        self.n = math.prod(shape)
        self.buf = torch.full((self.n + 16 * shape[-1],), R.SENTINEL, dtype=dtype, device=DEV)
        self.t = self.buf[:self.n].view(shape)
        if isinstance(fill, str):
            self.t.fill_(float("nan"))
        else:
            self.t.copy_(fill.to(dtype).reshape(shape))

    def get(self):
        assert bool((self.buf[self.n:] == R.SENTINEL).all()), "guard rows behind the output were written"
        return self.t

    def untouched(self):
        return bool(torch.isnan(self.get()).all())


def bits(t):
    return t.contiguous().view(torch.int32)


def judge(case, key, label, got, value, A):
    fam = R.FAMILY[(case["entry"], key)]
    K = R.K_BY_FAMILY[fam]
    r = R.ratio(got.reshape(value.shape), value, A)
    print("KD64 %-8s %-52s %8.3f  (K %.0f)" % (fam, "%s %s" % (case["name"], label), r, K))
    assert r <= K, "%s %s %s: err / (2^-24 A) = %.3f > K = %.1f" % (fam, case["name"], label, r, K)


def setup(name):
    case = R.CASE[name]
    inp = R.case_inputs(case)
    return case, inp, R.to(inp, torch.float32, DEV)


def ptrs(ts):
    return (VP * len(ts))(*[t.data_ptr() for t in ts])


# ------------------------------------------------------------------------------------------------ attention maps
@pytest.mark.parametrize("name", R.cases_of("att"))
def test_attention_forward_and_backward(name):
    """mmd_mta_attention and mmd_mta_attention_bwd (accumulate 0 on NaN, 1 on a non-zero df): one and two float4 trips with full and partial
    waves, partly filled last blocks, p = 2 / 3 / 1 on signed features, 2.5 on positive ones, powf(0, 0) in the p = 1 backward, rows whose
    da is exactly zero, and the pyramid-shaped launch of five levels' rows"""
    case, inp, dev = setup(name)
    rows, C, p = case["rows"], case["C"], case["p"]
    ref = R.case_ref(case, inp, D, DEV)
    a = Out((rows,), NAN)
    call("mmd_mta_attention", dev["f"], a.t, rows, C, p)
    judge(case, "a", "a", a.get(), *ref["a"])
    for acc, key in ((0, "df"), (1, "df_acc")):
        df = Out((rows, C), inp["df0"] if acc else NAN)
        call("mmd_mta_attention_bwd", dev["f"], dev["da"], df.t, rows, C, p, acc)
        judge(case, key, key, df.get(), *ref[key])
        if not acc:
            assert bool((df.get()[dev["da"] == 0] == 0).all()), "a row with da = 0 has a non-zero gradient"


# ------------------------------------------------------------------------------------------------ mmd_mta_kl
@pytest.mark.parametrize("name", R.cases_of("kl"))
def test_mta_kl_every_accumulate_mode(name):
    """mmd_mta_kl with one, two and three teacher maps at HW = 1 ... 1000, B = 1 and 3, T = 9 / 1 / 0.05: accumulate 0 (da NaN on entry),
    1 and 2 (on a non-zero da), the loss added to a non-zero slot; da_s = NULL gives, image by image, the same loss bits"""
    case, inp, dev = setup(name)
    B, HW, nt, T, gs = case["B"], case["levels"][0], case["nt"], case["T"], case["gscale"]
    ts = [dev["a_t"][k][0] for k in range(nt)] + [None] * (3 - nt)
    for acc in (0, 1, 2, None):
        ref = R.case_ref(case, inp, D, DEV, start="da0" if acc else None)
        loss = Out((1,), inp["loss0"][:1])
        da = Out((B, HW), inp["da0"][0] if acc else NAN)
        call("mmd_mta_kl", dev["a_s"][0], *ts, nt, B, HW, T, loss.t, None if acc is None else da.t, gs, acc or 0)
        judge(case, "loss", "acc %s loss" % acc, loss.get()[0], *ref["loss"])
        if acc is None:
            assert da.untouched()
        else:
            judge(case, "da", "acc %d da" % acc, da.get(), *ref["da"])
    # da_s = NULL gives the same loss bits as the gradient form.  The B blocks add their terms to the slot with float atomics, so the
    # bits of a whole launch depend on the order the blocks arrive in once three terms (B >= 3, or B = 2 and a non-zero slot) meet:
    # the comparison is made image by image, in one-block launches whose single add has no order
    for b in range(B):
        got = []
        for with_da in (True, False):
            loss, da = Out((1,), inp["loss0"][:1]), Out((1, HW), NAN)
            call("mmd_mta_kl", dev["a_s"][0][b:b + 1], *[t if t is None else t[b:b + 1] for t in ts], nt, 1, HW, T, loss.t,
                 da.t if with_da else None, gs, 0)
            got.append(bits(loss.get()).clone())
            assert with_da or da.untouched()
        assert torch.equal(*got), "image %d: da_s = NULL changes the loss" % b


# ------------------------------------------------------------------------------------------------ mmd_mta_kl_multi
def run_multi(case, inp, dev, start, with_da=True):
    """start: NAN (store mode), "zeros" or "da0" -> (loss Out, [da Out per level])"""
    nlev, nt, B = len(case["levels"]), case["nt"], case["B"]
    loss = Out(((1 if case["list"] else nt) * nlev,), inp["loss0"])
    das = [Out((B, HW), NAN if start == NAN else (torch.zeros(B, HW) if start == "zeros" else inp["da0"][l])) for l, HW in enumerate(case["levels"])]
    call("mmd_mta_kl_multi", ptrs(dev["a_s"]), ptrs([dev["a_t"][k][l] for k in range(nt) for l in range(nlev)]),
         ptrs([d.t for d in das]) if with_da else None, (ctypes.c_int * nlev)(*case["levels"]), nlev, nt, 1 if case["list"] else 0, B, case["T"],
         loss.t, case["gscale"])
    return loss, das


@pytest.mark.parametrize("name", R.cases_of("multi"))
def test_mta_kl_multi_pairwise_and_list(name):
    """mmd_mta_kl_multi: levels of HW = 1 ... 4352 mixed in one launch (the cached body with 1 - 16 register slots in use, the generic body
    above 4096), one teacher (store mode: da NaN on entry) and several (atomics: once on zeros, once on a non-zero start), the list mode
    with 1 - 4 maps (a store), T = 9 / 1 / 0.05, all-zero teacher and student maps, a single-spike image, signed teacher maps; every
    per-pair loss slot on a non-zero start; da_s = NULL leaves da alone and gives the same losses"""
    case, inp, dev = setup(name)
    store = case["list"] or case["nt"] == 1
    for l, HW in enumerate(case["levels"]):
        assert R.route_kl(case["list"], HW, case["nt"])[2] == ("store" if store else "atomic")
    for start in ([NAN] if store else ["zeros", "da0"]):
        ref = R.case_ref(case, inp, D, DEV, start="da0" if start == "da0" else None)
        loss, das = run_multi(case, inp, dev, start)
        judge(case, "loss", "%s loss" % start, loss.get(), *ref["loss"])
        for l, da in enumerate(das):
            judge(case, "da", "%s da[%d] HW %d" % (start, l, case["levels"][l]), da.get(), *ref["da"][l])
    # (the B blocks of a pair add to its slot with float atomics in no fixed order: the losses of the NULL form are judged like the others)
    loss, das = run_multi(case, inp, dev, NAN, with_da=False)
    assert all(d.untouched() for d in das)
    judge(case, "loss", "da_s NULL loss", loss.get(), *R.case_ref(case, inp, D, DEV)["loss"])


# ------------------------------------------------------------------------------------------------ mmd_at_loss_multi
def run_at(case, dev, with_da=True):
    nlev, nt, B = len(case["levels"]), case["nt"], case["B"]
    loss, ws = Out((nt * nlev,), NAN), Out((nt * nlev * B,), NAN)          # the workspace: exactly nt * nlev * B floats
    das = [Out((B, HW), NAN) for HW in case["levels"]]
    call("mmd_at_loss_multi", ptrs(dev["a_s"]), ptrs([dev["a_t"][k][l] for k in range(nt) for l in range(nlev)]),
         ptrs([d.t for d in das]) if with_da else None, (ctypes.c_int * nlev)(*case["levels"]), nlev, nt, B, loss.t, case["gscale"], ws.t)
    return loss, ws, das


@pytest.mark.parametrize("name", R.cases_of("at"))
def test_at_loss_multi_at_the_chunk_boundaries(name):
    """mmd_at_loss_multi at HW = 1, 255, 4096 (one full chunk), 4097 (one element in the second), 8193 (three chunks), 1 - 4 teachers, one and
    five levels, an all-zero student map (the g / 1e-12 branch), an all-zero teacher map, a spike: losses, the per-image partials and da
    (all NaN on entry); two identical launches agree bit for bit; da_s = NULL gives the same loss bits"""
    case, inp, dev = setup(name)
    ref = R.case_ref(case, inp, D, DEV)
    loss, ws, das = run_at(case, dev)
    judge(case, "loss", "loss", loss.get(), *ref["loss"])
    judge(case, "part", "part", ws.get(), *ref["part"])
    for l, da in enumerate(das):
        judge(case, "da", "da[%d] HW %d" % (l, case["levels"][l]), da.get(), *ref["da"][l])
    loss2, ws2, das2 = run_at(case, dev)
    assert torch.equal(bits(loss.get()), bits(loss2.get())) and torch.equal(bits(ws.get()), bits(ws2.get()))
    for a, b in zip(das, das2):
        assert torch.equal(bits(a.get()), bits(b.get())), "two identical launches differ"
    loss3, ws3, das3 = run_at(case, dev, with_da=False)
    assert all(d.untouched() for d in das3) and torch.equal(bits(loss.get()), bits(loss3.get())), "da_s = NULL changes the losses"


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_nothing():
    """C % 4 != 0, nlev 0 and 6, nteachers 0 and 5, T <= 0, a missing teacher pointer: MMD_EINVAL from the host, every output untouched"""
    dll = _lib.LIB.load()
    f = torch.ones(8, 6, device=DEV)
    a, df, da = Out((8,), NAN), Out((8, 6), NAN), torch.ones(8, device=DEV)
    assert R.route_att(8, 6) is None
    assert dll.mmd_mta_attention(f.data_ptr(), a.t.data_ptr(), 8, 6, 2.0, None) == -22
    assert dll.mmd_mta_attention_bwd(f.data_ptr(), da.data_ptr(), df.t.data_ptr(), 8, 6, 2.0, 0, None) == -22
    B, HW = 2, 8
    m = torch.ones(B, HW, device=DEV)
    loss, out, ws = Out((4,), torch.ones(4)), Out((B, HW), NAN), Out((4 * B,), NAN)
    one, hw = ptrs([m]), (ctypes.c_int * 1)(HW)
    four = ptrs([m, m, m, m])
    hole = (VP * 2)(m.data_ptr(), None)
    po = ptrs([out.t])
    for nlev, nt, T, at in ((0, 1, 9.0, one), (6, 1, 9.0, one), (1, 0, 9.0, one), (1, 5, 9.0, four), (1, 1, 0.0, one), (1, 1, -1.0, one), (1, 2, 9.0, hole)):
        assert R.refused_multi(nlev, nt, T) or at is hole
        for lm in (0, 1):
            assert dll.mmd_mta_kl_multi(one, at, po, hw, nlev, nt, lm, B, T, loss.t.data_ptr(), 1.0, None) == -22
        if T > 0:
            assert dll.mmd_at_loss_multi(one, at, po, hw, nlev, nt, B, loss.t.data_ptr(), 1.0, ws.t.data_ptr(), None) == -22
    p = m.data_ptr()
    for nt, T, t1 in ((0, 9.0, p), (4, 9.0, p), (1, 0.0, p), (1, -1.0, p), (2, 9.0, None)):
        assert dll.mmd_mta_kl(p, p, t1, None, nt, B, HW, T, loss.t.data_ptr(), out.t.data_ptr(), 1.0, 0, None) == -22
    assert dll.mmd_mta_kl(p, p, p, None, 3, B, HW, 9.0, loss.t.data_ptr(), out.t.data_ptr(), 1.0, 0, None) == -22      # third teacher missing
    torch.cuda.synchronize()
    assert a.untouched() and df.untouched() and out.untouched() and ws.untouched() and bool((loss.get() == 1).all())
