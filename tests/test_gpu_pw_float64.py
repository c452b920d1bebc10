"""GPU: the forward 1x1-conv GEMM entry points of csrc/pw_gemm.hip (mmd_pwconv_fwd, mmd_pwconv_fwd_form with forms 0 - 3 with and without
MMD_PW_FORM_NATIVE, mmd_pwconv_fwd_bf16) against the float64 reference of tests/pw_ref.py, through the C ABI, on the case table
pw_ref.PW_CASES - one entry per branch of the host dispatch (test_pw_ref_cpu.py proves through pw_ref.route that every branch is reached).

Every comparison is per element: |got_i - ref64_i| <= K * unit * A_i + tiny, A_i the magnitude the reference reports for that element, unit
2^-24 (2^-9 for the bf16 entry point) and K the family's constant of pw_ref (calibrated on the CPU by test_pw_ref_cpu.py, never on these
kernels).  y lies in front of 16 guard rows of a sentinel that must survive and is pre-filled with NaN; a remapped destination is
pre-filled with the sentinel throughout, and every element outside the written window must still hold it; the statistics are pre-filled
with non-zero values (the kernels accumulate).  A slot workspace is passed only where pw_ref.route says it is used, must be all zero
afterwards, and the launch must agree with the ws_slots = 0 launch (sums to 1e-12 on the LDS-tiled kernels, y in bits).  A forced form's record must name that family (or, for the refused
launches, the family they fall through to); the split and the native form of one launch must differ in bits; a long-K launch is repeated
three times with the same bits.  Each check prints `PW64 <family> <form> <case> <mode> <worst err / (unit A)> (K)` before it asserts.  The
float64 references run on the GPU in torch (a plain matmul: nothing of the library under test)."""
import os
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from mm_distillnet_amd import _lib

import pw_ref as R
from pw_ref import Out, GPU_ERROR          # the guarded output buffer; the list of GPU errors met by earlier tests

call = _lib.call
DEV = "cuda"
D = torch.float64
FORCED = ("f1", "f1n", "f2", "f2n", "f3", "f3n", "bf16")
SPLIT_DEFAULT = not os.environ.get("MMD_MFMA_F32")


def g(t):
    return None if t is None else t.detach().contiguous().to(DEV)


def judge(family, label, got, ref, A):
    K, unit = R.K_BY_FAMILY[family], R.UNIT[family]
    got = got.double()
    assert got.shape == ref.shape == A.shape, (got.shape, ref.shape, A.shape)
    assert bool(torch.isfinite(got).all()), "%s %s: non-finite output" % (family, label)
    r = float(((got - ref).abs() / (unit * A + R.TINY)).max())
    print("PW64 %-10s %-52s %8.3f  (K %.0f)" % (family, label, r, K))
    assert r <= K, "%s %s: err / (unit A) = %.3f > K = %.1f" % (family, label, r, K)


def launch(case, mode, flabel, dev, inp, rec, use_ws=True):
    """one call of the entry point of `flabel` -> {"y" [M, N], "sum", "sumsq"}, the slot workspace (or None)"""
    entry, form, native, bf16 = R.FORMS[flabel]
    M, K, N, B, rpi = case["M"], case["K"], case["N"], case["B"], case["rpi"]
    pro, gate, epi = mode
    aff, act = R.PRO_KINDS[pro]
    e = R.EPI[epi]
    stride = off = 0
    if e.get("remap"):
        stride, off = rpi * N + R.REMAP_SLACK, R.REMAP_OFFSET
        y = Out((B, stride), "sent")
    else:
        y = Out((M, N), inp["res"] if e.get("acc") else "nan")
    res = None if not e.get("res") else (y.t if e.get("acc") else dev["res"])
    st = Out((2 * N,), inp["stats0"], D) if e.get("stats") else None
    ws = None
    if e.get("ws") and use_ws:
        assert rec["slotted"], "the case passes a workspace the dispatch would not use: %s" % (rec,)
        ws = Out((e["ws"], 2 * N), torch.zeros(e["ws"], 2 * N), D)
    live = aff == "live"
    args = [dev["x"], dev["w"], y.t, M, K, N, dev["scale"] if aff == "given" else None, dev["shift"] if aff == "given" else None, act,
            dev["in_stats"] if live else None, dev["gamma"] if live else None, dev["beta"] if live else None, inp["in_count"] if live else 0,
            dev["gate"] if gate else None, rpi, dev["bias"] if e.get("bias") else None, dev["osc"] if e.get("osc") else None,
            dev["osh"] if e.get("osc") else None, e.get("act", 0), res, st.t if st else None, stride, off,
            ws.t if ws else None, e["ws"] if ws else 0]
    if entry == "mmd_pwconv_fwd_form":
        args += [None, 0, form | (R.MMD_PW_FORM_NATIVE if native else 0)]
    call(entry, *args)
    torch.cuda.synchronize()
    if e.get("remap"):
        flat = y.get().reshape(-1)
        idx = R.remap_index(M, N, rpi, stride, off, DEV)
        outside = torch.ones(flat.numel(), dtype=torch.bool, device=DEV)
        outside[idx.reshape(-1)] = False
        assert int(outside.sum()) == flat.numel() - M * N
        assert bool((flat[outside] == R.SENTINEL).all()), "the remapped launch wrote outside its window"
        got = {"y": flat[idx]}
    else:
        got = {"y": y.get()}
    if st:
        got["sum"], got["sumsq"] = st.get()[:N], st.get()[N:]
    return got, ws


def run_case(name, flabel):
    assert not GPU_ERROR, "an earlier test hit a GPU error (%s): not launching anything more" % GPU_ERROR[0]
    try:
        _run_case(name, flabel)
    except RuntimeError as e:
        GPU_ERROR.append("%s %s: %s" % (flabel, name, str(e)[:200]))
        raise


def _run_case(name, flabel):
    case = R.CASE[name]
    bf16 = R.FORMS[flabel][3]
    t0 = time.time()
    for mode in case["modes"]:
        inp = R.inputs_of(case, mode)
        dev = {k: (g(v) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
        rec = R.route_mode(case, mode, flabel, SPLIT_DEFAULT)
        assert rec["family"] != "slab", rec
        if flabel in FORCED:
            assert rec["family"] == case["fam"], "%s %s under %s: the dispatch takes %s" % (name, mode, flabel, rec)
        ref = R.case_ref(case, mode, inp, D, DEV)
        got, ws = launch(case, mode, flabel, dev, inp, rec)
        label = "%-4s %s %s [%s]" % (flabel, name, R.mode_label(mode), rec["family"])
        assert set(got) == set(ref), (sorted(got), sorted(ref))
        for out in got:
            judge(out + ("_bf16" if bf16 else ""), label, got[out], *ref[out])
        if ws is not None:
            assert bool((ws.get() == 0).all()), "the slot workspace is not left zero"
            direct, _ = launch(case, mode, flabel, dev, inp, rec, use_ws=False)
            for out in ("sum", "sumsq"):
                if rec["family"] == "tiled":
                    # a tile's fp32 partial sums are formed in a fixed order whichever copy they are added to: only the order of the float64
                    # atomics differs
                    assert float((got[out] - direct[out]).abs().max()) <= 1e-12 * float(direct[out].abs().max()), "slotted and direct %s differ" % out
                else:
                    # the row-slab kernel deals its slabs over another block count without a workspace (pw_rows.hip: maxblk = 128 * npanels,
                    # pw_ref.route's bpp) and a block adds its waves' fp32 partial sums with LDS atomics, in arrival order: the two launches
                    # differ by fp32 roundings of block partial sums, and each is judged against float64
                    judge(out, label + " direct", direct[out], *ref[out])
            assert torch.equal(got["y"], direct["y"])
        if rec["family"] == "longk":          # a race in the LDS-DMA ring would show as run-to-run differences
            for rep in range(2):
                again, _ = launch(case, mode, flabel, dev, inp, rec)
                assert torch.equal(again["y"], got["y"]), "long-K launch %d differs in bits from the first" % (rep + 2)
        if flabel.endswith("n") and SPLIT_DEFAULT:
            plain = flabel[:-1]
            prec = R.route_mode(case, mode, plain, SPLIT_DEFAULT)
            if prec["mfma"] == "split":
                assert rec["mfma"] == "f32"
                other, _ = launch(case, mode, plain, dev, inp, prec)
                assert not torch.equal(other["y"], got["y"]), "the split and the native form gave the same bits: one of them did not run"
    torch.cuda.synchronize()
    print("PW64 time %-4s %s %.2f s" % (flabel, name, time.time() - t0))


def names(flabel):
    return [c["name"] for c in R.PW_CASES if flabel in c["forms"]]


@pytest.mark.parametrize("name", names("auto"))
def test_pwconv_fwd(name):
    """mmd_pwconv_fwd: the measured shape filters decide (tiled, skinny, row-slab and long-K launches)"""
    run_case(name, "auto")


@pytest.mark.parametrize("name", names("f0"))
def test_pwconv_fwd_form0(name):
    run_case(name, "f0")


@pytest.mark.parametrize("name", names("f0n"))
def test_pwconv_fwd_form0_native(name):
    run_case(name, "f0n")


@pytest.mark.parametrize("name", names("f1"))
def test_pwconv_fwd_form1(name):
    """the thin-K row-slab kernel, every <K / 8, chunk width> instantiation, and the launches it refuses"""
    run_case(name, "f1")


@pytest.mark.parametrize("name", names("f1n"))
def test_pwconv_fwd_form1_native(name):
    run_case(name, "f1n")


@pytest.mark.parametrize("name", names("f2"))
def test_pwconv_fwd_form2(name):
    """the LDS-tiled kernels: skinny 32x64, 128x32, 64x64, 128x64, nkl 1 - 4, split form where K >= 64 and N > 48"""
    run_case(name, "f2")


@pytest.mark.parametrize("name", names("f2n"))
def test_pwconv_fwd_form2_native(name):
    """the same launches on v_mfma_f32; where the plain form is the split form the two must differ in bits"""
    run_case(name, "f2n")


@pytest.mark.parametrize("name", names("f3"))
def test_pwconv_fwd_form3(name):
    """the long-K kernel, launched three times, and the launch it refuses"""
    run_case(name, "f3")


@pytest.mark.parametrize("name", names("f3n"))
def test_pwconv_fwd_form3_native(name):
    run_case(name, "f3n")


@pytest.mark.parametrize("name", names("bf16"))
def test_pwconv_fwd_bf16(name):
    """operands rounded to bf16 at the MFMA input: against float64 of the unrounded operands in units of 2^-9 A"""
    run_case(name, "bf16")


@pytest.mark.parametrize("flabel", ["auto", "f2", "f1", "f3", "bf16"])
def test_bad_arguments_return_einval_and_write_nothing(flabel):
    """K % 4 != 0, N % 4 != 0, a gate with rows_per_image = 0, in_scale without in_shift, live statistics together with a given scale:
    -22 on the host, y keeps its NaN and the sums their pre-fill"""
    entry, form, _, _ = R.FORMS[flabel]
    f = lambda *s: torch.full(s, 0.25, device=DEV)
    live = (torch.ones(32, dtype=D, device=DEV), f(16), f(16), 40)
    no_live = (None, None, None, 0)
    bad = {"K % 4": dict(K=10), "N % 4": dict(N=6), "gate, rows_per_image 0": dict(gate=f(2, 16), rpi=0), "scale without shift": dict(scale=f(16)),
           "live and a given scale": dict(scale=f(16), shift=f(16), live=live)}
    for what, o in bad.items():
        M, K, N = 40, o.get("K", 16), o.get("N", 8)
        y, st = Out((M, N), "nan"), Out((2 * N,), torch.ones(2 * N), D)
        args = [f(M, K), f(N, K), y.t, M, K, N, o.get("scale"), o.get("shift"), 0, *o.get("live", no_live), o.get("gate"), o.get("rpi", 20), None, None,
                None, 0, None, st.t, 0, 0, None, 0]
        if entry == "mmd_pwconv_fwd_form":
            args += [None, 0, form]
        with pytest.raises(RuntimeError, match="status -22"):
            call(entry, *args)
        torch.cuda.synchronize()
        assert bool(torch.isnan(y.get()).all()) and bool((st.get() == 1).all()), what
