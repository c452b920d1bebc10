"""GPU: the 1x1-conv input-gradient entry points - mmd_pwconv_bwd_data, _bf16, mmd_pwconv_bwd_data_bn, _bn_bf16, mmd_pwconv_bwd_data_bn2,
_bn2_bf16 and mmd_pwconv_bwd_data_bn2_form (csrc/pw_gemm.hip, pw_slab.hip) - against the float64 reference of tests/bd_ref.py, through the C
ABI, on the tables bd_ref.BD_CASES / PLAIN_CASES (test_bd_ref_cpu.py proves through bd_ref.route that every branch is reached).  Sizes as in
bd_ref: M rows, K input and N output channels; the GEMM reduces over Kg = N and writes Ng = K columns.

Every comparison is per element: |got_i - ref64_i| <= K * unit * A_i + tiny, A_i the magnitude the reference reports for that element, unit
2^-24 (2^-9 for what the bf16 rounding reaches) and K the family's constant of bd_ref (calibrated on the CPU by test_bd_ref_cpu.py, never on
these kernels).  The float64 references run on the GPU in torch, with nothing of the library under test: the BatchNorm sums handed to the
kernels are elt_ref.bn_bwd_reduce's.  dx and dz_out lie in front of 16 guard rows and are pre-filled with NaN (dx with the residual where
it aliases it): dz_out finite everywhere is dz_out written; dgamma / dbeta, xs_sums and p5_out are pre-filled with non-zero values (the
kernels accumulate: a second add by another column tile would be an error of the size of the sums), or must keep their pre-fill where they
are not passed.  A slot workspace is all zero afterwards and dx has the bits of the ws_slots = 0 launch; a slab workspace has exactly
mmd_pwconv_slab_ws_floats floats of NaN in front of a guard, that number is the copied plan's, and a sliced launch is repeated twice more
with identical bits of dx and dz_out.  The split and the native form of one launch differ in bits; two launches of the same v_mfma_f32
kernel do not.  Each check prints `BD64 <family> <case> <mode> <form> <worst err / (unit A)> (K)` before it asserts."""
import os
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from mm_distillnet_amd import _lib

import bd_ref as R
import pw_ref
from pw_ref import Out, GPU_ERROR          # the guarded output buffer; the list of GPU errors met (shared: after one, no module launches)

call = _lib.call
DEV = "cuda"
D, F = torch.float64, torch.float32
SPLIT_DEFAULT = "MMD_MFMA_F32" not in os.environ          # mmd_split_default (common.h): set, to any value, is v_mfma_f32
WS_GUARD = 4096
NAN = float("nan")


def guarded(label, fn, *args):
    assert not GPU_ERROR, "an earlier test hit a GPU error (%s): not launching anything more" % GPU_ERROR[0]
    try:
        return fn(*args)
    except RuntimeError as e:
        GPU_ERROR.append("%s: %s" % (label, str(e)[:200]))
        raise


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64)


def judge(family, label, got, ref, A):
    """got / ref / A: tensors of one shape (every element is judged) -> the worst err / (unit A)"""
    K, unit = R.K_BY_FAMILY[family], R.UNIT[family]
    got, ref, A = got.double(), ref.double(), A.double()
    assert got.shape == ref.shape == A.shape, (got.shape, ref.shape, A.shape)
    assert bool(torch.isfinite(got).all()), "%s %s: an element was not written (or is not finite)" % (family, label)
    r = float(((got - ref).abs() / (unit * A + R.TINY)).max())
    print("BD64 %-14s %-58s %8.3f  (K %.0f)" % (family, label, r, K))
    assert r <= K, "%s %s: err / (unit A) = %.3f > K = %.1f" % (family, label, r, K)
    return r


# ------------------------------------------------------------------------------------------------ BatchNorm-operand launches
def launch(case, mode, form, inp, d, sums, ws_slots=None):
    """one launch of (case, mode) through the entry point of `form` on pre-filled outputs -> dict of the output tensors, guards checked"""
    f = R.flags(mode)
    entry, fm, bf16, sws = R.FORMS[form]
    M, K, N, B = case["M"], case["K"], case["N"], case["B"]
    slots = f["ws"] if ws_slots is None else ws_slots
    dx = Out((M, K), inp["res"] if f["res"] == "alias" else "nan")
    dz = Out((M, N), "nan")
    dg, db = Out((N,), inp["dgamma0"]), Out((N,), inp["dbeta0"])
    args = [d["g"], d["z"], d["wt"], dx.t, M, K, N, d["scale"], d["shift"], d["mean"], d["invstd"], sums, M, f["act"],
            d["mul_b"] if f["mulb"] else None, R.BN_RPI, dz.t if f["dz"] else None, dg.t if f["dsum"] else None, db.t if f["dsum"] else None]
    xs = Out((2 * K,), inp["xs0"], dtype=D)
    p5 = Out((5, B, K), inp["p5_0"])
    sw = torch.zeros(slots * 2 * K, dtype=D, device=DEV) if slots else None
    ws = nws = None
    if entry.startswith("mmd_pwconv_bwd_data_bn2"):
        args += [dx.t if f["res"] == "alias" else (d["res"] if f["res"] else None)]
        args += [d["xs_z"], d["xs_mean"], d["xs_invstd"], d["xs_mul_b"] if f["xs"] == "xsm" else None, R.XS_RPI, xs.t] if f["xs"] else [None, None, None, None, 0, None]
        args += [sw, slots]
        args += [d["p5_z"], d["p5_scale"], d["p5_shift"], d["p5_mean"], d["p5_invstd"], p5.t, B] if f["p5"] else [None, None, None, None, None, None, 0]
        if fm is not None:
            if sws:
                nws = int(_lib.LIB.load().mmd_pwconv_slab_ws_floats(M, case["Kg"], case["Ng"], 1))
                ws = torch.full((nws + WS_GUARD,), R.SENTINEL, device=DEV)
                ws[:nws].fill_(NAN)
            args += [ws, nws or 0, fm]
    else:
        assert R.bn_only(mode)
    call(entry, *args)
    torch.cuda.synchronize()
    if ws is not None:
        assert bool((ws[nws:] == R.SENTINEL).all()), "the launch wrote behind its slab workspace"
    if sw is not None:
        assert not bool(sw.any()), "the slot workspace must be left zero"
    out = {"dx": dx.get(), "dz": dz.get(), "dgamma": dg.get(), "dbeta": db.get(), "xs": xs.get(), "p5": p5.get()}
    if not f["dz"]:
        assert bool(torch.isnan(out["dz"]).all())
    if not f["dsum"]:
        assert torch.equal(out["dgamma"], d["dgamma0"]) and torch.equal(out["dbeta"], d["dbeta0"]), "dgamma / dbeta were not passed"
    if not f["xs"]:
        assert torch.equal(out["xs"], d["xs0"])
    if not f["p5"]:
        assert torch.equal(out["p5"], d["p5_0"])
    return out


def check(case, mode, form, out, ref, tag=""):
    """every element of every output of one launch against the float64 reference"""
    f = R.flags(mode)
    bf = bool(R.FORMS[form][2])
    sfx = "_bf16" if bf else ""
    label = "%s [%s] %s%s" % (case["name"], mode, form, tag)
    K = case["K"]
    judge("dx" + sfx, label, out["dx"], *ref["dx"])
    if f["dz"]:
        judge("dz", label, out["dz"], *ref["dz"])          # finite everywhere: every row and channel was stored, by whichever column tile owns it
    if f["dsum"]:
        judge("dsum", label + " dgamma", out["dgamma"], *ref["dgamma"])
        judge("dsum", label + " dbeta", out["dbeta"], *ref["dbeta"])
    if f["xs"]:
        judge("xs_sum" + sfx, label, out["xs"][:K], *ref["xs_sum"])
        judge("xs_sumsq" + sfx, label, out["xs"][K:], *ref["xs_sumsq"])
    if f["p5"]:
        judge("p5" + sfx, label, out["p5"], *ref["p5"])


def _case(name):
    t0 = time.time()
    case = R.CASE[name]
    inp = R.case_inputs(case)
    d, d64 = R.to(inp, F, DEV), R.to(inp, D, DEV)
    lib = _lib.LIB.load()
    for mode in case["modes"]:
        sums = R.case_sums(case, mode, d64)
        ref = R.case_ref(case, mode, d64, sums)
        res = {}
        for m, form in R.runs(case):
            if m != mode:
                continue
            r = R.route_mode(case, mode, form, split_default=SPLIT_DEFAULT)
            if r["family"] == "slab":          # the one place where the dispatch copy meets the host code
                assert int(lib.mmd_pwconv_slab_ws_floats(case["M"], case["Kg"], case["Ng"], 1)) == r["part_floats"], "slab_plan's copy is not the host's"
            out = res[form] = launch(case, mode, form, inp, d, sums)
            check(case, mode, form, out, ref)
            if R.flags(mode)["ws"]:
                assert r["slotted"]
                direct = launch(case, mode, form, inp, d, sums, ws_slots=0)
                check(case, mode, form, direct, ref, "/direct")
                assert torch.equal(bits(direct["dx"]), bits(out["dx"])), "%s [%s] %s: dx differs between slotted and direct sums" % (name, mode, form)
            if r["family"] == "slab" and r["nslice"] > 1:
                for _ in range(2):
                    again = launch(case, mode, form, inp, d, sums)
                    same_dz = torch.equal(bits(again["dz"]), bits(out["dz"]))
                    assert torch.equal(bits(again["dx"]), bits(out["dx"])) and same_dz, "%s [%s] %s: a sliced launch repeated with other bits" % (name, mode, form)
        if "f2" in res and "f2n" in res:
            r2, rn = R.route_mode(case, mode, "f2", split_default=SPLIT_DEFAULT), R.route_mode(case, mode, "f2n", split_default=SPLIT_DEFAULT)
            same = torch.equal(bits(res["f2"]["dx"]), bits(res["f2n"]["dx"]))
            if r2["mfma"] == "split":
                assert not same, "%s [%s]: the split form and v_mfma_f32 gave the same bits: the split kernel did not run" % (name, mode)
            elif r2 == rn:
                assert same, "%s [%s]: two launches of one v_mfma_f32 kernel gave other bits" % (name, mode)
    if name in ("sl_refused", "sl_p5", "t1_k12"):
        assert int(lib.mmd_pwconv_slab_ws_floats(case["M"], case["Kg"], case["Ng"], 1)) == 0
    print("BD64 time %s %.2f s" % (name, time.time() - t0))


@pytest.mark.parametrize("name", [c["name"] for c in R.BD_CASES])
def test_pwconv_bwd_data_bn(name):
    """every mode of the case through every entry point / form it lists: float64 per element, guards, pre-fills, workspaces, bits"""
    guarded("bwd_data_bn %s" % name, _case, name)


# ------------------------------------------------------------------------------------------------ plain launches
def _plain(name):
    t0 = time.time()
    pc = pw_ref.CASE[name]
    M, Kg, Ng = pc["M"], pc["K"], pc["N"]          # the conv's N is the launch's reduction length, its K the output width
    for acc in (0, 1):
        d, (v, A) = R.plain_ref(name, acc, D, DEV)
        d32 = {k: (t.float() if isinstance(t, torch.Tensor) else t) for k, t in d.items()}
        for sfx in ("", "_bf16"):
            dx = Out((M, Ng), d32["res"] if acc else "nan")
            call("mmd_pwconv_bwd_data" + sfx, d32["x"], d32["w"], dx.t, M, Ng, Kg, acc)
            torch.cuda.synchronize()
            judge("dx" + sfx, "plain %s acc %d%s" % (name, acc, sfx), dx.get(), v, A)
    print("BD64 time plain %s %.2f s" % (name, time.time() - t0))


@pytest.mark.parametrize("name", [n for n, _ in R.PLAIN_CASES])
def test_pwconv_bwd_data_plain(name):
    """mmd_pwconv_bwd_data / _bf16, accumulate 0 (dx pre-filled with NaN) and 1 (dx holds the gradient it is added to)"""
    guarded("bwd_data %s" % name, _plain, name)


# ------------------------------------------------------------------------------------------------ bad arguments
def _bad(form):
    entry, fm, _, _ = R.FORMS[form]
    bn2 = entry.startswith("mmd_pwconv_bwd_data_bn2")
    f = lambda *s: torch.full(s, 0.25, device=DEV)
    bad = {"K % 4": dict(K=10), "N % 4": dict(N=6), "scale null": dict(scale=None), "count 0": dict(count=0), "mul_b, rows_per_image 0": dict(mul_b=f(8), rpi=0),
           "dgamma without dbeta": dict(dbeta=None)}
    bad2 = {"xs_z without xs_mean": dict(xs=True, xs_mean=None), "p5_z with a residual": dict(p5=True, res=True), "M % p5_B": dict(p5=True, p5_B=3)}
    badf = {"form 5": dict(form=5), "form -1": dict(form=-1), "form 5 | native": dict(form=5 | R.MMD_PW_FORM_NATIVE),
            "form 4, sliced shape, no workspace": dict(M=32, K=64, N=512, form=4)}
    for what, o in {**bad, **(bad2 if bn2 else {}), **(badf if fm is not None else {})}.items():
        M, K, N = o.get("M", 40), o.get("K", 16), o.get("N", 8)
        if "sliced" in what:
            assert R.route(4, 0, 0, M, N, K) == {"rc": -22}
        dx, dz, dg, db = Out((M, K), torch.ones(M, K)), Out((M, N), torch.ones(M, N)), Out((N,), torch.ones(N)), Out((N,), torch.ones(N))
        xs, p5 = Out((2 * K,), torch.ones(2 * K), dtype=D), Out((5, 2, K), torch.ones(5, 2, K))
        args = [f(M, N), f(M, N), f(K, N), dx.t, M, K, N, o.get("scale", f(N)), f(N), f(N), f(N), torch.ones(2 * N, dtype=D, device=DEV), o.get("count", M), 1,
                o.get("mul_b"), o.get("rpi", 7), dz.t, dg.t, o.get("dbeta", db.t)]
        if bn2:
            args += [f(M, K) if o.get("res") else None]
            args += [f(M, K), o.get("xs_mean", f(K)), f(K), None, 0, xs.t] if o.get("xs") else [None, None, None, None, 0, None]
            args += [None, 0]
            args += [f(M, K), f(K), f(K), f(K), f(K), p5.t, o.get("p5_B", 2)] if o.get("p5") else [None, None, None, None, None, None, 0]
            if fm is not None:
                args += [None, 0, o.get("form", fm)]
        with pytest.raises(RuntimeError, match="status -22"):
            call(entry, *args)
        torch.cuda.synchronize()
        for t in (dx, dz, dg, db, xs, p5):
            assert bool((t.get() == 1).all()), "%s: a refused launch wrote an output" % what


@pytest.mark.parametrize("form", ["bn", "bn_bf16", "bn2", "bf16", "f0"])
def test_bad_arguments_return_einval_and_write_nothing(form):
    """K % 4, N % 4, a null scale, count = 0, mul_b with rows_per_image = 0, dgamma without dbeta; on the _bn2 entry points xs_z without xs_mean,
    p5_z together with a residual, M % p5_B != 0; on the form entry point a form above 4 (or below 0) and form 4 on a sliced shape without a
    workspace: -22, and dx, dz_out, dgamma, dbeta, xs_sums, p5_out keep their pre-fill"""
    guarded("bad arguments %s" % form, _bad, form)
