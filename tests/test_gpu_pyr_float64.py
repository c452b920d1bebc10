"""GPU: the detection heads' feature-pyramid launches - mmd_dwconv3_pyr, mmd_dwconv3_pyr_bwd_weight, mmd_pwconv_fwd_pyr(_bf16),
mmd_bn_bwd_reduce_pyr, mmd_bn_bwd_apply_pyr, mmd_pyr_add_bnsums, mmd_slice_rows_pyr and the grouped-nets mode of the two forward entry
points - against the float64 references of tests/pyr_ref.py, through the C ABI, on the case table pyr_ref.PYR_CASES (test_pyr_ref_cpu.py
proves through the copied dispatch that every route is reached, and the references against plain torch).

Every comparison is per element: |got_i - ref64_i| <= K * unit * A_i + tiny, A_i the magnitude the reference reports, unit 2^-24 (2^-9 for
the bf16 entry point) and K the family's constant of pyr_ref (calibrated on the CPU, never on these kernels).  Padding rows of every input
row buffer hold sentinel-sized finite garbage; every stored output is pre-filled with the sentinel and its padding rows must still hold it
bitwise afterwards (zeros for mmd_slice_rows_pyr: see the docstring of pyr_ref for what each entry point does with them); every reduction
output starts from non-zero values, is judged against the reference of the valid rows alone, and the entries between the level slots
(lev_stride > C) must keep their contents.  Each check prints `PYR64 <family> <case> <mode> <worst err / (unit A)> (K)` before it asserts and
names the worst element (level, row within the level, channel) when it fails.  After a launch or runtime error in one test the later tests
launch nothing (pw_ref.GPU_ERROR; an unexpected MMD_EINVAL, returned by the host before any launch, fails only its own test).  The float64 references run on the GPU in torch (nothing of the library under test)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from mm_distillnet_amd import _lib

import pyr_ref as R
from pw_ref import Out, GPU_ERROR

call = _lib.call
DEV = "cuda"
D = torch.float64
SENT = R.SENTINEL


def g(t):
    return None if t is None else t.detach().contiguous().to(DEV)


def guarded(fn):
    def run(name):
        assert not GPU_ERROR, "an earlier test hit a GPU error (%s): not launching anything more" % GPU_ERROR[0]
        try:
            fn(name)
            torch.cuda.synchronize()
        except RuntimeError as e:
            if "failed with status -22" not in str(e):          # (MMD_EINVAL is the host's refusal before any launch: the device is untouched)
                GPU_ERROR.append("%s: %s" % (name, str(e)[:200]))
            raise
    run.__name__, run.__doc__ = fn.__name__, fn.__doc__
    return run


def judge(fam, label, got, ref, A, lev=None):
    K, unit = R.K_BY_FAMILY[fam], R.UNIT[fam]
    r = R.ratio_u(got, ref, A, unit)
    print("PYR64 %-13s %-70s %8.3f  (K %.0f)" % (fam, label + ("" if lev is None else " L%d" % lev), r, K))
    if r > K:
        w, idx = R.worst(got, ref, A, unit)
        raise AssertionError("%s %s: err / (unit A) = %.3f > K = %.1f at level %s, (row in level, channel) %s" % (fam, label, w, K, lev, idx))


def judge_rows(fam, label, P, buf, ref):
    """a stored row buffer: every level against its reference; the padding rows still hold the sentinel, bitwise"""
    t = buf.get()
    for l in range(P.n):
        judge(fam, label, R.lvl(t, P, l), *ref[l], lev=l)
    assert bool((t[~P.valid().to(DEV)] == SENT).all()), "%s: padding rows of the output were written" % label


def judge_slots(fam, label, P, buf, init, ref, ls, o, width, two=True):
    """per-level reduction slots (width elements at (2 *) (o + l * ls)): each against its reference, everything else unchanged"""
    t = buf.get()
    keep = torch.ones(t.numel(), dtype=torch.bool)
    for l in range(P.n):
        a = (2 if two else 1) * (o + l * ls)
        keep[a:a + width] = False
        judge(fam, label, t[a:a + width], *ref[l], lev=l)
    assert torch.equal(t.cpu()[keep], init.to(t.dtype)[keep]), "%s: entries between the level slots were written" % label


def setup(name):
    case = R.CASE[name]
    inp = R.case_inputs(case)
    tens = lambda v: v is None or isinstance(v, torch.Tensor)
    dev = {k: (g(t) if isinstance(t, torch.Tensor) else [g(v) for v in t] if isinstance(t, list) and all(map(tens, t)) else t) for k, t in inp.items()}
    return case, inp, dev, R.pyr_of(case["pyr"])


# ------------------------------------------------------------------------------------------------ depthwise
def dw_args(mode, dev, o):
    """-> (x, flip, in_scale, in_shift, in_act, in_stats, in_gamma, in_beta, wg_x, wg_scale, wg_shift, wg_act, rider level)"""
    at = lambda k: dev[k][o:]
    n = None
    if mode == "fwd_plain":
        return (dev["x"], 0, n, n, 0, n, n, n, n, n, n, 0, 0)
    if mode == "fwd_given":
        return (dev["x"], 0, at("scale"), at("shift"), 1, n, n, n, n, n, n, 0, 0)
    if mode == "fwd_live":
        return (dev["x"], 0, n, n, 1, dev["stats"][2 * o:], at("gamma"), at("beta"), n, n, n, 0, 0)
    if mode == "bwd_plain":
        return (dev["dy"], 1, n, n, 0, n, n, n, n, n, n, 0, 0)
    if mode == "bwd_wg_plain":
        return (dev["dy"], 1, n, n, 0, n, n, n, dev["x"], n, n, 0, 1)
    return (dev["dy"], 1, n, n, 0, n, n, n, dev["x"], at("scale"), at("shift"), 1, 2 if mode == "bwd_wg_bn" else 1)


@pytest.mark.parametrize("name", R.cases_of("dw"))
@guarded
def test_dwconv3_pyr(name):
    """mmd_dwconv3_pyr, seven modes per case: flip 0 plain / folded scale, shift + swish / live BatchNorm from each level's own sums and
    count; flip 1 plain, + dw_grad (plain wg_x, wg_scale / shift + swish), + bn_sums - on the tile route and, where the dispatch allows it,
    the row-streaming route (riders fused) against the tile route's two follow-up launches"""
    case, inp, dev, P = setup(name)
    C, ls, o = case["C"], inp["ls"], inp["o"]
    for mode in R.DW_MODES:
        x, flip, isc, ish, iact, ist, iga, ibe, wgx, wsc, wsh, wact, rider = dw_args(mode, dev, o)
        rt = R.dw_route_of(case, mode)
        label = "%s %s [%s%s]" % (name, mode, rt["kernel"], "+" + rt["riders"] if rt["riders"] else "")
        ref = R.case_ref(case, mode, inp, D, DEV)
        y, dwg, bns = Out((P.Mt, C), "sent"), Out((9, C), inp["dw0"]), Out((inp["sums0"].numel(),), inp["sums0"], D)
        call("mmd_dwconv3_pyr", x, dev["w"], y.t, P.desc(), C, flip, isc, ish, iact, ist, iga, ibe, ls, wgx, wsc, wsh, wact,
             dwg.t if rider else None, dev["mean"][o:] if rider == 2 else None, dev["invstd"][o:] if rider == 2 else None,
             bns.t[2 * o:] if rider == 2 else None)
        judge_rows(R.family_of(case, mode, "y"), label + " y", P, y, ref["y"])
        if rider:
            judge("dwgrad", label + " dw_grad", dwg.get(), *ref["dw_grad"])
        else:
            assert torch.equal(dwg.get().cpu(), inp["dw0"])
        if rider == 2:
            judge_slots("bnsums", label + " bn_sums", P, bns, inp["sums0"], ref["bn_sums"], ls, o, 2 * C)
        else:
            assert torch.equal(bns.get().cpu(), inp["sums0"])


@pytest.mark.parametrize("name", R.cases_of("wg"))
@guarded
def test_dwconv3_pyr_bwd_weight(name):
    """mmd_dwconv3_pyr_bwd_weight, plain and with a per-level prologue, onto a non-zero dw; levels with one and with several blocks per image"""
    case, inp, dev, P = setup(name)
    C, ls, o = case["C"], inp["ls"], inp["o"]
    for mode in R.WG_MODES:
        dw = Out((9, C), inp["dw0"])
        pro = mode == "pro"
        call("mmd_dwconv3_pyr_bwd_weight", dev["x"], dev["dy"], dw.t, P.desc(), C, dev["scale"][o:] if pro else None, dev["shift"][o:] if pro else None,
             int(pro), ls if pro else 0)
        judge("dwgrad", "%s %s nsplit %s" % (name, mode, R.wgrad_nsplit(P)), dw.get(), *R.case_ref(case, mode, inp, D, DEV)["dw"])


# ------------------------------------------------------------------------------------------------ the GEMM
def run_pw(case, inp, dev, P, bf16, x, w, bias, label, ref):
    K, N, ls, o = case["C"], case["N"], inp["ls"], inp["o"]
    sfx = "_bf16" if bf16 else ""
    strided, stats = case.get("strided"), case.get("stats")
    y = Out((P.B, inp["bstride"]), "sent") if strided else Out((P.Mt, N), "sent")
    st = Out((inp["stats0"].numel(),), inp["stats0"], D) if stats else None
    yoff = (ctypes.c_longlong * P.n)(*inp["yoff"]) if strided else None
    call("mmd_pwconv_fwd_pyr" + sfx, x, w, y.t, P.desc(), K, N, bias, case.get("act", 0), st.t[2 * o:] if st else None, ls,
         inp["bstride"] if strided else 0, yoff)
    if strided:
        flat = y.get().reshape(-1)
        outside = torch.ones(flat.numel(), dtype=torch.bool, device=DEV)
        for l in range(P.n):
            idx = R.head_index(P, l, N, inp["bstride"], inp["yoff"], DEV)
            outside[idx.reshape(-1)] = False
            judge("pw_y" + sfx, label + " y", flat[idx], *ref["y"][l], lev=l)
        assert bool((flat[outside] == SENT).all()), "%s: the strided launch wrote outside the levels' windows" % label
    else:
        judge_rows("pw_y" + sfx, label + " y", P, y, ref["y"])
    if st:
        t, keep = st.get(), torch.ones(inp["stats0"].numel(), dtype=torch.bool)
        for l in range(P.n):
            a = 2 * (o + l * ls)
            keep[a:a + 2 * N] = False
            judge("pw_sum" + sfx, label + " sum", t[a:a + N], *ref["sum"][l], lev=l)
            judge("pw_sumsq" + sfx, label + " sumsq", t[a + N:a + 2 * N], *ref["sumsq"][l], lev=l)
        assert torch.equal(t.cpu()[keep], inp["stats0"][keep]), "%s: entries between the level slots were written" % label


@pytest.mark.parametrize("name", R.cases_of("pw"))
@guarded
def test_pwconv_fwd_pyr(name):
    """mmd_pwconv_fwd_pyr and _bf16 on the skinny, 128x32, 64x64, 128x64 and row-slab routes: bias on / off, sigmoid, per-level statistics
    onto non-zero starts lev_stride apart, the strided head output with per-level offsets; one float64 reference for both entry points"""
    case, inp, dev, P = setup(name)
    ref = R.case_ref(case, False, inp, D, DEV)
    for bf16 in (False, True):
        route = R.route_pw(P, case["C"], case["N"], bf16, bool(case["stats"]), bool(case["strided"]))[0]
        assert route == case["route"][bf16]
        run_pw(case, inp, dev, P, bf16, dev["x"], dev["w"], dev["bias"] if case["bias"] else None, "%s%s [%s]" % (name, " bf16" if bf16 else "", route), ref)


# ------------------------------------------------------------------------------------------------ the two BatchNorm passes
@pytest.mark.parametrize("name", R.cases_of("red"))
@guarded
def test_bn_bwd_reduce_pyr(name):
    """mmd_bn_bwd_reduce_pyr: g_out stored and null, swish and none, the sums onto non-zero starts with each level's own coefficients"""
    case, inp, dev, P = setup(name)
    C, ls, o = case["C"], inp["ls"], inp["o"]
    for act, store in R.RED_MODES:
        ref = R.case_ref(case, (act, store), inp, D, DEV)
        gout, sums = Out((P.Mt, C), "sent"), Out((inp["sums0"].numel(),), inp["sums0"], D)
        call("mmd_bn_bwd_reduce_pyr", dev["dy"], dev["x"], dev["scale"][o:], dev["shift"][o:], dev["mean"][o:], dev["invstd"][o:], act, P.desc(), ls,
             gout.t if store else None, sums.t[2 * o:], C)
        label = "%s act %d g_out %d" % (name, act, store)
        if store:
            judge_rows("red_g", label + " g", P, gout, ref["g"])
        else:
            assert bool((gout.get() == SENT).all())
        judge_slots("red_sums", label + " sums", P, sums, inp["sums0"], ref["sums"], ls, o, 2 * C)


@pytest.mark.parametrize("name", R.cases_of("app"))
@guarded
def test_bn_bwd_apply_pyr(name):
    """mmd_bn_bwd_apply_pyr: stored g (act none) and g recomputed from scale / shift + swish; the mean terms divide by each level's own
    B*H*W; dgamma / dbeta null and accumulated onto non-zero starts"""
    case, inp, dev, P = setup(name)
    C, ls, o = case["C"], inp["ls"], inp["o"]
    for rec, grads in R.APP_MODES:
        ref = R.case_ref(case, (rec, grads), inp, D, DEV)
        dz, dga, dbe = Out((P.Mt, C), "sent"), Out((inp["dgamma0"].numel(),), inp["dgamma0"]), Out((inp["dbeta0"].numel(),), inp["dbeta0"])
        call("mmd_bn_bwd_apply_pyr", dev["dy"], dev["x"], dev["mean"][o:], dev["invstd"][o:], dev["gamma"][o:], dev["sums"][2 * o:], P.desc(), ls,
             dz.t, dga.t[o:] if grads else None, dbe.t[o:] if grads else None, C, dev["scale"][o:] if rec else None, dev["shift"][o:] if rec else None, int(rec))
        label = "%s recompute %d grads %d" % (name, rec, grads)
        judge_rows("app_dz", label + " dz", P, dz, ref["dz"])
        if grads:
            judge_slots("app_dsum", label + " dgamma", P, dga, inp["dgamma0"], ref["dgamma"], ls, o, C, two=False)
            judge_slots("app_dsum", label + " dbeta", P, dbe, inp["dbeta0"], ref["dbeta"], ls, o, C, two=False)
        else:
            assert torch.equal(dga.get().cpu(), inp["dgamma0"]) and torch.equal(dbe.get().cpu(), inp["dbeta0"])


# ------------------------------------------------------------------------------------------------ add + BatchNorm sums, slice
def ptrs(ts, n):
    return (ctypes.c_void_p * n)(*[(t.data_ptr() if t is not None else None) for t in ts])


@pytest.mark.parametrize("name", R.cases_of("add"))
@guarded
def test_pyr_add_bnsums(name):
    """mmd_pyr_add_bnsums: c null and given, out aliasing a, levels with and without a z tensor of their own, sums onto non-zero starts"""
    case, inp, dev, P = setup(name)
    C = case["C"]
    for with_c, alias in R.ADD_MODES:
        ref = R.case_ref(case, (with_c, alias), inp, D, DEV)
        sums = [Out((2 * C,), s, D) if s is not None else None for s in inp["sums0"]]
        if alias:
            a = out = Out((P.Mt, C), inp["a"])
        else:
            a, out = None, Out((P.Mt, C), "sent")
        call("mmd_pyr_add_bnsums", a.t if alias else dev["a"], dev["b"], dev["c"] if with_c else None, out.t, P.desc(), C, ptrs(dev["z"], P.n),
             ptrs(dev["mean"], P.n), ptrs(dev["invstd"], P.n), ptrs([s.t if s else None for s in sums], P.n))
        label = "%s c %d alias %d" % (name, with_c, alias)
        t = out.get()
        for l in range(P.n):
            judge("add_out", label + " out", R.lvl(t, P, l), *ref["out"][l], lev=l)
            if sums[l] is not None:
                judge("add_sums", label + " sums", sums[l].get(), *ref["sums"][l], lev=l)
        pad = ~P.valid().to(DEV)
        assert torch.equal(t[pad], dev["a"][pad] if alias else torch.full_like(t[pad], SENT)), "%s: padding rows of out were written" % label


@pytest.mark.parametrize("name", R.cases_of("slice"))
@guarded
def test_slice_rows_pyr(name):
    """mmd_slice_rows_pyr: an exact gather on the vec 2 path (N, offsets and batch stride even) and the vec 1 path (odd offsets, odd N);
    the padding rows are written with zeros"""
    case, inp, dev, P = setup(name)
    N = case["N"]
    dst = Out((P.Mt, N), "sent")
    call("mmd_slice_rows_pyr", dev["src"], dst.t, P.desc(), N, inp["bstride"], (ctypes.c_longlong * P.n)(*inp["offs"]))
    assert torch.equal(dst.get().cpu(), R.slice_rows_pyr(P, inp["src"], N, inp["offs"]))


# ------------------------------------------------------------------------------------------------ grouped nets
def _einval(entry, *args):
    with pytest.raises(RuntimeError, match="status -22"):
        call(entry, *args)


@guarded
def _grouped(_):
    dll = _lib.LIB.load()
    case, inp, dev, P = setup(R.cases_of("gdw")[0])
    C, ls, o = case["C"], inp["ls"], inp["o"]
    pcase, pinp, pdev, _ = setup(R.cases_of("gpw")[0])
    N = pcase["N"]
    y, y2 = Out((P.Mt, C), "sent"), Out((P.Mt, C), "sent")
    z = {bf: Out((P.Mt, N), "sent") for bf in (False, True)}
    z2 = Out((R.pyr_of("pgbad").Mt, N), "sent")
    n = None
    assert dll.mmd_set_group(R.GROUP_N, R.GROUP_IMAGES, inp["w_stride"], inp["bn_stride"]) == 0
    try:
        call("mmd_dwconv3_pyr", dev["x"], dev["w_buf"], y.t, P.desc(), C, 0, dev["sc_buf"][o:], dev["sh_buf"][o:], 1, n, n, n, ls, n, n, n, 0, n, n, n, n)
        # refusals under a group: flip, dw_grad, in_stats
        _einval("mmd_dwconv3_pyr", dev["x"], dev["w_buf"], y2.t, P.desc(), C, 1, n, n, 0, n, n, n, ls, n, n, n, 0, n, n, n, n)
        _einval("mmd_dwconv3_pyr", dev["x"], dev["w_buf"], y2.t, P.desc(), C, 1, n, n, 0, n, n, n, ls, dev["x"], n, n, 0, dev["w_buf"], n, n, n)
        _einval("mmd_dwconv3_pyr", dev["x"], dev["w_buf"], y2.t, P.desc(), C, 0, n, n, 1, torch.ones(4 * inp["bn_stride"], dtype=D, device=DEV),
                dev["sc_buf"], dev["sh_buf"], ls, n, n, n, 0, n, n, n, n)
        assert dll.mmd_set_group(R.GROUP_N, R.GROUP_IMAGES, pinp["w_stride"], pinp["bn_stride"]) == 0
        for bf in (False, True):
            call("mmd_pwconv_fwd_pyr" + ("_bf16" if bf else ""), pdev["x"], pdev["w_buf"], z[bf].t, P.desc(), C, N, pdev["bias_buf"], 0, n, 0, 0, n)
        # a level that breaks the tile condition (15 rows per image on the 32-row kernel)
        _einval("mmd_pwconv_fwd_pyr", pdev["x"], pdev["w_buf"], z2.t, R.pyr_of("pgbad").desc(), C, N, pdev["bias_buf"], 0, n, 0, 0, n)
    finally:
        rc = dll.mmd_set_group(1, 0, 0, 0)
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((y2.get() == SENT).all()) and bool((z2.get() == SENT).all())
    judge_rows("dw", "grouped mmd_dwconv3_pyr", P, y, R.case_ref(case, None, inp, D, DEV)["y"])
    ref = R.case_ref(pcase, False, pinp, D, DEV)["y"]
    for bf in (False, True):
        judge_rows("pw_y" + ("_bf16" if bf else ""), "grouped mmd_pwconv_fwd_pyr%s" % ("_bf16" if bf else ""), P, z[bf], ref)


def test_grouped_nets_and_their_refusals():
    """mmd_set_group(2 nets, 1 image each): mmd_dwconv3_pyr (forward, folded coefficients bn_stride apart, taps w_stride apart) and
    mmd_pwconv_fwd_pyr(_bf16) (weights and bias w_stride apart; every group's rows per level are whole 32-row tiles of the skinny kernel)
    against the two nets evaluated separately in float64; flip / dw_grad / in_stats under a group and a level that breaks the tile condition
    return MMD_EINVAL and write nothing; the group is cleared in a finally.  Level 1 (64 valid rows) ends in two 32-row tiles of padding
    rows: their group index lies past the last net and must be clamped (pw_gemm_body / pw_gemm_skinny), or they load w and bias from beyond
    the parameter buffer"""
    assert R.group_tile_rows(R.pyr_of("pg"), 112, 36) == 32
    _grouped("grouped")


# ------------------------------------------------------------------------------------------------ refusals
@guarded
def _refusals(_):
    P, C, N = R.pyr_of("p3"), 16, 8
    f = lambda *s: torch.full(s, 0.25, device=DEV)
    dd = lambda *s: torch.ones(*s, dtype=D, device=DEV)
    x, w, co, n = f(P.Mt, C), f(9, C), f(8 * C), None
    y, dwg, sums = Out((P.Mt, C), "sent"), Out((9, C), torch.ones(9, C)), Out((16 * C,), torch.ones(16 * C), D)
    desc = P.desc()
    dw = lambda *a: _einval("mmd_dwconv3_pyr", *a)
    dw(x, w, y.t, desc, 6, 0, n, n, 0, n, n, n, 0, n, n, n, 0, n, n, n, n)                                   # C & 3
    dw(x, w, y.t, desc, C, 0, n, n, 0, n, n, n, 0, x, n, n, 0, dwg.t, n, n, n)                               # dw_grad without flip
    dw(x, w, y.t, desc, C, 1, n, n, 0, n, n, n, 0, n, n, n, 0, dwg.t, n, n, n)                               # dw_grad without wg_x
    dw(x, w, y.t, desc, C, 1, n, n, 0, n, n, n, C, x, co, co, 1, n, co, co, sums.t)                          # bn_sums without dw_grad
    dw(x, w, y.t, desc, C, 1, n, n, 0, n, n, n, C, x, co, co, 1, dwg.t, n, co, sums.t)                       # bn_sums without wg_mean
    dw(x, w, y.t, desc, C, 1, n, n, 0, n, n, n, C, x, co, co, 0, dwg.t, co, co, sums.t)                      # bn_sums without swish
    dw(x, w, y.t, desc, C, 0, co, co, 1, dd(16 * C), co, co, C, n, n, n, 0, n, n, n, n)                      # in_stats together with in_scale
    six = (ctypes.c_int * 14)(6, 1, *([2, 2] * 6))
    zero = (ctypes.c_int * 6)(2, 1, 2, 2, 0, 3)
    for bad in (six, zero):                                                                                   # n > 5; a zero-sized level
        dw(x, w, y.t, bad, C, 0, n, n, 0, n, n, n, 0, n, n, n, 0, n, n, n, n)
        _einval("mmd_dwconv3_pyr_bwd_weight", x, x, dwg.t, bad, C, n, n, 0, 0)
        _einval("mmd_pwconv_fwd_pyr", x, f(N, C), y.t, bad, C, N, n, 0, n, 0, 0, n)
        _einval("mmd_bn_bwd_reduce_pyr", x, x, co, co, co, co, 0, bad, C, y.t, sums.t, C)
        _einval("mmd_bn_bwd_apply_pyr", x, x, co, co, co, sums.t, bad, C, y.t, n, n, C, n, n, 0)
        _einval("mmd_pyr_add_bnsums", x, x, n, y.t, bad, C, n, n, n, n)
        _einval("mmd_slice_rows_pyr", x, y.t, bad, C, P.Mt * C, (ctypes.c_longlong * 6)(*([0] * 6)))
    _einval("mmd_pwconv_fwd_pyr", x, f(N, C), y.t, desc, C, N, n, 0, n, 0, 64, n)                            # y_batch_stride without y_off_lev
    _einval("mmd_pwconv_fwd_pyr_bf16", x, f(N, C), y.t, desc, C, N, n, 0, n, 0, 64, n)
    _einval("mmd_bn_bwd_apply_pyr", x, x, co, co, co, sums.t, desc, C, y.t, co, n, C, n, n, 0)               # dgamma without dbeta
    zs = ptrs([x[:P.rows[0]], None, None], 3)
    _einval("mmd_pyr_add_bnsums", x, x, n, y.t, desc, C, zs, ptrs([co, None, None], 3), ptrs([co, None, None], 3), ptrs([None, None, None], 3))   # z[l] but no sums[l]
    torch.cuda.synchronize()
    assert bool((y.get() == SENT).all()) and bool((dwg.get() == 1).all()) and bool((sums.get() == 1).all())


def test_refusals_return_einval_and_write_nothing():
    """the MMD_EINVAL contracts read off the entry points: C & 3; dw_grad without flip or wg_x; bn_sums without dw_grad / wg_mean / swish;
    in_stats together with in_scale; y_batch_stride without y_off_lev; n > 5; a zero-sized level; dgamma without dbeta; a level with z[l] but
    no sums[l] - each returns -22 on the host and leaves every output as it was"""
    _refusals("refusals")
