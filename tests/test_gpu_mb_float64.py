"""GPU: the frozen MBConv front half (mmd_mbconv_expand_dw_fwd, grouped nets included), the fused expand backward
(mmd_mbconv_expand_bwd_fused) and the stem kernels (mmd_stem_conv_fwd, mmd_stem_conv_bwd_weight, mmd_stem_conv_bwd_weight_bn, mmd_stem_im2col)
against the float64 references of tests/mb_ref.py, through the C ABI, on the case tables of mb_ref (test_mb_ref_cpu.py proves through
mb_ref.route that every instantiation and edge is reached, and the references against torch).

Every comparison is per element: |got_i - ref64_i| <= K * 2^-24 * A_i + tiny, A_i the magnitude the reference reports for that element and K
the family's constant of mb_ref (calibrated on the CPU by test_mb_ref_cpu.py, never on these kernels); mmd_stem_im2col is compared with
torch.equal.  Every output lies in front of 16 guard rows of a sentinel that must survive; it is pre-filled with NaN where the kernel must
overwrite and with non-zero values where it must accumulate; the stem weight gradient's workspace is filled with NaN before every call.
Each check prints `MB64 <family> <case> <worst err / (2^-24 A)> (K)` before it asserts.  The float64 references run on the GPU in torch
(matmul, shifted multiply-adds: nothing of the library under test).

Out of scope: the MMD_MBW_TM32 / MMD_MBW_GRID variants, the static bf16-storage entry point of mbx, MMD_STEM_DIRECT's direct kernel beyond
what the environment happens to select."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from mm_distillnet_amd import _lib

import mb_ref as R
from pw_ref import GPU_ERROR          # the list of GPU errors met (shared: after one, no module launches anything more)

DEV = "cuda"
D, S32 = torch.float64, torch.float32
NAN = "nan"
ISENT = -(7 << 58)


def gpu_test(fn):
    """nothing is launched after a GPU error; a launch or runtime error of this test (not a refusal) is recorded for the tests that follow"""
    @functools.wraps(fn)
    def run(*a, **k):
        assert not GPU_ERROR, "an earlier test hit a GPU error (%s): not launching anything more" % GPU_ERROR[0]
        try:
            out = fn(*a, **k)
            torch.cuda.synchronize()
            return out
        except RuntimeError as e:
            if "status -22" not in str(e):
                GPU_ERROR.append("%s: %s" % (fn.__name__, str(e)[:200]))
            raise
    return run


call = _lib.call


def g(t):
    return None if t is None else t.detach().contiguous().to(DEV)


class Out:
    """an output tensor of `shape` followed by 16 guard rows; fill: NAN (must be overwritten) or a CPU tensor (must be accumulated on)"""

    def __init__(self, shape, fill, dtype=S32):
        self.n = math.prod(shape)
        self.sent = ISENT if dtype == torch.int64 else R.SENTINEL
        self.buf = torch.full((self.n + 16 * shape[-1],), self.sent, dtype=dtype, device=DEV)
        self.t = self.buf[:self.n].view(shape)
        if isinstance(fill, str):
            self.t.fill_(float("nan"))
        else:
            self.t.copy_(fill.to(dtype))

    def get(self):
        assert bool((self.buf[self.n:] == self.sent).all()), "guard rows behind the output were written"
        return self.t

    def untouched(self):
        return bool(torch.isnan(self.get()).all())


def judge(kind, label, name, got, ref):
    fam = R.FAMILY[(kind, name)]
    K = R.K_BY_FAMILY[fam]
    r = R.ratio(got, *ref)
    print("MB64 %-10s %-56s %8.3f  (K %.0f)" % (fam, "%s %s" % (label, name), r, K))
    assert r <= K, "%s %s %s: err / (2^-24 A) = %.3f > K = %.1f" % (fam, label, name, r, K)


def judge_all(kind, label, got, ref):
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    for name in sorted(got):
        judge(kind, label, name, got[name], ref[name])


def bits_equal(a, b):
    return torch.equal(a.view(torch.int32) if a.dtype == S32 else a, b.view(torch.int32) if b.dtype == S32 else b)


# ------------------------------------------------------------------------------------------------ mbx
def run_mbx(c, dev, pool0, B=None):
    r = R.mbx_route_of(c)
    B = B or c["B"]
    y = Out((B,) + r["out"] + (c["Cmid"],), NAN)
    pool = Out((B, c["Cmid"]), pool0[:B], torch.int64) if pool0 is not None else None
    call("mmd_mbconv_expand_dw_fwd", dev["x"], dev["w0"], dev["sc0"], dev["sh0"], dev["wd"], dev["sc1"], dev["sh1"], y.t, pool.t if pool else None,
         B, c["H"], c["W"], c["Cin"], c["Cmid"], c["k"], c["s"])
    return y, pool


def check_mbx(c, inp, dev):
    """y and the Q36 pool (on a non-zero start) against float64; a second launch bit-identical; pool null leaves y as it was"""
    ref = R.mbx_case_ref(c, inp, D, DEV)
    y, pool = run_mbx(c, dev, inp["pool0"])
    judge_all("mbx", c["name"], {"y": y.get(), "pool": pool.get().double() / R.Q36}, ref)
    y2, pool2 = run_mbx(c, dev, inp["pool0"])
    assert bits_equal(y.get(), y2.get()) and torch.equal(pool.get(), pool2.get()), "two launches differ"
    y3, _ = run_mbx(c, dev, None)
    assert bits_equal(y.get(), y3.get()), "y depends on the pool argument"


@pytest.mark.parametrize("name", [c["name"] for c in R.MBX_CASES])
@gpu_test
def test_mbx_forward(name):
    """mmd_mbconv_expand_dw_fwd in all 24 instantiations (NK = Cin / 4 x (k, s); float4 and float2 x fragments), on sub-tile maps (H = 1,
    W = 1), exact tiles, ragged multi-tile maps, odd and even sizes at stride 2, grids of 1, < 8, a multiple of 8 and neither (the XCD swizzle),
    |shift0| = 3 (the halo is 0, not swish(BN0(0))), BatchNorm-1 all negative"""
    c = R.MBX[name]
    inp = R.mbx_inputs(c)
    check_mbx(c, inp, R._to(inp, S32, DEV))


@pytest.mark.parametrize("name", [c["name"] for c in R.MBX_GROUP_CASES])
@gpu_test
def test_mbx_forward_grouped_nets(name):
    """mmd_set_group(3 nets, 2 images each): image b reads w0 / wd of net b // 2 w_stride floats apart and the four BatchNorm vectors bn_stride
    floats apart; a B that is not n * images is refused; the group is cleared in a finally and the clear returns 0"""
    c = R.MBX[name]
    inp = R.mbx_inputs(c)
    dev = R._to(inp, S32, DEV)
    dll = _lib.LIB.load()
    refused = 0
    assert dll.mmd_set_group(R.GROUP_N, R.GROUP_IMAGES, inp["w_stride"], inp["bn_stride"]) == 0
    try:
        check_mbx(c, inp, dev)
        yb = Out((c["B"] - 1,) + R.mbx_route_of(c)["out"] + (c["Cmid"],), NAN)
        try:
            call("mmd_mbconv_expand_dw_fwd", dev["x"], dev["w0"], dev["sc0"], dev["sh0"], dev["wd"], dev["sc1"], dev["sh1"], yb.t, None,
                 c["B"] - 1, c["H"], c["W"], c["Cin"], c["Cmid"], c["k"], c["s"])
        except RuntimeError as e:
            refused += "status -22" in str(e)
    finally:
        rc = dll.mmd_set_group(1, 0, 0, 0)
    assert rc == 0
    torch.cuda.synchronize()
    assert refused == 1 and yb.untouched()


@gpu_test
def test_mbx_refusals_leave_the_output_untouched():
    """unsupported (Cin, Cmid, k, s) and null pointers return -22 (through the library handle directly) and write nothing"""
    dll = _lib.LIB.load()
    B, H, W = 2, 8, 8
    f = lambda *s: torch.full(s, 0.25, device=DEV)
    st = _lib.stream_ptr()
    for Cin, Cmid, k, s in R.MBX_REFUSED:
        assert dll.mmd_mbconv_expand_dw_supported(Cin, Cmid, k, s) == 0
        Cm = max(Cmid, 48)
        y, pool = Out((B, H, W, Cm), NAN), Out((B, Cm), torch.ones(B, Cm), torch.int64)
        ts = [f(B, H, W, max(Cin, 4)), f(Cm, max(Cin, 4)), f(Cm), f(Cm), f(k * k, Cm), f(Cm), f(Cm)]
        rc = dll.mmd_mbconv_expand_dw_fwd(*[t.data_ptr() for t in ts], y.t.data_ptr(), pool.t.data_ptr(), B, H, W, Cin, Cmid, k, s, st)
        torch.cuda.synchronize()
        assert rc == -22 and y.untouched() and bool((pool.get() == 1).all())
    Cin, Cm = 16, 48
    assert dll.mmd_mbconv_expand_dw_supported(Cin, Cm, 3, 1) == 1
    ts = [f(B, H, W, Cin), f(Cm, Cin), f(Cm), f(Cm), f(9, Cm), f(Cm), f(Cm)]
    for i in range(8):
        y, pool = Out((B, H, W, Cm), NAN), Out((B, Cm), torch.ones(B, Cm), torch.int64)
        ptrs = [t.data_ptr() for t in ts] + [y.t.data_ptr()]
        ptrs[i] = None
        rc = dll.mmd_mbconv_expand_dw_fwd(*ptrs, pool.t.data_ptr(), B, H, W, Cin, Cm, 3, 1, st)
        torch.cuda.synchronize()
        assert rc == -22 and y.untouched() and bool((pool.get() == 1).all()), i


# ------------------------------------------------------------------------------------------------ mbw
@pytest.mark.parametrize("name", [c["name"] for c in R.MBW_CASES])
@gpu_test
def test_mbw_expand_backward(name):
    """mmd_mbconv_expand_bwd_fused in its four instantiations at M = 1, TM - 1, TM, TM + 1, a ragged few tiles and just past cap * TM (blocks
    walk a second tile; the last is ragged): dx (NaN pre-fill / residual in place / a separate residual), dw, dgamma and dbeta on non-zero
    starts (or null), the upstream sums (off / without / with xs_mul_b, 35 rows per image: several images inside a tile) on a non-zero start,
    count != M, `sums` the reference's own float64 numbers"""
    c = R.MBW[name]
    M, Cin, C = c["M"], c["Cin"], c["Cmid"]
    inp = R.mbw_inputs(c)
    d64 = R._to(inp, D, DEV)
    sums = R.mbw_case_sums(d64)
    ref = R.mbw_case_ref(c, d64, sums)
    del d64
    dev = R._to(inp, S32, DEV)
    dll = _lib.LIB.load()
    assert dll.mmd_mbconv_expand_bwd_supported(Cin, C) == R.mbw_supported(Cin, C)
    dx = Out((M, Cin), inp["res"] if c["res"] == "alias" else NAN)
    dw, dg, db, xs = Out((C, Cin), inp["dw0"]), Out((C,), inp["dgamma0"]), Out((C,), inp["dbeta0"]), Out((2 * Cin,), inp["xs0"], D)
    res = {"none": None, "alias": dx.t, "sep": dev["res"]}[c["res"]]
    on = c["xs"] != "off"
    call("mmd_mbconv_expand_bwd_fused", dev["g0"], dev["z0"], dev["x"], dev["w"], dx.t, res, dw.t, M, Cin, C, dev["scale"], dev["shift"], dev["mean"],
         dev["invstd"], sums, inp["count"], dg.t if c["dsum"] else None, db.t if c["dsum"] else None, dev["xs_z"] if on else None,
         dev["xs_mean"] if on else None, dev["xs_invstd"] if on else None, dev["xs_mul_b"] if c["xs"] == "mulb" else None, R.XS_RPI,
         xs.t if on else None)
    got = {"dx": dx.get(), "dw": dw.get()}
    if c["dsum"]:
        got.update(dgamma=dg.get(), dbeta=db.get())
    else:
        assert torch.equal(dg.get().cpu(), inp["dgamma0"]) and torch.equal(db.get().cpu(), inp["dbeta0"])
    if on:
        got["xs_sums"] = xs.get()
    else:
        assert torch.equal(xs.get().cpu(), inp["xs0"])
    judge_all("mbw", name, got, ref)


@gpu_test
def test_mbw_refusals():
    """dgamma without dbeta, xs_z without xs_sums and an unsupported pair return -22 and write nothing"""
    M, Cin, C = 70, 16, 96
    f = lambda *s: torch.full(s, 0.25, device=DEV)

    def attempt(Cin_, C_, dgamma, dbeta, xs_z, xs_sums):
        dx, dw = Out((M, Cin_), NAN), Out((C_, Cin_), torch.ones(C_, Cin_))
        with pytest.raises(RuntimeError, match="status -22"):
            call("mmd_mbconv_expand_bwd_fused", f(M, C_), f(M, C_), f(M, Cin_), f(C_, Cin_), dx.t, None, dw.t, M, Cin_, C_, f(C_), f(C_), f(C_), f(C_),
                 torch.ones(2 * C_, dtype=D, device=DEV), M, dgamma, dbeta, xs_z, f(Cin_), f(Cin_), None, 1, xs_sums)
        torch.cuda.synchronize()
        assert dx.untouched() and bool((dw.get() == 1).all())
    attempt(Cin, C, f(C), None, None, None)
    attempt(Cin, C, None, f(C), None, None)
    attempt(Cin, C, None, None, f(M, Cin), None)
    attempt(16, 144, None, None, None, None)
    attempt(40, 240, None, None, None, None)


# ------------------------------------------------------------------------------------------------ stem forward
@pytest.mark.parametrize("name", [c["name"] for c in R.STEM_FWD_CASES])
@gpu_test
def test_stem_forward(name):
    """mmd_stem_conv_fwd: Cin 1 / 2 / 3 / 8 / 9 (nkl 2 / 3 / 4 / 1 / 3), every Cout, images down to 2 x 2 and 1 x 1, M % 128 zero and not;
    the raw output with the BatchNorm sums on a non-zero start, the folded epilogue with act 0 and 1; one launch past MMD_STATS_DEPTH row tiles
    with a slot workspace that must be zero afterwards"""
    c = R.STEM_FWD[name]
    B, Cin, H, W, Kp, Cout, slots = (c[k] for k in ("B", "Cin", "H", "W", "Kp", "Cout", "slots"))
    inp = R.stem_fwd_inputs(c)
    dev = R._to(inp, S32, DEV)
    for mode in R.STEM_FWD_MODES:
        r = R.stem_fwd_route_of(c, mode)
        ref = R.stem_fwd_case_ref(c, mode, inp, D, DEV)
        y, st = Out((r["M"], Cout), NAN), Out((2 * Cout,), inp["stats0"], D)
        ws = torch.zeros(slots * 2 * Cout, dtype=D, device=DEV) if slots else None
        stats = mode == "stats"
        call("mmd_stem_conv_fwd", dev["x"], dev["w"], y.t, B, Cin, H, W, Kp, Cout, None if stats else dev["osc"], None if stats else dev["osh"],
             1 if mode == "fold1" else 0, st.t if stats else None, ws if stats else None, slots if stats else 0)
        got = {"y": y.get()}
        if stats:
            got["stats"] = st.get()
            if slots:
                assert r["slotted"] and bool((ws == 0).all()), "the slot workspace is not zero after the launch"
        else:
            assert torch.equal(st.get().cpu(), inp["stats0"])
        judge_all("stem_fwd", "%s %s %s" % (name, mode, r["kernel"]), got, ref)


@gpu_test
def test_stem_forward_refusals():
    B, Cin, H, W = 2, 3, 8, 8
    f = lambda *s: torch.full(s, 0.25, device=DEV)
    for Kp, Cout, shift in ((28, 36, True), (28, 32, False), (24, 32, True)):
        y = Out((B * 16, Cout), NAN)
        with pytest.raises(RuntimeError, match="status -22"):
            call("mmd_stem_conv_fwd", f(B, Cin, H, W), f(Cout, 28), y.t, B, Cin, H, W, Kp, Cout, f(Cout), f(Cout) if shift else None, 1, None, None, 0)
        torch.cuda.synchronize()
        assert y.untouched()


@pytest.mark.parametrize("B,Cin,H,W,Kp", R.IM2COL_CASES)
@gpu_test
def test_stem_im2col_is_the_exact_gather(B, Cin, H, W, Kp):
    x = torch.randn(B, Cin, H, W, generator=R.rng(81, B, Cin, H, W))
    want = R.stem_im2col_ref(x, Kp)
    col = Out(tuple(want.shape), NAN)
    call("mmd_stem_im2col", g(x), col.t, B, Cin, H, W, Kp)
    assert torch.equal(col.get().cpu(), want), "padding columns included"


# ------------------------------------------------------------------------------------------------ stem weight gradient
@pytest.mark.parametrize("name", [c["name"] for c in R.STEM_WG_CASES])
@gpu_test
def test_stem_weight_gradient(name):
    """mmd_stem_conv_bwd_weight and _bn (act 0 / 1, dgamma / dbeta on a non-zero start or null): COT 1 / 2 / 3 with and without Cout < 16 COT,
    one and two tiles per row, pad_l 0 / 1, H down to 2, every boundary of the fold kernel's 64- / 16-strided loop, blocks that walk two tiles;
    dw accumulated on a non-zero start, the padding columns untouched, the workspace full of NaN on entry, two launches bit-identical"""
    c = R.STEM_WG[name]
    B, Cin, H, W, Kp, Cout = (c[k] for k in ("B", "Cin", "H", "W", "Kp", "Cout"))
    dll = _lib.LIB.load()
    assert dll.mmd_stem_conv_bwd_weight_supported(Cin, H, W, Kp, Cout) == 1
    nws = int(dll.mmd_stem_wgrad_ws_floats(Cout))
    assert nws == R.stem_wg_ws_floats(Cout)
    ws = torch.empty(nws, device=DEV)
    inp = R.stem_wg_inputs(c)
    d64, dev = R._to(inp, D, DEV), R._to(inp, S32, DEV)
    for mode in c["modes"]:
        sums = None if mode == "plain" else R.stem_wg_case_sums(d64, R.stem_wg_act(mode))
        ref = R.stem_wg_case_ref(c, mode, d64, sums)
        ds = mode in ("bn0", "bn1")

        def launch():
            dw, dg, db = Out((Cout, Kp), inp["dw0"]), Out((Cout,), inp["dgamma0"]), Out((Cout,), inp["dbeta0"])
            ws.fill_(float("nan"))
            if mode == "plain":
                call("mmd_stem_conv_bwd_weight", dev["x"], dev["dz"], dw.t, ws, B, Cin, H, W, Kp, Cout)
            else:
                call("mmd_stem_conv_bwd_weight_bn", dev["x"], dev["dz"], dev["z"], dw.t, ws, B, Cin, H, W, Kp, Cout, dev["scale"], dev["shift"],
                     dev["mean"], dev["invstd"], sums, inp["count"], R.stem_wg_act(mode), dg.t if ds else None, db.t if ds else None)
            got = {"dw": dw.get()}
            if ds:
                got.update(dgamma=dg.get(), dbeta=db.get())
            else:
                assert torch.equal(dg.get().cpu(), inp["dgamma0"]) and torch.equal(db.get().cpu(), inp["dbeta0"])
            return got
        got = launch()
        r = R.stem_wg_route_of(c, mode)
        judge_all("stem_wg" if mode == "plain" else "stem_wg_bn", "%s %s slots %d" % (name, mode, r["slots"]), got, ref)
        assert torch.equal(got["dw"][:, 9 * Cin:].cpu(), inp["dw0"][:, 9 * Cin:]), "the padding columns received something"
        again = launch()
        assert all(bits_equal(got[k], again[k]) for k in got), "two launches differ"


@gpu_test
def test_stem_weight_gradient_supported_truth_table():
    """mmd_stem_conv_bwd_weight_supported at its edges (OW = 63 / 64 / 65, Cin = 0 / 8 / 9, Cout = 0 / 48 / 52 / 6, Kp = 84, H = 1) against
    mb_ref's copy; a refused call returns -22 and leaves dw as it was"""
    dll = _lib.LIB.load()
    for e in R.STEM_WG_EDGES:
        assert dll.mmd_stem_conv_bwd_weight_supported(*e) == R.stem_wg_supported(*e), e
    f = lambda *s: torch.full(s, 0.25, device=DEV)
    ws = torch.empty(int(dll.mmd_stem_wgrad_ws_floats(32)), device=DEV)
    for Cin, H, W, Kp, Cout in ((3, 8, 126, 28, 32), (3, 1, 128, 28, 32), (3, 8, 128, 24, 32)):
        dw = Out((Cout, Kp), torch.ones(Cout, Kp))
        M = 2 * ((H + 1) // 2) * ((W + 1) // 2)
        with pytest.raises(RuntimeError, match="status -22"):
            call("mmd_stem_conv_bwd_weight", f(2, Cin, H, W), f(M, Cout), dw.t, ws, 2, Cin, H, W, Kp, Cout)
        torch.cuda.synchronize()
        assert bool((dw.get() == 1).all())
    dw, dg = Out((32, 28), torch.ones(32, 28)), Out((32,), torch.ones(32))
    M = 2 * 4 * 64
    with pytest.raises(RuntimeError, match="status -22"):          # dgamma without dbeta
        call("mmd_stem_conv_bwd_weight_bn", f(2, 3, 8, 128), f(M, 32), f(M, 32), dw.t, ws, 2, 3, 8, 128, 28, 32, f(32), f(32), f(32), f(32),
             torch.ones(64, dtype=D, device=DEV), M, 1, dg.t, None)
    torch.cuda.synchronize()
    assert bool((dw.get() == 1).all()) and bool((dg.get() == 1).all())
