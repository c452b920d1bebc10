"""GPU: the row-streaming kernels of csrc/elt.hip (BatchNorm finalize / fold / backward, affine+activation, squeeze-excite pools and
FCs, column sums) against the float64 references of tests/elt_ref.py, through the C ABI.

Every comparison is per element: |got_i - ref64_i| <= K * 2^-24 * A_i + tiny, A_i the magnitude the reference reports for that element
and K the family's constant of elt_ref (calibrated on the CPU by test_elt_ref_cpu.py, never on these kernels).  Every output lies in
front of 16 guard rows of a sentinel that must survive; it is pre-filled with NaN where the kernel must overwrite and with non-zero
values where it must accumulate.  Each check prints `ELT64 <family> <case> <worst err / (2^-24 A)>` before it asserts."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from mm_distillnet_amd import _lib

import elt_ref as R

call = _lib.call
DEV = "cuda"
D = torch.float64
ISENT = -(2 ** 40) - 12345


def g(t):
    return None if t is None else t.detach().contiguous().to(DEV)


class Out:
    """an output tensor of `shape` followed by 16 guard rows; fill: 'nan' (must be overwritten) or a CPU tensor (must be accumulated on)"""

    def __init__(self, shape, fill, dtype=torch.float32):
        n = math.prod(shape)
        self.n = n
        sent = ISENT if dtype == torch.int64 else R.SENTINEL
        self.buf = torch.full((n + 16 * shape[-1],), sent, dtype=dtype, device=DEV)
        self.t = self.buf[:n].view(shape)
        self.sent = sent
        if isinstance(fill, str):
            self.t.fill_(float("nan"))
        else:
            self.t.copy_(fill.to(dtype))

    def guard_ok(self):
        return bool((self.buf[self.n:] == self.sent).all())

    def cpu(self):
        assert self.guard_ok(), "guard rows behind the output were written"
        return self.t.cpu()


def judge(family, label, got, ref, A):
    K = R.K_BY_FAMILY[family]
    r = R.ratio(got, ref, A)
    print("ELT64 %-9s %-60s %8.3f  (K %.0f)" % (family, label, r, K))
    assert r <= K, "%s %s: err / (2^-24 A) = %.3f > K = %.1f" % (family, label, r, K)


def live_args(case, coef):
    """(scale, shift, in_stats, in_gamma, in_beta, in_count) of the forward consumers"""
    if coef == "given":
        return g(case["scale"]), g(case["shift"]), None, None, None, 0
    if coef == "live":
        return None, None, g(case["stats"]), g(case["gamma"]), g(case["beta"]), case["stats_count"]
    return None, None, None, None, None, 0


# ------------------------------------------------------------------------------------------------ mmd_affine_act
@pytest.mark.parametrize("M,C", R.ELT_SHAPES)
def test_affine_act(M, C):
    """rows per block: (1,4) (15,68) (77,36) (257,64) take 64 - (15,68) has fewer rows than the 16 row groups and a one-quad tail chunk
    (C on both sides of 64), (257,64) a second row block of one row; (4091,1028) takes 128 with an M tail and a C tail; (4091,4036)
    takes 256.  Modes per shape (elt_ref.affine_modes): act 0 / 1 / 2 (MMD_ACT_SIGMOID), coefficients null / given / live, rowscale with
    rows_per_image = M // 7 (a ragged last image; 584 divides no rows-per-block value) and res present / absent, and y == z in place."""
    case = R.affine_case(M, C)
    zd, rsd, resd = g(case["z"]), g(case["rowscale"]), g(case["res"])
    for mode in R.affine_modes(M, C):
        act, coef, rs, res, inplace = mode
        ref, A = R.affine_ref(case, mode, D)
        y = Out((M, C), case["z"] if inplace else "nan")
        sc, sh, st, ga, be, cnt = live_args(case, coef)
        call("mmd_affine_act", y.t if inplace else zd, sc, sh, st, ga, be, cnt, act, rsd if rs else None, case["rpi"] if rs else 0,
             resd if res else None, y.t, M, C)
        judge("affine", "M%d C%d act%d %s rs%d res%d inplace%d" % (M, C, act, coef, rs, res, inplace), y.cpu(), ref, A)


# ------------------------------------------------------------------------------------------------ mmd_bn_bwd_apply
@pytest.mark.parametrize("M,C", R.ELT_SHAPES)
def test_bn_bwd_apply(M, C):
    """the same shapes and rows-per-block branches as test_affine_act (64: the first four, 128: (4091,1028), 256: (4091,4036)).
    Modes: g given (act 0, no modifiers) and g recomputed from g_in with swish and all three per-image modifiers; dgamma / dbeta
    pre-filled non-zero and null; count = 2M + 1 != M."""
    case = R.apply_case(M, C)
    dev = {k: g(case[k]) for k in ("g_in", "z", "mean", "invstd", "gamma", "sums", "scale", "shift", "mul_bc", "mul_b", "add_bc")}
    for mode in R.apply_modes(M, C):
        recompute, grads = mode
        ref = R.apply_ref(case, mode, D)
        dz = Out((M, C), "nan")
        dga, dbe = (Out((C,), case["dgamma0"]), Out((C,), case["dbeta0"])) if grads else (None, None)
        mods = (dev["scale"], dev["shift"], 1, dev["mul_bc"], dev["mul_b"], dev["add_bc"], case["rpi"]) if recompute else \
            (None, None, 0, None, None, None, 0)
        call("mmd_bn_bwd_apply", dev["g_in"], dev["z"], dev["mean"], dev["invstd"], dev["gamma"], dev["sums"], case["count"], dz.t,
             dga.t if grads else None, dbe.t if grads else None, M, C, *mods)
        label = "M%d C%d recompute%d grads%d" % (M, C, recompute, grads)
        judge("apply", label + " dz", dz.cpu(), *ref["dz"])
        if grads:
            judge("apply", label + " dgamma", dga.cpu(), *ref["dgamma"])
            judge("apply", label + " dbeta", dbe.cpu(), *ref["dbeta"])


# ------------------------------------------------------------------------------------------------ mmd_bn_bwd_reduce
@pytest.mark.parametrize("M,C,B,rpi,slots", R.REDUCE_CASES)
def test_bn_bwd_reduce(M, C, B, rpi, slots):
    """rows per block of the reducing kernel: (1,4) (15,68) (500,48) take 64; (4097,20) doubles to 128 (65 row blocks of 64 > 64);
    (16385,20) doubles twice to 256; (33000,8) with ws_slots = 8 takes the slotted sums (129 row blocks of 256 > MMD_STATS_DEPTH):
    the workspace must be left zero and the sums must equal the ws_slots = 0 call to within K.  Modes (elt_ref.reduce_modes): act 0 / 1,
    each of mul_bc / mul_b / add_bc alone and all together, g_out null / given.  Both sums per channel against float64 with
    A = |sums0| + sum |g| and |sums0| + sum |g*xhat|; the sums are pre-filled non-zero."""
    case = R.reduce_case(M, C, B, rpi)
    dev = {k: g(case[k]) for k in ("g_in", "z", "scale", "shift", "mean", "invstd", "mul_bc", "mul_b", "add_bc")}
    for mode in R.reduce_modes(M, C):
        act, mods, store = mode
        gref, Ag, sref, As = R.reduce_ref(case, mode, D)
        m = [dev[k] if k in mods else None for k in ("mul_bc", "mul_b", "add_bc")]
        label = "M%d C%d act%d %s gout%d" % (M, C, act, "+".join(mods) or "plain", store)
        got = {}
        for ws_slots in sorted({0, slots}):
            sums = Out((2 * C,), case["sums0"], D)
            gout = Out((M, C), "nan") if store else None
            ws = Out((ws_slots, 2 * C), torch.zeros(ws_slots, 2 * C), D) if ws_slots else None
            call("mmd_bn_bwd_reduce", dev["g_in"], dev["z"], dev["scale"], dev["shift"], dev["mean"], dev["invstd"], act, *m, rpi,
                 gout.t if store else None, sums.t, M, C, ws.t if ws_slots else None, ws_slots)
            got[ws_slots] = sums.cpu()
            judge("reduce", label + " slots%d sums" % ws_slots, got[ws_slots], sref, As)
            if store:
                judge("reduce", label + " slots%d g_out" % ws_slots, gout.cpu(), gref, Ag)
            if ws_slots:
                assert bool((ws.cpu() == 0).all()), "the slot workspace is not left zero"
        if slots:
            judge("reduce", label + " slotted vs plain", got[slots], got[0], As)


# ------------------------------------------------------------------------------------------------ mmd_chan_pool / mmd_chan_pool_bwd
@pytest.mark.parametrize("B,rpi,C", R.POOL_SHAPES)
def test_chan_pool(B, rpi, C):
    """z-split of the rows of an image: (1,1,4) and (3,17,68) run ns = 1 (17 rows: a second trip of the 16-row stride; C = 68: a one-quad
    tail chunk), (2,65,36) ns = 2 with row 64 back in z-block 0, (1,1000,20) ns = 16, (5,200,1028) ns = 4, (16,130,4100) ns = 1 because
    the (channel chunk, image) grid alone has 1040 blocks.  Modes (elt_ref.pool_modes): g null / given, act 0 / 1, coefficients null /
    given / live, out_scale 1 and 1 / rpi; out is pre-filled (the kernel accumulates)."""
    case = R.pool_case(B, rpi, C)
    zd, gd = g(case["z"]), g(case["g"])
    for mode in R.pool_modes(B, rpi, C):
        gg, act, coef, inv = mode
        ref, A = R.pool_ref(case, mode, D)
        out = Out((B, C), case["out0"])
        sc, sh, st, ga, be, cnt = live_args(case, coef)
        call("mmd_chan_pool", zd, sc, sh, st, ga, be, cnt, act, gd if gg else None, out.t, R.f32(1.0 / rpi) if inv else 1.0, B, rpi, C)
        judge("pool", "B%d R%d C%d g%d act%d %s inv%d" % (B, rpi, C, gg, act, coef, inv), out.cpu(), ref, A)


@pytest.mark.parametrize("B,rpi,C", R.POOL_SHAPES)
def test_chan_pool_bwd_all_five_planes(B, rpi, C):
    """the same z-split cases as test_chan_pool (ns 1, 1, 2, 16, 4, 1).  All five planes - sum g*a, sum g*s', sum g*s'*xhat, sum s',
    sum s'*xhat - each against float64 with its own A, on a pre-filled out5."""
    case = R.pool_case(B, rpi, C)
    ref, A = R.pool_bwd_ref(case, D)
    out = Out((5, B, C), case["out5"])
    call("mmd_chan_pool_bwd", g(case["z"]), g(case["scale"]), g(case["shift"]), g(case["mean"]), g(case["invstd"]), g(case["g"]), out.t,
         B, rpi, C)
    got = out.cpu()
    for k in range(5):
        judge("pool_bwd", "B%d R%d C%d plane %d" % (B, rpi, C, k), got[k], ref[k], A[k])


# ------------------------------------------------------------------------------------------------ mmd_colsum
@pytest.mark.parametrize("M,C", R.COLSUM_SHAPES)
def test_colsum(M, C):
    """M = 1, 255, 256 (one full row block), 257 (a second block of one row), 700; C = 4, 36, 68 (tail chunk of one quad), 132 (three
    chunks); out is pre-filled."""
    a, o = R.colsum_case(M, C)
    ref, A = R.colsum(a.double(), o.double())
    out = Out((C,), o)
    call("mmd_colsum", g(a), out.t, M, C)
    judge("colsum", "M%d C%d" % (M, C), out.cpu(), ref, A)


# ------------------------------------------------------------------------------------------------ BatchNorm coefficients
def run_finalize(case, kind):
    C = case["gamma"].numel()
    run, mo = kind != "no_running", kind != "no_mean_out"
    outs = {k: Out((C,), "nan") for k in ("scale", "shift")}
    if mo:
        outs.update({k: Out((C,), "nan") for k in ("mean", "invstd")})
    if run:
        outs.update({"rmean": Out((C,), case["rmean"]), "rvar": Out((C,), case["rvar"])})
    p = lambda k: outs[k].t if k in outs else None
    call("mmd_bn_finalize", g(case["stats"]), case["count"], g(case["gamma"]), g(case["beta"]), p("rmean"), p("rvar"), R.MOMENTUM, R.EPS,
         p("scale"), p("shift"), p("mean"), p("invstd"), C)
    return {k: o.cpu() for k, o in outs.items()}


@pytest.mark.parametrize("kind", R.FINALIZE_KINDS)
@pytest.mark.parametrize("C", R.FINALIZE_WIDTHS)
def test_bn_finalize(C, kind):
    """C = 4, 68 inside one 256-thread block, 260 crosses it.  Channel 0 is constant (var exactly 0), channel 1 constant with var slightly
    negative (clamped), channel 2 has |mean| = 1e3 and std = 1e-2 (C > 2, count > 1).  Kinds: plain; count == 1 (the unbiased-variance
    guard); running_mean / running_var null; mean_out / invstd_out null.  Per channel, relative to the coefficient's own magnitude."""
    case = R.finalize_case(C, kind)
    ref, A = R.finalize_ref(case, kind, D)
    got = run_finalize(case, kind)
    assert set(got) == set(ref) - ({"mean", "invstd"} if kind == "no_mean_out" else set())
    for k in got:
        judge("finalize", "C%d %s %s" % (C, kind, k), got[k], ref[k], A[k])


def test_bn_finalize_all_idle_layer_and_bit_equality():
    """three layers of widths 4, 68, 20 with counts 300, 0 (idle), 1: the idle layer's six outputs keep their values, every layer's
    num_batches_tracked goes up by one, and the active layers equal mmd_bn_finalize bit for bit (count == 1 included)."""
    case = R.finalize_all_case()
    ref, A, nbt_ref = R.finalize_all_ref(case, D)
    tot = sum(R.ALL_WIDTHS)
    off = [sum(R.ALL_WIDTHS[:i]) for i in range(3)]
    per = lambda vals, dt: torch.cat([torch.full((C,), v, dtype=dt) for v, C in zip(vals, R.ALL_WIDTHS)])
    outs = {k: Out((tot,), case["prev"][k]) for k in ("scale", "shift", "mean", "invstd")}
    outs["rmean"], outs["rvar"] = Out((tot,), case["rmean"]), Out((tot,), case["rvar"])
    nbt = Out((3,), case["nbt"], torch.int64)
    call("mmd_bn_finalize_all", g(case["stats"]), g(per(R.ALL_COUNTS, torch.float32)), g(per(off, torch.int32)),
         g(per(R.ALL_WIDTHS, torch.int32)), g(case["gamma"]), g(case["beta"]), outs["rmean"].t, outs["rvar"].t, R.MOMENTUM, R.EPS,
         outs["scale"].t, outs["shift"].t, outs["mean"].t, outs["invstd"].t, tot, nbt.t, 3)
    got = {k: o.cpu() for k, o in outs.items()}
    assert nbt.cpu().tolist() == nbt_ref.tolist()
    for k in got:
        judge("finalize", "all %s" % k, got[k], ref[k], A[k])
    for o, n, C in zip(off, R.ALL_COUNTS, R.ALL_WIDTHS):
        sl = slice(o, o + C)
        if n == 0:
            for k in ("scale", "shift", "mean", "invstd", "rmean", "rvar"):
                keep = case["prev"][k] if k in case["prev"] else case[k]
                assert torch.equal(got[k][sl], keep[sl]), "idle layer: %s was written" % k
        else:
            one = run_finalize({"stats": case["stats"][2 * o:2 * o + 2 * C], "count": n, "gamma": case["gamma"][sl], "beta": case["beta"][sl],
                                "rmean": case["rmean"][sl], "rvar": case["rvar"][sl]}, "plain")
            for k in one:
                assert torch.equal(got[k][sl], one[k]), "layer of %d channels: %s differs from mmd_bn_finalize" % (C, k)


@pytest.mark.parametrize("C", R.FINALIZE_WIDTHS)
def test_bn_fold(C):
    """eval-mode fold; channel 0 has a running variance of 0, channel 1 of 1e-6"""
    case = R.fold_case(C)
    ref, A = R.fold_ref(case, D)
    sc, sh = Out((C,), "nan"), Out((C,), "nan")
    call("mmd_bn_fold", g(case["gamma"]), g(case["beta"]), g(case["rmean"]), g(case["rvar"]), R.EPS, sc.t, sh.t, C)
    judge("finalize", "fold C%d scale" % C, sc.cpu(), ref["scale"], A["scale"])
    judge("finalize", "fold C%d shift" % C, sh.cpu(), ref["shift"], A["shift"])


# ------------------------------------------------------------------------------------------------ squeeze-excite FCs
def judge_all(label, got, ref, names=None):
    for k in (names or got):
        judge("se", "%s %s" % (label, k), got[k], *ref[k])


@pytest.mark.parametrize("B,C,S", R.SE_SHAPES)
def test_se_fc_forward(B, C, S):
    """(1,4,1): one quad, S = 1; (5,16,4); (3,252,5): the last quad of the first 256-channel trip, S no multiple of 4; (3,260,6): a second
    trip of the `lane * 4 ... += 256` loops and a second blockIdx.y; (2,1028,43): five trips, odd S; (2,64,256): the cap S = 256;
    (2,3072,128): SE_MAXC.  From floats, and from the Q36 pool: the integers are a float64 pool (with bits below fp32) * 2^36
    rounded, and the reference uses the rounded integers."""
    case = R.se_case(B, C, S)
    w = [g(case[k]) for k in ("wr", "br", "wet", "be")]
    ref = R.se_fwd_ref(case, D)
    hp, gt = Out((B, S), "nan"), Out((B, C), "nan")
    call("mmd_se_fc_fwd", g(case["pooled"]), *w, hp.t, gt.t, B, C, S)
    judge_all("B%d C%d S%d fwd" % (B, C, S), {"hpre": hp.cpu(), "gate": gt.cpu()}, ref)
    q = (case["pooled64"] * 2.0 ** 36).round().to(torch.int64)
    assert bool((q.double() / 2.0 ** 36 != case["pooled"].double()).any())      # the integers hold bits below fp32: mmd_pool_get rounds
    refq = R.se_fwd_ref(case, D, q.double() / 2.0 ** 36)
    hp, gt = Out((B, S), "nan"), Out((B, C), "nan")
    call("mmd_se_fc_fwd_q", g(q), *w, hp.t, gt.t, B, C, S)
    judge_all("B%d C%d S%d fwd_q" % (B, C, S), {"hpre": hp.cpu(), "gate": gt.cpu()}, refq)


@pytest.mark.parametrize("B,C,S", R.SE_SHAPES)
def test_se_fc_backward_three_forms(B, C, S):
    """the shapes of test_se_fc_forward (C on both sides of 256, S % 4 != 0, S = 256, C = SE_MAXC = 3072).  Form 1: mmd_se_fc_bwd with the
    weight gradients and the BatchNorm-1 sums from pool5; form 2: mmd_se_fc_bwd with dwr == NULL and no sums, then mmd_se_fc_wgrad;
    form 3: mmd_se_fc_bwd_fused, then mmd_se_fc_wgrad_batched over two table entries of different (C, S).  All gradients and the sums
    are pre-filled non-zero; the weight gradients are judged against the float64 sums over the dpe / dpr the launch itself produced."""
    case = R.se_case(B, C, S)
    ref = R.se_bwd_ref(case, D)
    dv = {k: g(case[k]) for k in ("dgate", "gate", "hpre", "pooled", "wr", "wet", "pool5")}
    label = "B%d C%d S%d" % (B, C, S)
    names = ("dwr", "dbr", "dwe", "dbe")

    def data_outs():
        return {"dpe": Out((B, C), "nan"), "dpr": Out((B, S), "nan"), "dpooled": Out((B, C), "nan")}

    def wgrad_ref(o, src=case, g0=None):
        return R.se_wgrad_ref(o["dpe"], o["dpr"], src["hpre"], src["pooled"], g0 or src["g0"], D)

    # form 1
    o, dh = data_outs(), Out((B, S), torch.zeros(B, S))
    gr = [Out(tuple(t.shape), t) for t in case["g0"]]
    sums = Out((2 * C,), case["bn_sums0"], D)
    call("mmd_se_fc_bwd", dv["dgate"], dv["gate"], dv["hpre"], dv["pooled"], dv["wr"], dv["wet"], o["dpe"].t, o["dpr"].t, dh.t, o["dpooled"].t,
         case["scale"], *[x.t for x in gr], B, C, S, dv["pool5"], sums.t)
    got = {k: v.cpu() for k, v in o.items()}
    got["dh"], got["bn_sums"] = dh.cpu(), sums.cpu()
    judge_all(label + " bwd", got, ref)
    judge_all(label + " bwd", dict(zip(names, (x.cpu() for x in gr))), wgrad_ref(got))
    # form 2
    o, dh = data_outs(), Out((B, S), torch.zeros(B, S))
    call("mmd_se_fc_bwd", dv["dgate"], dv["gate"], dv["hpre"], dv["pooled"], dv["wr"], dv["wet"], o["dpe"].t, o["dpr"].t, dh.t, o["dpooled"].t,
         case["scale"], None, None, None, None, B, C, S, None, None)
    got = {k: v.cpu() for k, v in o.items()}
    got["dh"] = dh.cpu()
    judge_all(label + " bwd/nowg", got, ref, ("dpe", "dh", "dpr", "dpooled"))
    gr = [Out(tuple(t.shape), t) for t in case["g0"]]
    call("mmd_se_fc_wgrad", o["dpe"].t, o["dpr"].t, dv["hpre"], dv["pooled"], *[x.t for x in gr], B, C, S)
    judge_all(label + " wgrad", dict(zip(names, (x.cpu() for x in gr))), wgrad_ref(got))
    # form 3
    o = data_outs()
    sums = Out((2 * C,), case["bn_sums0"], D)
    call("mmd_se_fc_bwd_fused", dv["dgate"], dv["gate"], dv["hpre"], dv["wr"], dv["wet"], o["dpe"].t, o["dpr"].t, o["dpooled"].t, case["scale"],
         B, C, S, dv["pool5"], sums.t)
    got = {k: v.cpu() for k, v in o.items()}
    got["bn_sums"] = sums.cpu()
    judge_all(label + " fused", got, ref, ("dpe", "dpr", "dpooled", "bn_sums"))
    aux = case["aux"]
    Ca, Sa = R.SE_AUX
    gr = [Out(tuple(t.shape), t) for t in case["g0"]]
    gra = [Out(tuple(t.shape), t) for t in aux["g0"]]
    ad = {k: g(aux[k]) for k in ("dpe", "dpr", "hpre", "pooled")}
    tab = torch.tensor([[o["dpe"].t.data_ptr(), o["dpr"].t.data_ptr(), dv["hpre"].data_ptr(), dv["pooled"].data_ptr()] + [x.t.data_ptr() for x in gr] + [C, S],
                        [ad[k].data_ptr() for k in ("dpe", "dpr", "hpre", "pooled")] + [x.t.data_ptr() for x in gra] + [Ca, Sa]],
                       dtype=torch.int64, device=DEV)
    call("mmd_se_fc_wgrad_batched", tab, 2, max(C * S, Ca * Sa), B)
    judge_all(label + " batched", dict(zip(names, (x.cpu() for x in gr))), wgrad_ref(got))
    judge_all(label + " batched aux", dict(zip(names, (x.cpu() for x in gra))), wgrad_ref(aux, aux))


def test_se_fc_refusals_write_nothing():
    """S = 257 is refused by every SE entry point and C = 3076 > SE_MAXC by the fused backward: the status is returned on the host before
    any launch (the argument checks at the top of each entry point in elt.hip), and no output is touched."""
    B = 2

    def attempt(C, S, which):
        f = lambda *s: torch.full(s, 0.25, device=DEV)
        outs = [Out(s, "nan") for s in ((B, S), (B, C), (B, C), (B, S), (B, C), (S, C), (S,), (S, C), (C,))]
        sums = Out((2 * C,), torch.ones(2 * C), D)
        hp, gt, dpe, dpr, dpo, dwr, dbr, dwe, dbe = (x.t for x in outs)
        calls = {
            "fwd": ("mmd_se_fc_fwd", f(B, C), f(S, C), f(S), f(S, C), f(C), hp, gt, B, C, S),
            "fwd_q": ("mmd_se_fc_fwd_q", torch.ones(B, C, dtype=torch.int64, device=DEV), f(S, C), f(S), f(S, C), f(C), hp, gt, B, C, S),
            "bwd": ("mmd_se_fc_bwd", f(B, C), f(B, C), f(B, S), f(B, C), f(S, C), f(S, C), dpe, dpr, hp, dpo, 1.0, dwr, dbr, dwe, dbe, B, C, S,
                    f(5, B, C), sums.t),
            "fused": ("mmd_se_fc_bwd_fused", f(B, C), f(B, C), f(B, S), f(S, C), f(S, C), dpe, dpr, dpo, 1.0, B, C, S, f(5, B, C), sums.t),
            "wgrad": ("mmd_se_fc_wgrad", f(B, C), f(B, S), f(B, S), f(B, C), dwr, dbr, dwe, dbe, B, C, S),
        }
        with pytest.raises(RuntimeError):
            call(*calls[which])
        torch.cuda.synchronize()
        for x in outs:
            assert x.guard_ok() and bool(torch.isnan(x.t).all()), "%s C%d S%d wrote an output" % (which, C, S)
        assert bool((sums.cpu() == 1).all())

    for which in ("fwd", "fwd_q", "bwd", "fused", "wgrad"):
        attempt(64, 257, which)
    attempt(3076, 128, "fused")
