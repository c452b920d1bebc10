"""GPU: the depthwise kernels of csrc/dwconv.hip (mmd_dwconv_fwd, mmd_dwconv_bwd_data, mmd_dwconv_bwd_data_bn1, mmd_dwconv_bwd_weight)
against the float64 references of tests/dw_ref.py, through the C ABI, on the case table dw_ref.DW_CASES - one entry per branch of the host
dispatch (test_dw_ref_cpu.py proves through dw_ref.route that every branch is reached).

Every comparison is per element: |got_i - ref64_i| <= K * 2^-24 * A_i + tiny, A_i the magnitude the reference reports for that element
and K the family's constant of dw_ref (calibrated on the CPU by test_dw_ref_cpu.py, never on these kernels).  Every output lies in
front of 16 guard rows of a sentinel that must survive; it is pre-filled with NaN where the kernel must overwrite (y, dx) and with
non-zero values where it must accumulate (stats, bn_sums, dw, dw_grad, pool, q_dgamma / q_dbeta).  A slotted workspace is asserted to be
in use by dw_ref.route and must be all zero afterwards.  Each check prints `DW64 <family> <case> <worst err / (2^-24 A)> (K)` before it
asserts.  The float64 references run on the GPU in torch (plain shifted multiply-adds: nothing of the library under test)."""
import math
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from mm_distillnet_amd import _lib

import dw_ref as R

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

    def get(self):
        assert self.guard_ok(), "guard rows behind the output were written"
        return self.t


def judge(family, label, got, ref, A):
    K = R.K_BY_FAMILY[family]
    r = R.ratio(got, ref, A)
    print("DW64 %-10s %-44s %8.3f  (K %.0f)" % (family, label, r, K))
    assert r <= K, "%s %s: err / (2^-24 A) = %.3f > K = %.1f" % (family, label, r, K)


def judge_all(case, label, got, ref):
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    for name in got:
        judge(R.FAMILY[(case["entry"], name)], "%s %s" % (label, name), got[name], *ref[name])


def workspace(slots, C, rec):
    """the slot workspace of a call that passes ws_slots = slots: route must say it is used"""
    if not slots:
        return None
    assert rec["slotted"], "the case passes a workspace the dispatch would not use: %s" % (rec,)
    return Out((slots, 2 * C), torch.zeros(slots, 2 * C), D)


def ws_left_zero(ws):
    assert ws is None or bool((ws.get() == 0).all()), "the slot workspace is not left zero"


def same_as_direct(slotted, direct, what):
    """slotted and direct sums: equal to 1e-12 of the largest (as test_slotted_bn_sums_match_direct)"""
    assert float((slotted - direct).abs().max()) <= 1e-12 * float(direct.abs().max()), what


def fwd_call(case, mode, dev, inp, slots, ws):
    B, H, W, C = case["shape"]
    k, s = case["k"], case["s"]
    pro, epi, _ = mode
    sums, out = R.EPI_FLAGS[epi]
    full = out and epi != "3a"
    bn = dev["bn"]
    OH, OW = R.same_pad_lo(H, k, s)[0], R.same_pad_lo(W, k, s)[0]
    y = Out((B, OH, OW, C), "nan")
    st = Out((2 * C,), inp["stats0"], D) if sums else None
    pool = Out((B, C), inp["pool0"], torch.int64) if full else None
    given = pro in ("given", "affine")
    live = pro == "live"
    call("mmd_dwconv_fwd", dev["x"], dev["w"], y.t, B, H, W, C, k, s, bn["scale"] if given else None, bn["shift"] if given else None,
         1 if pro in ("given", "live", "act") else 0, bn["stats"] if live else None, bn["gamma"] if live else None, bn["beta"] if live else None,
         bn["count"] if live else 0, dev["osc"] if full else None, dev["osh"] if full else None, 1 if out else 0, st.t if sums else None,
         pool.t if full else None, ws.t if ws is not None else None, slots)
    got = {"y": y.get()}
    if sums:
        got["stats"] = st.get()
    if full:
        got["pool"] = pool.get().double() / R.Q36
    return got


def bwd_data_call(case, mode, dev, inp, slots, ws):
    B, H, W, C = case["shape"]
    k, s = case["k"], case["s"]
    kind = mode[0]
    bn = dev["bn"]
    dx = Out((B, H, W, C), "nan")
    sums = Out((2 * C,), inp["sums0"], D) if kind != "plain" else None
    dwg = Out((k * k, C), inp["dw0"]) if kind == "bnwg" else None
    b = [dev["bn_z"], bn["scale"], bn["shift"], bn["mean"], bn["invstd"], sums.t] if sums else [None] * 6
    call("mmd_dwconv_bwd_data", dev["dy"], dev["w"], dx.t, B, H, W, C, k, s, *b, ws.t if ws is not None else None, slots, dwg.t if dwg else None)
    got = {"dx": dx.get()}
    if sums:
        got["bn_sums"] = sums.get()
    if dwg:
        got["dw_grad"] = dwg.get()
    return got


def to_dev(d):
    return {k_: (to_dev(v) if isinstance(v, dict) else (g(v) if isinstance(v, torch.Tensor) else v)) for k_, v in d.items()}


def cases_of(entry):
    return [c["name"] for c in R.DW_CASES if c["entry"] == entry]


# ------------------------------------------------------------------------------------------------ mmd_dwconv_fwd
@pytest.mark.parametrize("name", cases_of("fwd"))
def test_dwconv_fwd(name):
    """every forward case of dw_ref.DW_CASES (its `why` names the kernel instantiation and the geometry it exists for), every mode of its
    list: producer none / given / live / activation only / affine only x epilogue raw / sums / folded + pool / activation only / sums + folded
    + pool.  y, the raw BatchNorm sums and the Q36 pool against float64; slotted launches also against the ws_slots = 0 launch."""
    case = R.CASE[name]
    C = case["shape"][3]
    inp = R.case_inputs(case)
    dev = to_dev(inp)
    t0 = time.time()
    for mode in case["modes"]:
        slots = mode[2]
        rec = R.route_mode(case, mode)
        ref = R.case_ref(case, mode, inp, D, DEV)
        ws = workspace(slots, C, rec)
        got = fwd_call(case, mode, dev, inp, slots, ws)
        judge_all(case, "%s %s" % (name, R.mode_label(mode)), got, ref)
        ws_left_zero(ws)
        if slots:
            direct = fwd_call(case, mode, dev, inp, 0, None)
            same_as_direct(got["stats"], direct["stats"], "slotted and direct sums differ")
            assert torch.equal(got["y"], direct["y"])
    torch.cuda.synchronize()
    print("DW64 time %s %.2f s" % (name, time.time() - t0))


# ------------------------------------------------------------------------------------------------ mmd_dwconv_bwd_data
@pytest.mark.parametrize("name", cases_of("bwd_data"))
def test_dwconv_bwd_data(name):
    """every input-gradient case: plain, with the `bz` sums of the consuming BatchNorm(+swish) backward, and with the conv's weight gradient
    riding along; stride 1 (rows and tile kernels, flipped taps) and stride 2 (the two gather kernels: rows per block 2 and 4, clamped to
    H, slotted sums)."""
    case = R.CASE[name]
    C = case["shape"][3]
    inp = R.case_inputs(case)
    dev = to_dev(inp)
    t0 = time.time()
    for mode in case["modes"]:
        slots = mode[1]
        rec = R.route_mode(case, mode)
        ref = R.case_ref(case, mode, inp, D, DEV)
        ws = workspace(slots, C, rec)
        got = bwd_data_call(case, mode, dev, inp, slots, ws)
        judge_all(case, "%s %s" % (name, R.mode_label(mode)), got, ref)
        ws_left_zero(ws)
        if slots:
            direct = bwd_data_call(case, mode, dev, inp, 0, None)
            same_as_direct(got["bn_sums"], direct["bn_sums"], "slotted and direct sums differ")
            assert torch.equal(got["dx"], direct["dx"])
    torch.cuda.synchronize()
    print("DW64 time %s %.2f s" % (name, time.time() - t0))


# ------------------------------------------------------------------------------------------------ mmd_dwconv_bwd_data_bn1
@pytest.mark.parametrize("name", cases_of("bn1"))
def test_dwconv_bwd_data_bn1(name):
    """the BatchNorm-1 (+swish, gate, pooled term) backward evaluated in the prologue: dx, the BatchNorm-0 sums, the conv's weight gradient
    and q_dgamma / q_dbeta (present: accumulated on a non-zero pre-fill; null) with a gate and an added term per image."""
    case = R.CASE[name]
    B, H, W, C = case["shape"]
    k = case["k"]
    inp = R.case_inputs(case)
    dev = to_dev(inp)
    bn, q = dev["bn"], dev["q"]
    for mode in case["modes"]:
        ref = R.case_ref(case, mode, inp, D, DEV)
        dx, sums, dwg = Out((B, H, W, C), "nan"), Out((2 * C,), inp["sums0"], D), Out((k * k, C), inp["dw0"])
        dga, dbe = (Out((C,), inp["dgamma0"]), Out((C,), inp["dbeta0"])) if mode else (None, None)
        call("mmd_dwconv_bwd_data_bn1", dev["g1"], dev["z1"], dev["w"], dx.t, B, H, W, C, k, q["scale"], q["shift"], q["mean"], q["invstd"],
             dev["q_sums"], inp["q_count"], dev["gate"], dev["add"], dga.t if mode else None, dbe.t if mode else None,
             dev["bn_z"], bn["scale"], bn["shift"], bn["mean"], bn["invstd"], sums.t, None, 0, dwg.t)
        got = {"dx": dx.get(), "bn_sums": sums.get(), "dw_grad": dwg.get()}
        if mode:
            got["q_dgamma"], got["q_dbeta"] = dga.get(), dbe.get()
        judge_all(case, "%s dgamma-%s" % (name, R.mode_label(mode)), got, ref)


def test_dwconv_bwd_data_bn1_refuses_fewer_than_64_channels():
    """C = 60: -22 on the host, nothing written"""
    B, H, W, C, k = 2, 5, 6, 60, 3
    f = lambda *s: torch.full(s, 0.25, device=DEV)
    dx, sums, dwg = Out((B, H, W, C), "nan"), Out((2 * C,), torch.ones(2 * C), D), Out((9, C), torch.ones(9, C))
    with pytest.raises(RuntimeError, match="status -22"):
        call("mmd_dwconv_bwd_data_bn1", f(B, H, W, C), f(B, H, W, C), f(9, C), dx.t, B, H, W, C, k, f(C), f(C), f(C), f(C),
             torch.ones(2 * C, dtype=D, device=DEV), B * H * W, f(B, C), f(B, C), None, None, f(B, H, W, C), f(C), f(C), f(C), f(C), sums.t, None, 0, dwg.t)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx.get()).all()) and bool((sums.get() == 1).all()) and bool((dwg.get() == 1).all())


# ------------------------------------------------------------------------------------------------ mmd_dwconv_bwd_weight
@pytest.mark.parametrize("name", cases_of("bwd_weight"))
def test_dwconv_bwd_weight(name):
    """the tile form for all four (k, s) with nsplit on both clamps, and the row-streaming form (rh 5 on 641 rows, rh 4, rh = H = 3), with
    and without the producer transform; dw is pre-filled (the kernels accumulate)."""
    case = R.CASE[name]
    B, H, W, C = case["shape"]
    k, s = case["k"], case["s"]
    inp = R.case_inputs(case)
    dev = to_dev(inp)
    bn = dev["bn"]
    t0 = time.time()
    for mode in case["modes"]:
        ref = R.case_ref(case, mode, inp, D, DEV)
        dw = Out((k * k, C), inp["dw0"])
        call("mmd_dwconv_bwd_weight", dev["x"], dev["dy"], dw.t, B, H, W, C, k, s, bn["scale"] if mode else None, bn["shift"] if mode else None,
             1 if mode else 0)
        judge_all(case, "%s pro-%s" % (name, R.mode_label(mode)), {"dw": dw.get()}, ref)
    torch.cuda.synchronize()
    print("DW64 time %s %.2f s" % (name, time.time() - t0))


# ------------------------------------------------------------------------------------------------ group mode of mmd_dwconv_fwd
@pytest.mark.parametrize("name,shape,k,s,pro,why", R.GROUP_CASES)
def test_dwconv_fwd_group_mode(name, shape, k, s, pro, why):
    """mmd_set_group(3 nets, 2 images each): image b reads the taps of net b // 2 w_stride floats apart and its folded coefficients
    bn_stride floats apart; each image against the float64 reference with its own net's parameters.  The descriptor is set, read and
    cleared on the calling thread (tests/test_gpu_net.py), the clear returns 0 (a launch honoured it)."""
    B, H, W, C = shape
    inp = R.group_inputs(shape, k, s)
    ref = R.group_ref(shape, k, s, pro, inp, D, DEV)
    dev = to_dev(inp)
    OH, OW = R.same_pad_lo(H, k, s)[0], R.same_pad_lo(W, k, s)[0]
    y, pool = Out((B, OH, OW, C), "nan"), Out((B, C), inp["pool0"], torch.int64)
    given = pro == "given"
    dll = _lib.LIB.load()
    assert dll.mmd_set_group(R.GROUP_N, R.GROUP_IMAGES, inp["w_stride"], inp["bn_stride"]) == 0
    try:
        call("mmd_dwconv_fwd", dev["x"], dev["wbuf"], y.t, B, H, W, C, k, s, dev["isc"] if given else None, dev["ish"] if given else None,
             1 if given else 0, None, None, None, 0, dev["osc"], dev["osh"], 1, None, pool.t, None, 0)
    finally:
        rc = dll.mmd_set_group(1, 0, 0, 0)
    assert rc == 0
    judge("conv", name + " y", y.get(), *ref["y"])
    judge("pool", name + " pool", pool.get().double() / R.Q36, *ref["pool"])
