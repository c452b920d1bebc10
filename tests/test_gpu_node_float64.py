"""GPU: the BiFPN node kernels of csrc/bifpn.hip (mmd_bifpn_fuse_fwd, mmd_bifpn_node_dw_fwd, mmd_bifpn_node_fwd_fused with and without grouped
nets, mmd_bifpn_node_fwd_fused_train(_lz), mmd_maxpool_same_fwd, mmd_bifpn_node_dw_bwd, mmd_bifpn_node_bwd_full_form, mmd_bifpn_theta_bwd)
against the float64 references of tests/node_ref.py, through the C ABI, on the case table node_ref.NODE_CASES - one entry per branch of the
host dispatch (test_node_ref_cpu.py proves through node_ref.route that every instantiation is reached, and the references against torch).

Every comparison is per element: |got_i - ref64_i| <= K * 2^-24 * A_i + tiny, A_i the magnitude the reference reports for that element and
K the family's constant of node_ref (calibrated on the CPU by test_node_ref_cpu.py, never on these kernels).  Every output lies in front of
16 guard rows of a sentinel that must survive; it is pre-filled with NaN where the kernel must overwrite (y, z, zd, f_out, dz_out, dx and
the gradients with acc = 0) and with non-zero values where it must accumulate (stats, wdot, dw_grad, dgamma / dbeta, operand BatchNorm sums,
the gradients with acc = 1, the pooled operand's scatter target).  Each check prints `NODE64 <family> <case> <worst err / (2^-24 A)> (K)`
before it asserts.  The float64 references run on the GPU in torch (shifted multiply-adds and matmul: nothing of the library under test)."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from mm_distillnet_amd import _lib

import node_ref as R

call = _lib.call
DEV = "cuda"
D = torch.float64
NAN = "nan"


def g(t):
    return None if t is None else t.detach().contiguous().to(DEV)


def to_dev(d):
    return {k_: (to_dev(v) if isinstance(v, dict) else (g(v) if isinstance(v, torch.Tensor) else v)) for k_, v in d.items()}


class Out:
    """an output tensor of `shape` followed by 16 guard rows; fill: NAN (must be overwritten) or a CPU tensor (must be accumulated on)"""

    def __init__(self, shape, fill, dtype=torch.float32):
        self.n = math.prod(shape)
        self.buf = torch.full((self.n + 16 * shape[-1],), R.SENTINEL, dtype=dtype, device=DEV)
        self.t = self.buf[:self.n].view(shape)
        if isinstance(fill, str):
            self.t.fill_(float("nan"))
        else:
            self.t.copy_(fill.to(dtype))

    def get(self):
        assert bool((self.buf[self.n:] == R.SENTINEL).all()), "guard rows behind the output were written"
        return self.t

    def untouched(self):
        return bool(torch.isnan(self.get()).all())


def judge(label, name, got, ref):
    fam = R.FAMILY[name]
    K = R.K_BY_FAMILY[fam]
    r = R.ratio(got, *ref)
    print("NODE64 %-8s %-52s %8.3f  (K %.0f)" % (fam, "%s %s" % (label, name), r, K))
    assert r <= K, "%s %s %s: err / (2^-24 A) = %.3f > K = %.1f" % (fam, label, name, r, K)


def judge_all(label, got, ref):
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    for name in sorted(got):
        judge(label, name, got[name], ref[name])


def ops_of(dev, mode):
    return [dev["in0"], dev["in1"] if mode & 1 else None, dev["up"] if mode & 2 else None, dev["pl"] if mode & 4 else None]


def ptr4(ts):
    """host array of four device pointers (null: that operand is a plain tensor)"""
    return (ctypes.c_void_p * 4)(*[(t.data_ptr() if t is not None else None) for t in ts])


def setup(name):
    case = R.CASE[name]
    inp = R.case_inputs(case)
    return case, inp, to_dev(inp)


# ------------------------------------------------------------------------------------------------ whole-node forward
def run_eval(case, dev, y=None):
    B, H, W, C = case["shape"]
    y = y or Out((B, H, W, C), NAN)
    call("mmd_bifpn_node_fwd_fused", *ops_of(dev, case["mode"]), dev["theta"], dev["w_dw"], dev["w_pw"], dev["bias"], dev["scale"], dev["shift"],
         y.t, B, H, W, C)
    return {"y": y.get()}


def run_train(case, dev, inp, lazy=False):
    B, H, W, C = case["shape"]
    z, zd, st = Out((B, H, W, C), NAN), Out((B, H, W, C), NAN), Out((2 * C,), inp["stats0"], D)
    head = (*ops_of(dev, case["mode"]), dev["theta"], dev["w_dw"], dev["w_pw"], dev["bias"], z.t, zd.t, st.t, B, H, W, C)
    if lazy:
        lz = [dev.get("lz%d" % i) for i in range(4)]
        cnt = (ctypes.c_longlong * 4)(*[(l["count"] if l else 0) for l in lz])
        call("mmd_bifpn_node_fwd_fused_train_lz", *head, ptr4([l and l["stats"] for l in lz]), ptr4([l and l["gamma"] for l in lz]),
             ptr4([l and l["beta"] for l in lz]), cnt)
    else:
        call("mmd_bifpn_node_fwd_fused_train", *head)
    return {"z": z.get(), "zd": zd.get(), "stats": st.get()}


@pytest.mark.parametrize("name", R.cases_of("fwd"))
def test_node_forward_eval_and_train(name):
    """mmd_bifpn_node_fwd_fused (y) and mmd_bifpn_node_fwd_fused_train (z, zd, the BatchNorm sums on a non-zero start) at every width and
    operand set (1 included), on full, ragged, sub-tile and multi-tile maps; theta with zero / negative / very unequal entries; pooled
    operands that are all negative (the padding zero wins the border windows) and all positive"""
    case, inp, dev = setup(name)
    ref = R.case_ref(case, inp, D, DEV)
    got = run_eval(case, dev)
    got.update(run_train(case, dev, inp))
    judge_all(name, got, ref)


@pytest.mark.parametrize("name", R.cases_of("eval"))
def test_node_forward_nopark_by_launch_size(name):
    """mode 2, C = 112: launches of >= 1024 blocks take bifpn_node_fused_kernel<2, false, 112, PK = false>, one image fewer the parked
    kernel; both against the same reference"""
    case, inp, dev = setup(name)
    B, H, W, C = case["shape"]
    assert R.route("eval", B, H, W, C, case["mode"])[3] == (not name.startswith("nopark"))
    judge_all(name, run_eval(case, dev), R.case_ref(case, inp, D, DEV))


@pytest.mark.parametrize("name", R.cases_of("lazy"))
def test_node_forward_lazy_operands(name):
    """mmd_bifpn_node_fwd_fused_train_lz: operands given raw with the live sums of their BatchNorm, against the float64 BatchNorm of the raw
    operand; the pooled operand is transformed inside the image only - its zero padding stays zero and takes part in the max"""
    case, inp, dev = setup(name)
    judge_all(name, run_train(case, dev, inp, lazy=True), R.case_ref(case, inp, D, DEV))


# ------------------------------------------------------------------------------------------------ fusion (+ depthwise) launches
@pytest.mark.parametrize("name", R.cases_of("dw"))
def test_fuse_and_node_dw_forward(name):
    """mmd_bifpn_fuse_fwd and mmd_bifpn_node_dw_fwd (with and without f_out) at C = 48 (ragged chunk), 64, 112, every operand set"""
    case, inp, dev = setup(name)
    B, H, W, C = case["shape"]
    ref = R.case_ref(case, inp, D, DEV)
    ops = ops_of(dev, case["mode"])
    f = Out((B, H, W, C), NAN)
    call("mmd_bifpn_fuse_fwd", *ops, dev["theta"], f.t, B, H, W, C)
    judge(name + " fuse_fwd", "f", f.get(), ref["f"])
    for with_f in (True, False):
        fo, zd = Out((B, H, W, C), NAN), Out((B, H, W, C), NAN)
        call("mmd_bifpn_node_dw_fwd", *ops, dev["theta"], dev["w_dw"], fo.t if with_f else None, zd.t, B, H, W, C)
        judge(name + " f_out %d" % with_f, "zd", zd.get(), ref["zd"])
        if with_f:
            judge(name + " f_out", "f", fo.get(), ref["f"])
        else:
            assert fo.untouched()


@pytest.mark.parametrize("name", R.cases_of("maxpool"))
def test_maxpool_same_forward(name):
    case, inp, dev = setup(name)
    B, PH, PW, C = case["shape"]
    out = Out((B, (PH + 1) // 2, (PW + 1) // 2, C), NAN)
    call("mmd_maxpool_same_fwd", dev["src"], out.t, B, PH, PW, C)
    judge(name, "pool", out.get(), R.case_ref(case, inp, D, DEV)["pool"])


# ------------------------------------------------------------------------------------------------ grouped frozen nets
@pytest.mark.parametrize("name", R.cases_of("group"))
def test_node_forward_grouped_nets(name):
    """mmd_set_group(3 nets, 2 images each): image b reads theta / w_dw / w_pw / bias of net b // 2 w_stride floats apart and scale / shift
    bn_stride floats apart, in mmd_bifpn_node_fwd_fused and mmd_bifpn_node_dw_fwd; a B that is not n * images is refused"""
    case, inp, dev = setup(name)
    B, H, W, C = case["shape"]
    ref = R.case_ref(case, inp, D, DEV)
    ops = ops_of(dev, case["mode"])
    y, fo, zd, y2 = (Out((B, H, W, C), NAN) for _ in range(4))
    refused = 0
    dll = _lib.LIB.load()
    assert dll.mmd_set_group(R.GROUP_N, R.GROUP_IMAGES, inp["w_stride"], inp["bn_stride"]) == 0
    try:
        call("mmd_bifpn_node_fwd_fused", *ops, dev["theta_buf"], dev["w_dw_buf"], dev["w_pw_buf"], dev["bias_buf"], dev["scale_buf"],
             dev["shift_buf"], y.t, B, H, W, C)
        call("mmd_bifpn_node_dw_fwd", *ops, dev["theta_buf"], dev["w_dw_buf"], fo.t, zd.t, B, H, W, C)
        for entry, tail in (("mmd_bifpn_node_fwd_fused", (dev["w_pw_buf"], dev["bias_buf"], dev["scale_buf"], dev["shift_buf"], y2.t)),
                            ("mmd_bifpn_node_dw_fwd", (None, y2.t))):
            try:
                call(entry, *ops, dev["theta_buf"], dev["w_dw_buf"], *tail, B - 1, H, W, C)
            except RuntimeError as e:
                refused += "status -22" in str(e)
    finally:
        rc = dll.mmd_set_group(1, 0, 0, 0)
    assert rc == 0
    torch.cuda.synchronize()
    assert refused == 2 and y2.untouched()
    judge_all(name, {"y": y.get(), "f": fo.get(), "zd": zd.get()}, ref)


# ------------------------------------------------------------------------------------------------ backward
def grad_outs(case, inp, acc):
    B, H, W, C = case["shape"]
    mode = case["mode"]
    shapes = {"d0": (B, H, W, C), "d1": (B, H, W, C), "dup": (B, H // 2, W // 2, C)}
    o = {k: Out(shapes[k], inp["init"][k] if acc else NAN) for k, on in (("d0", True), ("d1", mode & 1), ("dup", mode & 2)) if on}
    o["wdot"], o["dw_grad"] = Out((4,), inp["init"]["wdot"]), Out((9, C), inp["init"]["dw_grad"])
    return o


def check_wdot(got, inp, n):
    assert torch.equal(got["wdot"][n:].cpu(), inp["init"]["wdot"][n:]), "wdot written past the operand count"
    got["wdot"] = got["wdot"][:n]


def theta_check(case, inp, dev, ref, label):
    n = R.nops(case["mode"])
    dth = Out((n,), inp["dtheta0"])
    call("mmd_bifpn_theta_bwd", dev["theta"], dev["wdot_in"], dth.t, n)
    judge(label, "dtheta", dth.get(), ref["dtheta"])


@pytest.mark.parametrize("name", R.cases_of("bwd_dw"))
def test_node_dw_backward_generic_operand_sets(name):
    """mmd_bifpn_node_dw_bwd on the operand sets the BiFPN itself never builds (1, 3, 6: 'others through the generic forms'), C = 48 and
    112 on a ragged map, acc = 0 (NaN pre-fill) and 1: dx, the operand gradients, wdot, the depthwise weight gradient"""
    case, inp, dev = setup(name)
    B, H, W, C = case["shape"]
    mode, n = case["mode"], R.nops(case["mode"])
    for acc in (0, 1):
        ref = R.case_ref(case, inp, D, DEV, variant=(acc, 0))
        o = grad_outs(case, inp, acc)
        dx = Out((B, H, W, C), NAN)
        t = lambda k: o[k].t if k in o else None
        call("mmd_bifpn_node_dw_bwd", *ops_of(dev, mode), dev["theta"], dev["w_dw"], dev["dzd"], dx.t, o["wdot"].t, B, H, W, C,
             t("d0"), acc, t("d1"), acc, t("dup"), acc, o["dw_grad"].t)
        got = {k: v.get() for k, v in o.items()}
        got["dx"] = dx.get()
        check_wdot(got, inp, n)
        dth = ref.pop("dtheta")
        judge_all("%s acc %d" % (name, acc), got, ref)
    theta_check(case, inp, dev, {"dtheta": dth}, name)


@pytest.mark.parametrize("name", R.cases_of("bwd_full"))
def test_node_backward_full_forms(name):
    """mmd_bifpn_node_bwd_full_form in every form node_ref.route allows for the case (64- / 16-channel blocks, the pooled gradient by global
    atomics / through the LDS tile): dz, dgamma / dbeta, the operand gradients (overwritten and accumulated), the pooled operand's scatter
    onto a non-zero map, wdot, the depthwise weight gradient and the operands' BatchNorm sums (of the total and of this launch's share),
    with plain and with lazy operands, generic-K and fixed-K GEMM forms, an inactive theta entry"""
    case, inp, dev = setup(name)
    B, H, W, C = case["shape"]
    mode, n, lazy = case["mode"], R.nops(case["mode"]), case["lazy"]
    wpt = g(inp["w_pw"].t())
    idx = R.op_indices(mode)
    sc4 = ptr4([dev["lz%d" % i]["scale"] if lazy >> i & 1 else None for i in range(4)]) if lazy else None
    sh4 = ptr4([dev["lz%d" % i]["shift"] if lazy >> i & 1 else None for i in range(4)]) if lazy else None
    for (sb, pl), rt in R.bwd_forms(case):
        for acc, own in R.BWD_VARIANTS:
            ref = R.case_ref(case, inp, D, DEV, variant=(acc, own))
            o = grad_outs(case, inp, acc)
            if mode & 4:
                o["dpl"] = Out((B, 2 * H, 2 * W, C), inp["init"]["dpl"])
            o["dz"], o["dgamma"], o["dbeta"] = Out((B, H, W, C), NAN), Out((C,), inp["init"]["dgamma"]), Out((C,), inp["init"]["dbeta"])
            x = {}
            for i in range(4):
                if i in idx:
                    b = dev["bn%d" % i]
                    o[R.SUMS_KEY[i]] = Out((2 * C,), inp["bn%d" % i]["sums0"], D)
                    x[i] = (dev[R.SLOT_KEY[i]] if b["z"] is None else b["z"], b["mean"], b["invstd"], o[R.SUMS_KEY[i]].t)
                else:
                    x[i] = (None, None, None, None)
            t = lambda k: o[k].t if k in o else None
            call("mmd_bifpn_node_bwd_full_form", *ops_of(dev, mode), dev["theta"], dev["w_dw"], o["wdot"].t, B, H, W, C,
                 t("d0"), acc, t("d1"), acc, t("dup"), acc, o["dw_grad"].t, *x[0], *x[1], *x[2], t("dpl"), *x[3], own, sc4, sh4,
                 dev["g"], dev["z"], dev["bn_scale"], dev["bn_mean"], dev["bn_invstd"], dev["bn_sums"], inp["count"], wpt,
                 o["dz"].t, o["dgamma"].t, o["dbeta"].t, sb, pl)
            got = {k: v.get() for k, v in o.items()}
            check_wdot(got, inp, n)
            dth = ref.pop("dtheta")
            judge_all("%s NK%d CW%d lds%d acc%d own%d" % (name, rt[3], rt[4], rt[5], acc, own), got, ref)
    theta_check(case, inp, dev, {"dtheta": dth}, name)


# ------------------------------------------------------------------------------------------------ refusals
def _refused(entry, *args):
    with pytest.raises(RuntimeError, match="status -22"):
        call(entry, *args)
    torch.cuda.synchronize()


def test_refusals_leave_the_outputs_untouched():
    """unsupported width, in1 together with up in the whole-node forward, a lazy operand at C = 224, odd H with an up operand, four
    operands (operand set 7: the fusion has three weights) - each returns -22 on the host and writes nothing"""
    B, H, W = 2, 8, 8
    f = lambda *s: torch.full(s, 0.25, device=DEV)
    opt = lambda on, *s: f(*s) if on else None
    th2, th3 = f(2), f(3)

    def fwd(C, in1, up, pool, theta, H_=H):
        y = Out((B, H_, W, C), NAN)
        _refused("mmd_bifpn_node_fwd_fused", f(B, H_, W, C), opt(in1, B, H_, W, C), opt(up, B, H_ // 2, W // 2, C), opt(pool, B, 2 * H_, 2 * W, C),
                 theta, f(9, C), f(C, C), f(C), f(C), f(C), y.t, B, H_, W, C)
        assert y.untouched()
        z, zd, st = Out((B, H_, W, C), NAN), Out((B, H_, W, C), NAN), Out((2 * C,), torch.ones(2 * C), D)
        _refused("mmd_bifpn_node_fwd_fused_train", f(B, H_, W, C), opt(in1, B, H_, W, C), opt(up, B, H_ // 2, W // 2, C),
                 opt(pool, B, 2 * H_, 2 * W, C), theta, f(9, C), f(C, C), f(C), z.t, zd.t, st.t, B, H_, W, C)
        assert z.untouched() and zd.untouched() and bool((st.get() == 1).all())
    fwd(96, False, True, False, th2)            # unsupported width
    fwd(112, True, True, False, th3)            # in1 together with up
    fwd(112, False, True, False, th2, H_=7)     # odd H with an up operand
    # a lazy operand at C = 224
    C = 224
    z, zd, st = Out((B, H, W, C), NAN), Out((B, H, W, C), NAN), Out((2 * C,), torch.ones(2 * C), D)
    stats, ga, be = torch.ones(2 * C, dtype=D, device=DEV), f(C), f(C)
    _refused("mmd_bifpn_node_fwd_fused_train_lz", f(B, H, W, C), None, f(B, H // 2, W // 2, C), None, th2, f(9, C), f(C, C), f(C), z.t, zd.t, st.t,
             B, H, W, C, ptr4([stats, None, None, None]), ptr4([ga, None, None, None]), ptr4([be, None, None, None]),
             (ctypes.c_longlong * 4)(B * H * W, 0, 0, 0))
    assert z.untouched() and zd.untouched() and bool((st.get() == 1).all())
    # odd H with up / four operands in the fusion launches
    C = 48
    for Hx, in1, pool in ((7, False, False), (8, True, True)):
        assert (R.route("bwd_dw", B, Hx, W, C, 2 | (1 if in1 else 0) | (4 if pool else 0))) is None
        ops = (f(B, Hx, W, C), opt(in1, B, Hx, W, C), f(B, Hx // 2, W // 2, C), opt(pool, B, 2 * Hx, 2 * W, C))
        out, zd = Out((B, Hx, W, C), NAN), Out((B, Hx, W, C), NAN)
        _refused("mmd_bifpn_fuse_fwd", *ops, f(4), out.t, B, Hx, W, C)
        _refused("mmd_bifpn_node_dw_fwd", *ops, f(4), f(9, C), out.t, zd.t, B, Hx, W, C)
        dx, d0, wdot, dwg = Out((B, Hx, W, C), NAN), Out((B, Hx, W, C), NAN), Out((4,), torch.ones(4)), Out((9, C), torch.ones(9, C))
        _refused("mmd_bifpn_node_dw_bwd", *ops, f(4), f(9, C), f(B, Hx, W, C), dx.t, wdot.t, B, Hx, W, C, d0.t, 0, None, 0, None, 0, dwg.t)
        assert out.untouched() and zd.untouched() and dx.untouched() and d0.untouched()
        assert bool((wdot.get() == 1).all()) and bool((dwg.get() == 1).all())
