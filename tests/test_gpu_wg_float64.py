"""GPU: the 1x1-conv weight-gradient kernels - the grouped launch of csrc/pw_wgrad_grouped.hip in its default rectangular form
(mmd_wgrad_plan, mmd_wgrad_grouped, mmd_wgrad_grouped_bf16, mmd_wgrad_grouped_form with bf16 0 / 1 / 2 and rows32 0 / 1) and the per-layer
pw_wgrad_kernel (mmd_pwconv_bwd_weight, _bf16, _bn, _bn_bf16) - against the float64 reference of tests/wg_ref.py, through the C ABI, on the
tables wg_ref.WG_TABLES / PER_LAYER_CASES (test_wg_ref_cpu.py proves through wg_ref.plan / describe that every branch is reached).

Every comparison is per element: |got_i - ref64_i| <= K * unit * A_i + tiny, A_i the magnitude the reference reports for that element, unit
2^-24 (2^-9 for the bf16 forms) and K the family's constant of wg_ref (calibrated on the CPU by test_wg_ref_cpu.py, never on these kernels).
All dW of a table lie in one arena, each in front of 16 guard rows of a sentinel; the grouped launches find dW pre-filled with NaN (it is
written), the per-layer launches with a random dw0 (they accumulate).  The workspace has exactly ws_floats floats of NaN in front of a
guard region.  After every launch every dW of the table is finite, every other float of the arena and the workspace guard keep their bits.
The table the C planner fills is compared field by field with wg_ref.plan.  In bits: every grid size gives the same dW; rows32 changes
nothing on v_mfma_f32 and on the bf16 form; bf16 = 0 without rows32 is bf16 = 2; bf16 = 0 with rows32 is the split kernel (other bits) up to
255 layers and v_mfma_f32 above, or throughout under MMD_MFMA_F32.  Each check prints `WG64 <family> <mode> <table/layer> <worst err / (unit
A)> (K)` before it asserts.  The float64 references run on the GPU in torch (plain matmuls: nothing of the library under test)."""
import ctypes
import functools
import os
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from mm_distillnet_amd import _lib
from mm_distillnet_amd.engine import WgLayer

import wg_ref as W
from pw_ref import Out, GPU_ERROR          # the guarded output buffer; the list of GPU errors met (shared: after one, neither module launches)

call = _lib.call
DEV = "cuda"
D, F = torch.float64, torch.float32
SPLIT_DEFAULT = "MMD_MFMA_F32" not in os.environ          # mmd_split_default (common.h): set, to any value, is v_mfma_f32
PLAN_OVERRIDE = [k for k in W.PLAN_ENV if k in os.environ]
grouped = pytest.mark.skipif(bool(PLAN_OVERRIDE), reason="%s set: wg_ref.plan describes the planner's default rectangular form only" % PLAN_OVERRIDE)
GUARD_ROWS, WS_GUARD = 16, 8192
NAN = float("nan")


def guarded(label, fn, *args):
    assert not GPU_ERROR, "an earlier test hit a GPU error (%s): not launching anything more" % GPU_ERROR[0]
    try:
        return fn(*args)
    except RuntimeError as e:
        GPU_ERROR.append("%s: %s" % (label, str(e)[:200]))
        raise


def bits(t):
    return t.view(torch.int32)


def judge(family, label, got, ref, A, lid=None):
    """got / ref / A: tensors of one shape (every element is judged).  lid: per element the layer it belongs to (the worst one is named)"""
    K, unit = W.K_BY_FAMILY[family], W.UNIT[family]
    got = got.double()
    assert got.shape == ref.shape == A.shape, (got.shape, ref.shape, A.shape)
    assert bool(torch.isfinite(got).all()), "%s %s: non-finite output" % (family, label)
    q = ((got - ref).abs() / (unit * A + W.TINY)).reshape(-1)
    i = int(q.argmax())
    r = float(q[i])
    where = "" if lid is None else "/%d" % int(lid[i])
    print("WG64 %-10s %-46s %8.3f  (K %.0f)" % (family, label + where, r, K))
    assert r <= K, "%s %s%s: err / (unit A) = %.3f > K = %.1f" % (family, label, where, r, K)


# ------------------------------------------------------------------------------------------------ grouped launches: tables
@functools.lru_cache(maxsize=None)
def table_data(name):
    """inputs of every layer on the device, the arena layout ([N, K] floats of dW then GUARD_ROWS * K of guard, per layer) and, in that layout,
    the float64 reference, its magnitudes and the layer of every element (-1: guard)"""
    layers = W.TABLE[name]["layers"]
    offs, pos = [], 0
    for M, K, N, _, _ in layers:
        offs.append(pos)
        pos += (N + GUARD_ROWS) * K
    ref, A = torch.zeros(pos, dtype=D, device=DEV), torch.ones(pos, dtype=D, device=DEV)
    lid = torch.full((pos,), -1, dtype=torch.int32, device=DEV)
    dev = []
    for i, layer in enumerate(layers):
        inp = W.layer_inputs(i, *layer)
        dev.append(W.to(inp, F, DEV))
        v, a = W.layer_ref(layer, W.to(inp, D, DEV))["dw"]
        sl = slice(offs[i], offs[i] + v.numel())
        ref[sl], A[sl], lid[sl] = v.reshape(-1), a.reshape(-1), i
    arena0 = torch.where(lid >= 0, torch.full_like(ref, NAN), torch.full_like(ref, W.SENTINEL)).float()
    return {"layers": layers, "offs": offs, "dev": dev, "ref": ref, "A": A, "lid": lid, "arena0": arena0, "arena": arena0.clone()}


@functools.lru_cache(maxsize=None)
def planned(name, n):
    """the first n layers of a table through mmd_wgrad_plan, compared with wg_ref.plan field by field; the planned table on the device and a
    workspace of exactly ws_floats floats in front of its guard"""
    td, t = table_data(name), W.TABLE[name]
    arr = (WgLayer * n)()
    base = td["arena"].data_ptr()
    for i, (M, K, N, flags, B) in enumerate(td["layers"][:n]):
        d, a = td["dev"][i], arr[i]
        a.dy, a.x, a.dw = d["dy"].data_ptr(), d["x"].data_ptr(), base + 4 * td["offs"][i]
        a.in_scale, a.in_shift = (d["scale"].data_ptr(), d["shift"].data_ptr()) if "aff" in flags else (None, None)
        a.gate = d["gate"].data_ptr() if "gate" in flags else None
        a.M, a.K, a.N, a.in_act, a.rows_per_image = M, K, N, (1 if "aff" in flags else 0), W.cdiv(M, B)
    ni, nt, wsf = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_longlong(-7)
    cv = lambda o: ctypes.cast(ctypes.pointer(o), ctypes.c_void_p)
    assert _lib.LIB.load().mmd_wgrad_plan(ctypes.cast(arr, ctypes.c_void_p), n, t["rows_per_item"], cv(ni), cv(nt), cv(wsf)) == 0
    want, items, tiles, ws_floats = W.plan(td["layers"][:n], t["rows_per_item"])
    assert (ni.value, nt.value, wsf.value) == (items, tiles, ws_floats), "the planner's totals are not its copy's"
    for i, lp in enumerate(want):
        got = {f: getattr(arr[i], f) for f in W.PLAN_FIELDS}
        assert got == {f: lp[f] for f in W.PLAN_FIELDS}, "%s layer %d %s: the planner's table is not its copy's" % (name, i, td["layers"][i])
    ws = torch.full((ws_floats + WS_GUARD,), W.SENTINEL, device=DEV)
    return {"n": n, "table": torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV), "items": items, "tiles": tiles, "ws": ws,
            "ws_floats": ws_floats, "live": (td["lid"] >= 0) & (td["lid"] < n), "keep": arr}


def launch(name, p, entry, blocks, mode=None, rows32=None):
    """one grouped launch on a NaN dW / NaN workspace -> a copy of the whole arena, guards and all, after the checks every launch gets"""
    td = table_data(name)
    assert not rows32 or all(l[0] % 32 == 0 for l in td["layers"][:p["n"]]), "rows32 promises that every M is a multiple of 32"
    td["arena"].copy_(td["arena0"])
    p["ws"][:p["ws_floats"]].fill_(NAN)
    args = [p["table"], p["n"], p["items"], p["tiles"], p["ws"], blocks, 0.0, 0.0]
    call(entry, *(args + ([mode, rows32] if entry == "mmd_wgrad_grouped_form" else [])))
    torch.cuda.synchronize()
    out = td["arena"].clone()
    assert bool((p["ws"][p["ws_floats"]:] == W.SENTINEL).all()), "the launch wrote behind its workspace"
    assert torch.equal(bits(out)[~p["live"]], bits(td["arena0"])[~p["live"]]), "the launch wrote outside the dW of its layers (guard rows or another layer)"
    assert bool(torch.isfinite(out[p["live"]]).all()), "a dW element was not written (or not finite)"
    return out


GROUPED = [(t["name"], n) for t in W.WG_TABLES for n in t["prefixes"]]


@grouped
@pytest.mark.parametrize("name,n", GROUPED)
def test_planner_equals_its_copy(name, n):
    guarded("plan %s/%d" % (name, n), planned, name, n)


def _grouped(name, n):
    t0 = time.time()
    td, t, p = table_data(name), W.TABLE[name], planned(name, n)
    live = p["live"]
    res = {}

    def sweep(key, entry, mode=None, rows32=None):
        label = "%s %s/%d" % (key, name, n)
        for blocks in t["grids"]:
            out = launch(name, p, entry, blocks, mode, rows32)
            if key not in res:
                res[key] = out
                judge("dw_bf16" if (mode == 1 or entry.endswith("bf16")) else "dw", label, out[live], td["ref"][live], td["A"][live], td["lid"][live])
            else:
                assert torch.equal(bits(out), bits(res[key])), "%s: %d blocks and %d blocks give other bits" % (label, blocks, t["grids"][0])

    for rows32 in t["rows32"]:
        for mode in (0, 1, 2):
            sweep("form%d%s" % (mode, "r" if rows32 else ""), "mmd_wgrad_grouped_form", mode, rows32)
    eq = lambda a, b: torch.equal(bits(res[a]), bits(res[b]))
    if name == "tails":
        sweep("plain", "mmd_wgrad_grouped")
        sweep("plain_bf16", "mmd_wgrad_grouped_bf16")
        assert eq("plain", "form0") and eq("plain_bf16", "form1"), "the plain entry points are not the form entry point with rows32 = 0"
    assert eq("form0", "form2"), "bf16 = 0 without the rows32 promise is not v_mfma_f32: there is no split kernel without the promise"
    if 1 in t["rows32"]:
        assert eq("form2r", "form2"), "rows32 changed the bits of the v_mfma_f32 form: it changes addressing, not arithmetic"
        assert eq("form1r", "form1"), "rows32 changed the bits of the bf16 form"
        if SPLIT_DEFAULT and n <= W.GW_MAXL3:
            assert not eq("form0r", "form2r"), "the split form and v_mfma_f32 gave the same bits: the split kernel did not run"
        else:          # MMD_MFMA_F32, or more layers than the split kernel's table copy holds: v_mfma_f32
            assert eq("form0r", "form2r"), "bf16 = 0 with rows32 is not v_mfma_f32 (%d layers, split default %d)" % (n, SPLIT_DEFAULT)
    print("WG64 time grouped %s/%d %.2f s" % (name, n, time.time() - t0))


@grouped
@pytest.mark.parametrize("name,n", GROUPED)
def test_wgrad_grouped(name, n):
    """every (bf16, rows32) form legal for the table at every grid size: float64, guards, bits"""
    guarded("grouped %s/%d" % (name, n), _grouped, name, n)


# ------------------------------------------------------------------------------------------------ per-layer launches
def _per_layer(ci):
    t0 = time.time()
    M, K, N, B = case = W.PER_LAYER_CASES[ci]
    layer, rpi = (M, K, N, "", B), W.cdiv(M, B)
    inp, bn = W.layer_inputs(ci, *layer), W.bn_layer_inputs(M, N)
    d, d64, b, b64 = W.to(inp, F, DEV), W.to(inp, D, DEV), W.to(bn, F, DEV), W.to(bn, D, DEV)
    plain, bnm = W.per_layer_modes()

    def pro(flags):
        aff = "aff" in flags
        return [d["scale"] if aff else None, d["shift"] if aff else None, 1 if aff else 0, d["gate"] if "gate" in flags else None, rpi]

    for flags in plain:
        v, A = W.layer_ref(layer, d64, flags=flags, with_dw0=True)["dw"]
        for sfx in ("", "_bf16"):
            dw = Out((N, K), inp["dw0"])
            call("mmd_pwconv_bwd_weight" + sfx, d["dy"], d["x"], dw.t, M, K, N, *pro(flags))
            torch.cuda.synchronize()
            judge("dw" + sfx, "per-layer %s [%s]" % (case, flags), dw.get(), v, A)
    for flags, mode in bnm:
        act, mul_b, dsum = mode
        ref = W.layer_ref(layer, d64, bn=b64, bn_mode=mode, flags=flags, with_dw0=True)
        for sfx in ("", "_bf16"):
            dw, dg, db = Out((N, K), inp["dw0"]), Out((N,), bn["dgamma0"]), Out((N,), bn["dbeta0"])
            call("mmd_pwconv_bwd_weight_bn" + sfx, d["dy"], b["z"], d["x"], dw.t, M, K, N, *pro(flags), b["scale"], b["shift"], b["mean"], b["invstd"],
                 b["sums"], bn["count"], act, b["mul_b"] if mul_b else None, W.BN_RPI, dg.t if dsum else None, db.t if dsum else None)
            torch.cuda.synchronize()
            label = "per-layer bn %s [%s] act %d mul_b %d dsum %d" % (case, flags, act, mul_b, dsum)
            judge("dw_bn" + sfx, label, dw.get(), *ref["dw"])
            if dsum:
                judge("dsum", label + " dgamma" + sfx, dg.get(), *ref["dgamma"])
                judge("dsum", label + " dbeta" + sfx, db.get(), *ref["dbeta"])
            else:
                assert set(ref) == {"dw"} and torch.equal(dg.get(), b["dgamma0"]) and torch.equal(db.get(), b["dbeta0"])
    print("WG64 time per-layer %s %.2f s" % (case, time.time() - t0))


@pytest.mark.parametrize("ci", range(len(W.PER_LAYER_CASES)), ids=["M%d_K%d_N%d" % c[:3] for c in W.PER_LAYER_CASES])
def test_pwconv_bwd_weight(ci):
    """mmd_pwconv_bwd_weight, _bf16, _bn, _bn_bf16: dw accumulated onto a random dw0 with atomics (judged, not compared in bits), dgamma / dbeta
    added to their pre-fill, or left alone where they are null"""
    guarded("per-layer %s" % (W.PER_LAYER_CASES[ci],), _per_layer, ci)


# ------------------------------------------------------------------------------------------------ bad arguments
def _plan_bad():
    dll = _lib.LIB.load()
    buf = torch.zeros(64, device=DEV)
    cv = lambda o: ctypes.cast(ctypes.pointer(o), ctypes.c_void_p)
    planner_fields = ("mchunk", "nsplit", "ntn", "ntk", "item0", "tile0", "pad_", "ws_off")
    bad = {"K % 4": dict(K=10), "N % 4": dict(N=6), "gate, rows_per_image 0": dict(gate=buf.data_ptr(), rows_per_image=0),
           "gate, rows_per_image -1": dict(gate=buf.data_ptr(), rows_per_image=-1), "scale without shift": dict(in_scale=buf.data_ptr()),
           "shift without scale": dict(in_shift=buf.data_ptr()), "n = 513": dict()}
    for what, o in bad.items():
        n = W.GW_MAXL + 1 if what == "n = 513" else 1
        arr = (WgLayer * n)()
        for a in arr:
            a.dy = a.x = a.dw = buf.data_ptr()
            a.M, a.K, a.N, a.rows_per_image = 40, 16, 8, 20
            for f in planner_fields:
                setattr(a, f, -1)
        for k, v in o.items():
            setattr(arr[0], k, v)
        ni, nt, wsf = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_longlong(-7)
        rc = dll.mmd_wgrad_plan(ctypes.cast(arr, ctypes.c_void_p), n, 32, cv(ni), cv(nt), cv(wsf))
        assert rc == -22, (what, rc)
        assert (ni.value, nt.value, wsf.value) == (-7, -7, -7) and all(getattr(arr[0], f) == -1 for f in planner_fields), what
        assert arr[0].rows_per_image == o.get("rows_per_image", 20), what
    # (the planner's limit itself is legal: the 512-layer prefix of the `many` table is planned and launched)


def test_plan_bad_arguments_return_einval_and_write_nothing():
    """K % 4, N % 4, a gate with rows_per_image <= 0, scale without shift, n = 513: -22, totals and table untouched (the checks come before
    anything a tile-form variable changes: not skipped under them)"""
    guarded("plan, bad arguments", _plan_bad)


def _form_bad():
    td, p = table_data("tails"), planned("tails", len(W.TABLE["tails"]["layers"]))
    td["arena"].copy_(td["arena0"])
    p["ws"][:p["ws_floats"]].fill_(NAN)
    for bf16 in (3, -1):
        with pytest.raises(RuntimeError, match="status -22"):
            call("mmd_wgrad_grouped_form", p["table"], p["n"], p["items"], p["tiles"], p["ws"], 0, 0.0, 0.0, bf16, 0)
    torch.cuda.synchronize()
    assert torch.equal(bits(td["arena"]), bits(td["arena0"])), "a refused launch wrote dW"
    assert bool(torch.isnan(p["ws"][:p["ws_floats"]]).all()) and bool((p["ws"][p["ws_floats"]:] == W.SENTINEL).all()), "a refused launch wrote the workspace"


@grouped
def test_form_bad_arguments_return_einval_and_write_nothing():
    guarded("form, bad arguments", _form_bad)


def _per_layer_bad(sfx):
    f = lambda *s: torch.full(s, 0.25, device=DEV)
    bad = {"K % 4": dict(K=10), "N % 4": dict(N=6), "gate, rows_per_image 0": dict(gate=f(2, 16), rpi=0), "scale without shift": dict(scale=f(16)),
           "shift without scale": dict(shift=f(16))}
    bn_bad = {"missing z": dict(z=None), "count 0": dict(count=0), "count -3": dict(count=-3), "dgamma without dbeta": dict(dbeta=None),
              "dbeta without dgamma": dict(dgamma=None), "mul_b, bn_rows_per_image 0": dict(mul_b=f(8), bn_rpi=0)}
    for bnp in (False, True):
        for what, o in {**bad, **(bn_bad if bnp else {})}.items():
            M, K, N = 40, o.get("K", 16), o.get("N", 8)
            dw, dg, db = Out((N, K), torch.ones(N, K)), Out((N,), torch.ones(N)), Out((N,), torch.ones(N))
            args = [f(M, K), dw.t, M, K, N, o.get("scale"), o.get("shift"), 0, o.get("gate"), o.get("rpi", 20)]
            if bnp:
                args = [f(M, N), o.get("z", f(M, N))] + args + [f(N), f(N), f(N), f(N), torch.ones(2 * N, dtype=D, device=DEV), o.get("count", 40), 1,
                                                                o.get("mul_b"), o.get("bn_rpi", 7), o.get("dgamma", dg.t), o.get("dbeta", db.t)]
            else:
                args = [f(M, N)] + args
            with pytest.raises(RuntimeError, match="status -22"):
                call("mmd_pwconv_bwd_weight" + ("_bn" if bnp else "") + sfx, *args)
            torch.cuda.synchronize()
            assert bool((dw.get() == 1).all()) and bool((dg.get() == 1).all()) and bool((db.get() == 1).all()), what


@pytest.mark.parametrize("sfx", ["", "_bf16"])
def test_per_layer_bad_arguments_return_einval_and_write_nothing(sfx):
    """the planner's K / N / gate / scale checks on the per-layer entry points; missing z, count <= 0, dgamma without dbeta on the _bn ones: -22,
    dw / dgamma / dbeta keep their pre-fill"""
    guarded("per-layer%s, bad arguments" % sfx, _per_layer_bad, sfx)
