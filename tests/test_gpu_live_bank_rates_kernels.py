"""The two batched launches of a live bank's round on the GPU: mmd_rings_push against mmd_ring_push / mmd_ring_push_pcm entry by
entry, mmd_rings_resample against mmd_ring_resample entry by entry (and against mmd_resample_poly on the whole input), on copies of
the same rings, whole rings compared bit for bit; and their refusals, which launch nothing."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 8
_CACHE = {}


def _call(name, *args):
    from mm_distillnet_amd import _lib
    return _lib.call(name, *args)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _rs():
    from mm_distillnet_amd.audio import Resampler
    if "rs" not in _CACHE:
        _CACHE["rs"] = Resampler(DEV)
    return _CACHE["rs"]


# ---------------------------------------------------------------------------------------------- mmd_rings_push
# (kind: 0 float rows, else the PCM width; n; cap; absolute position; floats between the rows of a float chunk)
PUSH_CASES = {
    "five": [(0, 1, 1500, 3 * 1500 + 1499, 1), (2, 1025, 2048, 5 * 2048 + 1500, 0), (0, 1024, 1024, 7, 1024), (3, 1023, 3000, 2999, 0),
             (4, 1531, 1531, 100, 0)],
    "three": [(2, 1, 1024, 1023, 0), (0, 1025, 1100, (1 << 40) + 900, 1300), (0, 3000, 3000, 1234, 3000)],
    "four": [(3, 1024, 1025, 1024, 0), (0, 1023, 4096, 4000, 1023), (4, 1025, 1026, 513, 0), (2, 2048, 2048, 2047, 0)],
}


def _payloads(entries, seed):
    """one byte buffer holding every entry's chunk at a multiple of 16 bytes -> (device buffer, offsets)"""
    rng = np.random.default_rng(seed)
    parts, offs, at = [], [], 0
    for kind, n, cap, pos, stride in entries:
        if kind == 0:
            raw = rng.standard_normal((C, stride)).astype(np.float32).view(np.uint8).reshape(-1)
        else:
            raw = rng.integers(0, 256, size=n * C * kind, dtype=np.uint8)         # every byte pattern: the extremes of each width among them
        offs.append(at)
        parts.append(np.concatenate([raw, np.zeros(-len(raw) % 16, np.uint8)]))
        at += len(parts[-1])
    return torch.from_numpy(np.concatenate(parts)).to(DEV), offs


@pytest.mark.parametrize("fill", [float("nan"), -7.5e8])
@pytest.mark.parametrize("case", sorted(PUSH_CASES))
def test_rings_push_equals_the_single_pushes_bit_for_bit(case, fill):
    from mm_distillnet_amd.audio import rings_push_entry, rings_push_into
    entries = PUSH_CASES[case]
    assert 3 <= len(entries) <= 5 and len({cap for _, _, cap, _, _ in entries}) == len(entries)
    assert any(pos % cap + n > cap for _, n, cap, pos, _ in entries) and any(n == cap for _, n, cap, _, _ in entries)
    buf, offs = _payloads(entries, len(entries))
    rings = [torch.full((C, cap), fill, device=DEV) for _, _, cap, _, _ in entries]
    want = [r.clone() for r in rings]
    tab = np.zeros((len(entries), 8), np.int64)
    for k, ((kind, n, cap, pos, stride), off) in enumerate(zip(entries, offs)):
        rings_push_entry(tab, k, off, stride, n, kind, rings[k], cap, pos)
        if kind == 0:
            _call("mmd_ring_push", buf.data_ptr() + off, stride, C, n, want[k], cap, pos)
        else:
            _call("mmd_ring_push_pcm", buf.data_ptr() + off, n, C, kind, want[k], cap, pos)
    rings_push_into(buf, tab, torch.from_numpy(tab).to(DEV), len(entries), C)
    torch.cuda.synchronize()
    for k, (kind, n, cap, pos, _) in enumerate(entries):
        assert torch.equal(_bits(rings[k]), _bits(want[k])), (case, k)
        slots = (pos + torch.arange(n, device=DEV)) % cap
        untouched = torch.ones(cap, dtype=torch.bool, device=DEV)
        untouched[slots] = False
        assert torch.isfinite(rings[k][:, slots]).all() and int(untouched.sum()) == cap - n
        assert torch.equal(_bits(rings[k][:, untouched]), _bits(torch.full((C, cap - n), fill, device=DEV)))     # only the n slots are touched


def test_rings_push_refuses_on_the_host_and_launches_nothing():
    from mm_distillnet_amd import _lib
    dll = _lib.LIB.load()
    ring = torch.full((C, 2048), -7.5e8, device=DEV)
    src = torch.randn(C, 1024, device=DEV)
    tab = np.zeros((2, 8), np.int64)
    tab[:] = (0, 1024, 1000, 0, ring.data_ptr(), 2048, 5, 0)
    dev = torch.from_numpy(tab).to(DEV)
    stream = torch.cuda.current_stream().cuda_stream
    assert dll.mmd_rings_push(src.data_ptr(), tab.ctypes.data, dev.data_ptr(), 0, C, stream) == -22           # n_desc < 1
    assert dll.mmd_rings_push(src.data_ptr(), None, dev.data_ptr(), 2, C, stream) == -22                      # a null table
    assert dll.mmd_rings_push(src.data_ptr(), tab.ctypes.data, None, 2, C, stream) == -22
    tab[1, 2] = 2049                                                                                          # n > cap in the second entry
    assert dll.mmd_rings_push(src.data_ptr(), tab.ctypes.data, dev.data_ptr(), 2, C, stream) == -22
    torch.cuda.synchronize()
    assert bool((ring == -7.5e8).all())                                                                       # the first entry did not run


# ---------------------------------------------------------------------------------------------- mmd_rings_resample
N_IN = 4097
# rate -> (in_cap or None for the smallest the session allows, inputs pushed, out_cap, t_lo, t_hi or None for the last ready output)
RS_ENTRIES = {48000: (None, 1500, 1531, None, None), 16000: (3000, N_IN, 1531, 3301, 4700), 22050: (500, 600, 97, 777, 778),
              192000: (2000, N_IN, 400, 551, None)}


def _oldest(t, L, M, half):
    return (t * M) // L - half + 1


def _rs_case(fill):
    """per rate: a seeded input, the last in_cap samples of its first n_valid in an input ring (one mmd_ring_push), a filled output ring
    and the range - with the checks that the four entries hold the cases this file is about"""
    from mm_distillnet_amd.audio import live_in_ring_min, live_resample_ready
    out, seen = [], dict(min_ring=0, in_wrap=0, out_wrap=0, single=0, unaligned=0)
    for sr, (in_cap, n_valid, out_cap, t_lo, t_hi) in RS_ENTRIES.items():
        L, M, taps, bank, off = _rs()._bank(sr, 44100)
        half = taps // 2
        if ("x", sr) not in _CACHE:
            xd = torch.from_numpy(np.random.default_rng(sr).standard_normal((C, N_IN)).astype(np.float32)).to(DEV)
            _CACHE["x", sr] = (xd, _rs().resample(xd, sr))
        xd, whole = _CACHE["x", sr]
        least = live_in_ring_min(L, M, half)
        in_cap = least if in_cap is None else in_cap
        v_lo = max(0, n_valid - in_cap)
        ready = live_resample_ready(n_valid, L, M, half)
        t_hi = ready if t_hi is None else t_hi
        if t_lo is None:                                   # the first output whose oldest input is still resident
            t_lo = next(t for t in range(ready) if _oldest(t, L, M, half) >= v_lo)
        assert 0 <= t_lo < t_hi <= ready and t_hi - t_lo <= out_cap and _oldest(t_lo, L, M, half) >= v_lo, (sr, t_lo, t_hi, ready)
        in_ring = torch.full((C, in_cap), fill, device=DEV)
        _call("mmd_ring_push", xd.data_ptr() + 4 * v_lo, N_IN, C, n_valid - v_lo, in_ring, in_cap, v_lo)
        lo_in, hi_in = _oldest(t_lo, L, M, half), _oldest(t_hi - 1, L, M, half) + taps - 1
        seen["min_ring"] += in_cap == least
        seen["in_wrap"] += lo_in % in_cap > hi_in % in_cap
        seen["out_wrap"] += t_lo % out_cap > (t_hi - 1) % out_cap
        seen["single"] += t_hi - t_lo == 1
        seen["unaligned"] += t_lo % L != 0 and t_hi % L != 0
        out.append(dict(sr=sr, in_ring=in_ring, n_valid=n_valid, out_ring=torch.full((C, out_cap), fill, device=DEV), t_lo=t_lo, t_hi=t_hi,
                        whole=whole, args=(L, M, taps, bank, off)))
    print(seen, [(e["sr"], e["in_ring"].shape[1], e["t_lo"], e["t_hi"]) for e in out])
    assert seen["min_ring"] >= 1 and seen["in_wrap"] >= 2 and seen["out_wrap"] >= 2 and seen["single"] == 1 and seen["unaligned"] >= 3
    return out


@pytest.mark.parametrize("fill", [float("nan"), -7.5e8])
def test_rings_resample_equals_the_single_launches_bit_for_bit(fill):
    from mm_distillnet_amd.audio import RINGS_RS_DESC
    entries = _rs_case(fill)
    rs = _rs()
    tab = np.zeros(len(entries) * RINGS_RS_DESC, np.uint8)
    want = []
    for k, e in enumerate(entries):
        L, M, taps, bank, off = e["args"]
        ref = e["out_ring"].clone()
        _call("mmd_ring_resample", e["in_ring"], e["in_ring"].shape[1], C, e["n_valid"], bank, off, L, M, taps, ref, ref.shape[1], e["t_lo"], e["t_hi"])
        want.append(ref)
        rs.rings_resample_plan(tab, k, e["in_ring"], e["n_valid"], e["sr"], e["out_ring"], e["t_lo"], e["t_hi"])
    assert len({e["args"][:3] for e in entries}) == 4                                # four ratios in one launch
    rs.rings_resample_into(tab, torch.from_numpy(tab).to(DEV), len(entries), C)
    torch.cuda.synchronize()
    for e, ref in zip(entries, want):
        assert torch.equal(_bits(e["out_ring"]), _bits(ref)), e["sr"]
        cap = ref.shape[1]
        slots = torch.arange(e["t_lo"], e["t_hi"], device=DEV) % cap
        expect = torch.full((C, cap), fill, device=DEV)
        expect[:, slots] = e["whole"][:, e["t_lo"]:e["t_hi"]]                        # and so the offline kernel's bits on the whole input
        assert torch.equal(_bits(e["out_ring"]), _bits(expect)), e["sr"]


def test_rings_resample_refuses_on_the_host_and_launches_nothing():
    from mm_distillnet_amd import _lib
    from mm_distillnet_amd.audio import RINGS_RS_DESC
    dll = _lib.LIB.load()
    entries = _rs_case(-7.5e8)[:2]
    rs = _rs()
    tab = np.zeros(2 * RINGS_RS_DESC, np.uint8)
    for k, e in enumerate(entries):
        rs.rings_resample_plan(tab, k, e["in_ring"], e["n_valid"], e["sr"], e["out_ring"], e["t_lo"], e["t_hi"])
    e = entries[1]                                                                   # 16 kHz: the ring holds the inputs 1097 .. 4096
    with pytest.raises(RuntimeError, match="mmd_rings_resample_plan failed with status -22"):
        rs.rings_resample_plan(tab, 1, e["in_ring"], e["n_valid"], e["sr"], e["out_ring"], 3190, e["t_hi"])      # its oldest input, 1094, is gone
    dev = torch.from_numpy(tab).to(DEV)
    stream = torch.cuda.current_stream().cuda_stream
    assert dll.mmd_rings_resample(tab.ctypes.data, dev.data_ptr(), 0, C, stream) == -22
    assert dll.mmd_rings_resample(None, dev.data_ptr(), 2, C, stream) == -22
    assert dll.mmd_rings_resample(tab.ctypes.data, None, 2, C, stream) == -22
    words = tab.view(np.int64).reshape(2, -1)
    assert words[1, 7] == e["t_lo"]
    words[1, 7] = 3190                                                               # the overwritten range, written past the planner
    assert dll.mmd_rings_resample(tab.ctypes.data, dev.data_ptr(), 2, C, stream) == -22
    torch.cuda.synchronize()
    for e in entries:
        assert bool((e["out_ring"] == -7.5e8).all())                                 # nothing was launched: the good entry did not run either
