"""Live bank at per-session sample rates on the GPU, end to end: a bank at (48 kHz, 44.1 kHz, 16 kHz) against a 44.1 kHz bank of a second
detector that is fed `Resampler.resample` of the same recordings, cut where `live_resample_ready` says the outputs become available;
`push_all` / `push_all_pcm` against the sequential pushes; the unchanged default; `reset` on a 48 kHz session; detect.py --any_rate.
The small student and the 44.1 kHz recordings are tests/test_gpu_live_bank.py's; the bias is tuned, as there, on windows of what this
file's bank hears: the recordings brought to the sessions' rates and resampled back."""
import os
import sys
import wave

import numpy as np
import pytest
import torch

import test_gpu_live_bank as B
from helpers import make_state
from test_gpu_live_bank import BATCH, C, COEF, DEV, HOP, NS, ROOT, S, SPAN, WIN, _same, _track_config

pytestmark = pytest.mark.gpu
RATES = (48000, None, 16000)
IN_RING0 = 2000                                        # session 0's input ring: pieces of 2000 - 140 - 160 = 1700 samples
PLAN_SEED = 4
_CACHE = {}


def _rate(s):
    return 44100 if RATES[s] is None else RATES[s]


def _recording(s, src=None):
    """session s's recording AT ITS OWN RATE -> (int16 [C, n], float32 int16 / 2^15): tests/test_gpu_live_bank.py's 44.1 kHz recording
    src (default: s) brought to 16 kHz - so that all three sessions hear audio of one bandwidth, and the student, which answers a
    source without anything above 8 kHz far more strongly, stays in one regime for all of them - then to the session's rate, and quantised"""
    key = ("rec", s, src)
    if key not in _CACHE:
        from mm_distillnet_amd.audio import Resampler
        w = B._quantised(s if src is None else src)[1].to(DEV)
        base = Resampler(DEV).resample(w, 44100, 16000)
        at_rate = Resampler(DEV).resample(base, 16000, _rate(s)).cpu()
        q = torch.clamp(torch.round(at_rate * 32767.0), -32768, 32767).to(torch.int16)
        _CACHE[key] = (q, q.to(torch.float32) / 32768.0)
    return _CACHE[key]


def _resampled(s, src=None):
    """the oracle's input: `Resampler.resample(whole recording of s, R_s)` on the device"""
    key = ("res", s, src)
    if key not in _CACHE:
        from mm_distillnet_amd.audio import Resampler
        _CACHE[key] = Resampler(DEV).resample(_recording(s, src)[1].to(DEV).contiguous(), _rate(s))
    return _CACHE[key]


def _state():
    """make_state's D2 audio net, the classifier bias tuned on seven windows of what the three sessions hear (8 candidates per window:
    the answer differs widely between recordings - with this bias session 0's gives no row in the three-rate run, 1's some 50 and
    2's some 80, at most 46 in one window; session 0's ring is compared sample for sample there, and a 48 kHz session that returns
    rows is the reset test's second recording)"""
    if "state" not in _CACHE:
        from mm_distillnet_amd.audio import MelFrontEnd
        from mm_distillnet_amd.synth import tune_teacher_bias
        spec, st = make_state(COEF, 8, 13, "audio")
        wins = torch.stack([_resampled(s)[:, w * HOP:w * HOP + WIN] for s, w in ((0, 0), (0, 3), (0, 6), (1, 0), (1, 3), (2, 0), (2, 2))])
        tune_teacher_bias(spec, st, MelFrontEnd(DEV).student_input(wins, None, S, db=True).cpu(), DEV, 8)
        _CACHE["state"] = (spec, st)
    spec, st = _CACHE["state"]
    return spec, {k: v.clone() for k, v in st.items()}


def _detector(**kw):
    from mm_distillnet_amd.detector import AudioDetector
    spec, st = _state()
    det = AudioDetector(spec, DEV, image_size=S, **kw)
    det.load(st)
    return det


def _ready(s, n_in, final=False):
    from mm_distillnet_amd.audio import live_resample_ready, resample_ratio
    if RATES[s] is None:
        return n_in
    return live_resample_ready(n_in, *resample_ratio(RATES[s]), final)


def _lengths():
    return [_recording(s)[0].shape[1] for s in range(NS)]


def _plan():
    """The seeded interleaving (session, input samples) and what it must hold, checked on the host schedule before any device work"""
    if "plan" not in _CACHE:
        from mm_distillnet_amd.audio import bank_schedule, bank_state
        rng = np.random.default_rng(PLAN_SEED)
        lengths = _lengths()
        at, pushes = [0] * NS, []
        while any(a < n for a, n in zip(at, lengths)):
            s = int(rng.choice([k for k in range(NS) if at[k] < lengths[k]]))
            n = min(max(1, int(rng.choice([1, 500, 1000, 1531, 2500, 4096, 8000]) * _rate(s) / 44100)) if rng.random() > 0.1 else 1, lengths[s] - at[s])
            pushes.append((s, n))
            at[s] += n
        state, ticks, at = bank_state(NS), [], [0] * NS
        for s, n in pushes:
            at[s] += n
            steps, state = bank_schedule(state, s, _ready(s, at[s]) - state[0][s], WIN, HOP, BATCH, 2 * SPAN)
            ticks += [st[1] for st in steps if st[0] == "run"]
        assert any(len({q for q, _ in t}) == 3 for t in ticks)                    # a tick mixing the three sessions
        assert any(s == 0 and n > IN_RING0 - 140 - 160 for s, n in pushes)        # a chunk longer than an input ring's piece
        assert any(n == 1 for _, n in pushes) and len(ticks) >= 6                 # a one-sample push
        _CACHE["plan"] = pushes
    return _CACHE["plan"]


def _push(bank, s, k, lo, hi):
    """input samples lo .. hi-1 of session s in the k-th argument form: numpy, host tensor, device tensor (a column slice), PCM bytes"""
    q, w = _recording(s)
    if k % 4 == 0:
        return bank.push(s, w[:, lo:hi].numpy())
    if k % 4 == 1:
        return bank.push(s, w[:, lo:hi])
    if k % 4 == 2:
        return bank.push(s, w.to(DEV)[:, lo:hi])
    return bank.push_pcm(s, np.ascontiguousarray(q[:, lo:hi].numpy().T).astype("<i2").tobytes(), 2)


@pytest.mark.parametrize("tracked", [True, False])
def test_bank_at_three_rates_equals_the_bank_fed_the_resampled_recordings(tracked):
    pushes, lengths = _plan(), _lengths()
    track = _track_config() if tracked else None
    det = _detector()
    bank = det.open_bank(NS, WIN, HOP, track=track, sample_rates=RATES, in_ring_len=[IN_RING0, None, None])
    assert [r is not None for r in bank.in_rings] == [True, False, True] and bank.in_ring_len[0] == IN_RING0 and det.resampler is not None
    assert bank.in_ring_len[2] == 128 + 160 - ((-2 * SPAN * 160) // 441)          # the default: taps + M + ceil(ring_len * M / L)
    at, parts = [0] * NS, []
    for k, (s, n) in enumerate(pushes):
        parts.append(_push(bank, s, k, at[s], at[s] + n))
        at[s] += n
    assert at == lengths
    parts.append(bank.flush())
    got, ticks = bank.concat(parts), [list(t) for t in bank.ticks]
    rings = bank.chain.source.clone()
    bank.close()
    assert det.bank_captures == 1

    oracle = _detector()                                                          # today's bank on another detector
    ref = oracle.open_bank(NS, WIN, HOP, track=track)
    assert ref.in_rings == [None] * NS and oracle.resampler is None
    at, done, parts = [0] * NS, [0] * NS, []
    for s, n in pushes:
        at[s] += n
        ready = _ready(s, at[s])
        if ready > done[s]:
            parts.append(ref.push(s, _resampled(s)[:, done[s]:ready]))
            done[s] = ready
    for s in range(NS):                                                           # flush: the tails, in ascending session order
        total = _resampled(s).shape[1]
        assert total == _ready(s, lengths[s], final=True)
        if total > done[s]:
            parts.append(ref.push(s, _resampled(s)[:, done[s]:total]))
    parts.append(ref.flush())
    want, want_ticks = ref.concat(parts), [list(t) for t in ref.ticks]
    assert ticks == want_ticks and len(ticks) >= 7
    _same(got, want)
    print("rows per session", np.bincount(got[1], minlength=NS), "per window at most", max(np.bincount(got[1] * 64 + got[2])))
    assert len(got) == (4 if tracked else 3) and len(got[0]) >= 10
    # clause 1 of the contract: what each session's ring received is the whole-recording resample, bit for bit (the last ring_len samples)
    for s in range(NS):
        total, cap = _resampled(s).shape[1], 2 * SPAN
        first = max(0, total - cap, min([w for t in ticks for q, w in t if q == s]) * HOP)
        p = torch.arange(first, total, device=DEV)
        assert torch.equal(rings[s][:, p % cap].view(torch.int32), _resampled(s)[:, first:total].view(torch.int32)), s
    ref.close()


def _rounds():
    """seeded rounds {session: (lo, hi)} in input samples: mostly about 0.03 s of every session, now and then a session left out, a
    chunk longer than session 0's input piece, or one longer than a ring"""
    rng = np.random.default_rng(12)
    lengths, at, rounds = _lengths(), [0] * NS, []
    while any(a < n for a, n in zip(at, lengths)):
        r = {}
        for s in range(NS):
            if at[s] < lengths[s] and rng.random() < 0.9:
                n = int(rng.choice([1, 1323, 1323, 1323, 2000, 4500, 16000]) * _rate(s) / 44100) or 1
                r[s] = (at[s], min(lengths[s], at[s] + n))
                at[s] = r[s][1]
        if r:
            rounds.append(r)
    return rounds


def _bank(det, tracked=True):
    return det.open_bank(NS, WIN, HOP, track=_track_config() if tracked else None, sample_rates=RATES, in_ring_len=[IN_RING0, None, None])


def test_push_all_equals_the_sequential_pushes():
    rounds = _rounds()
    det = _detector()
    bank = _bank(det)
    seq = []
    for r in rounds:
        seq.append(bank.concat([bank.push(s, _recording(s)[1][:, lo:hi]) for s, (lo, hi) in sorted(r.items())]))
    seq.append(bank.flush())
    seq_ticks, seq_rings, seq_in = [list(t) for t in bank.ticks], bank.chain.source.clone(), [None if x is None else x.clone() for x in bank.in_rings]
    assert bank.launches["fast_rounds"] == 0 and bank.launches["rings_push"] == 0 and bank.launches["staging_copies"] >= len(rounds)
    bank.close()

    bank = _bank(det)
    fast = 0
    for k, (r, want) in enumerate(zip(rounds, seq)):
        before = dict(bank.launches)
        chunks = {s: _recording(s)[1][:, lo:hi] for s, (lo, hi) in r.items()}
        got = bank.push_all(chunks if k % 2 else list(reversed(list(chunks.items()))))      # a mapping, or pairs in any order
        _same(got, want)
        d = {key: bank.launches[key] - before[key] for key in before}
        assert d["fast_rounds"] + d["fallback_rounds"] == 1
        if d["fast_rounds"]:
            fast += 1
            assert d["staging_copies"] == 1 and d["rings_push"] == 1 and d["rings_resample"] <= 1, d
        else:
            assert d["rings_push"] == 0 and d["rings_resample"] == 0 and d["staging_copies"] == len(r), d
    _same(bank.flush(), seq[-1])
    print("rounds", len(rounds), bank.launches)
    assert bank.launches["fast_rounds"] == fast >= 3 and bank.launches["fallback_rounds"] >= 1 and bank.launches["rings_resample"] >= 1
    assert [list(t) for t in bank.ticks] == seq_ticks and len(seq_ticks) >= 7
    assert torch.equal(bank.chain.source.view(torch.int32), seq_rings.view(torch.int32))
    for a, b in zip(bank.in_rings, seq_in):
        assert (a is None) == (b is None) and (a is None or torch.equal(a.view(torch.int32), b.view(torch.int32)))
    with pytest.raises(ValueError, match="named twice"):
        bank.reset(0) or bank.push_all([(0, _recording(0)[1][:, :10]), (0, _recording(0)[1][:, :10])])
    with pytest.raises(RuntimeError, match="flushed"):
        bank.push_all({1: _recording(1)[1][:, :10]})
    bank.close()


def test_push_all_pcm_with_24_bit_frames_equals_push_all_of_the_decoded_floats():
    rng = np.random.default_rng(24)
    det = _detector()
    frames = {}
    for s in range(NS):
        v = (_recording(s)[0].to(torch.int32).numpy() << 8) + rng.integers(0, 256, size=_recording(s)[0].shape)      # int24 in an int32
        assert v.min() >= -(1 << 23) and v.max() < (1 << 23)
        frames[s] = v.astype(np.int32)
    chunk = {s: max(1, int(0.03 * _rate(s))) for s in range(NS)}
    n_rounds = max(-(-frames[s].shape[1] // chunk[s]) for s in range(NS))

    def run(pcm):
        bank = _bank(det, tracked=False)
        parts = []
        for k in range(n_rounds):
            part = {s: frames[s][:, k * chunk[s]:(k + 1) * chunk[s]] for s in range(NS) if k * chunk[s] < frames[s].shape[1]}
            if pcm:
                raw = {s: np.ascontiguousarray(v.T).astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes() for s, v in part.items()}
                parts.append(bank.push_all_pcm(raw, 3 if k % 2 else {s: 3 for s in raw}))
            else:
                parts.append(bank.push_all({s: (v.astype(np.float32) / np.float32(1 << 23)) for s, v in part.items()}))
        parts.append(bank.flush())
        out, ticks, launches = bank.concat(parts), [list(t) for t in bank.ticks], dict(bank.launches)
        bank.close()
        return out, ticks, launches

    got, ticks, launches = run(True)
    want, want_ticks, _ = run(False)
    assert ticks == want_ticks and len(ticks) >= 7 and launches["fast_rounds"] >= n_rounds // 2
    _same(got, want)
    assert len(got[0]) >= 10


def test_the_default_bank_is_unchanged():
    want, ticks = B._main_run()
    for rates in (None, [44100] * NS):
        det = B._detector()
        bank = det.open_bank(NS, WIN, HOP, track=_track_config(), sample_rates=rates)
        assert bank.in_rings == [None] * NS and bank.rs == [None] * NS and det.resampler is None
        at, parts = [0] * NS, []
        for k, (s, n) in enumerate(B._plan()[0]):
            parts.append(B._push(bank, s, k, at[s], at[s] + n))
            at[s] += n
        parts.append(bank.flush())
        assert [list(t) for t in bank.ticks] == ticks and bank.launches["rings_push"] == 0 and bank.launches["fast_rounds"] == 0
        _same(bank.concat(parts), want)
        bank.close()
        assert det.bank_captures == 1 and det.bank_replays == len(ticks) == 8 and det.resampler is None


def test_reset_on_a_48_khz_session_starts_its_next_recording_afresh():
    det = _detector()
    second = _recording(0, src=1)[1]                                              # session 0's second recording: session 1's audio, at 48 kHz
    bank = _bank(det)
    first = bank.push(0, _recording(0)[1][:, :11000])
    assert len(bank.ticks) == 1 and len(bank.state[2]) >= 1 and bank.in_written[0] == 11000      # one tick ran, windows wait
    bank.reset(0)
    assert bank.in_written[0] == 0 and bank.state[0][0] == 0 and not bank.state[2]
    n0 = len(bank.ticks)
    got = bank.concat([bank.push(0, second[:, :7000]), bank.push_all({0: second[:, 7000:]}), bank.flush()])
    got_ticks = [list(t) for t in bank.ticks[n0:]]
    bank.close()
    fresh = _bank(det)
    want = fresh.concat([fresh.push(0, second[:, :7000]), fresh.push(0, second[:, 7000:]), fresh.flush()])
    assert [list(t) for t in fresh.ticks] == got_ticks and len(got_ticks) >= 3
    fresh.close()
    _same(got, want)
    print("rows before the reset", len(first[0]), "behind it", len(got[0]))
    assert len(got[0]) >= 3 and (got[3].max() < 0 or got[3][got[3] >= 0].min() == 0)                             # ids from 0 again


# ---------------------------------------------------------------------------------------------- detect.py --any_rate
def test_command_line_tool_reads_three_wavs_at_their_own_rates(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    sys.path.insert(0, ROOT)
    import detect
    spec, st = _state()
    torch.save({"state_dict": st, "epoch": 3}, tmp_path / "student.pth")
    widths, chunk_s = (2, 3, 4), 0.03
    raws = []
    for k in range(NS):
        q = _recording(k)[0].numpy().T.astype(np.int64)                           # [frames, C]
        if widths[k] == 2:
            raw = q.astype("<i2").tobytes()
        elif widths[k] == 3:
            raw = np.ascontiguousarray((q << 8) + 37).astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
        else:
            raw = np.ascontiguousarray((q << 16) + 4099).astype("<i4").tobytes()
        raws.append(raw)
        with wave.open(str(tmp_path / ("mic%d.wav" % k)), "wb") as w:
            w.setnchannels(C); w.setsampwidth(widths[k]); w.setframerate(_rate(k))
            w.writeframes(raw)
    args = ["--config_file", os.path.join(ROOT, "configs", "mm-distillnet.cfg"), "--checkpoint", str(tmp_path / "student.pth"),
            "--overwrite", '{"image_size": %d}' % S, "--window_s", repr(WIN / 44100), "--hop_s", repr(HOP / 44100),
            "--chunk_s", repr(chunk_s), "--any_rate", "--output", str(tmp_path / "bank.csv")]
    for k in range(NS):
        args += ["--input", str(tmp_path / ("mic%d.wav" % k))]
    got = detect.main(args)
    # the API on the same rounds: round(chunk_s * rate) frames of every file that still has some
    det = _detector()
    bank = det.open_bank(NS, WIN, HOP, sample_rates=[_rate(k) for k in range(NS)])
    assert [r is not None for r in bank.in_rings] == [True, False, True]
    step = [int(round(chunk_s * _rate(k))) * C * widths[k] for k in range(NS)]
    parts, k_round = [], 0
    while any(k_round * step[k] < len(raws[k]) for k in range(NS)):
        parts.append(bank.push_all_pcm({k: raws[k][k_round * step[k]:(k_round + 1) * step[k]] for k in range(NS) if k_round * step[k] < len(raws[k])},
                                       list(widths)))
        k_round += 1
    parts.append(bank.flush())
    want = bank.concat(parts)
    assert bank.launches["fast_rounds"] >= k_round // 2
    bank.close()
    _same(got, want)
    assert len(want) == 3 and len(want[0]) >= 10
    lines = open(tmp_path / "bank.csv").read().splitlines()
    assert lines[0] == "session,window,t_start_s,x1,y1,x2,y2,score,label" and len(lines) == 1 + len(want[0])
    for line, r, s, w in zip(lines[1:], want[0], want[1], want[2]):
        assert line == ",".join([str(int(s)), str(int(w)), "%.9g" % (int(w) * HOP / 44100)] + ["%.9g" % float(v) for v in r])
