"""A LiveSession and a LiveBank of ONE session share their host path (detector._LiveHost) and differ in their chains alone.  Pinned
here from both sides: the recording of tests/test_gpu_live.py, cut into the same chunks, goes through `open_stream(batch=3)` on one
detector and through `open_bank(1, batch=3)` on a second one with the same weights.  Rows, windows and track ids are equal bit for bit
push by push (each equals `detect` on the stacked windows of the same groups), the bank's ticks are the session's groups, and at
48 kHz - an input ring so small that a chunk is several pieces - the 44.1 kHz rings both resampled into are equal too.  The
detectors, recordings and oracles are those of tests/test_gpu_live.py and tests/test_gpu_live_resample.py, shared through their caches."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIN, HOP, BATCH = 4096, 1531, 3           # W = 7 windows in 14,000 samples: two full groups, one of one window
SPAN = (BATCH - 1) * HOP + WIN


def _case(rate):
    """-> (the test module whose detector is tuned for the recording, the recording at `rate`, chunk lengths, in_ring_len)"""
    if rate is None:
        import test_gpu_live as T
        return T, T._recording(11), [1, 2999, 7500, 1, 3499], None                    # a 1-sample chunk; 7500 > the ring of one span
    import test_gpu_live_resample as T
    return T, T._recording48(11), [1, 3299, 8200, 1, 3737], T.IN_MIN + 999            # pieces of 1000 samples: 8200 is nine of them


@pytest.mark.parametrize("rate", [None, 48000])
def test_a_session_and_a_bank_of_one_session_give_the_same_bits(rate):
    T, w, lengths, in_ring_len = _case(rate)
    assert (T.WIN, T.HOP, T.BATCH, T.S, T.N_REC) == (WIN, HOP, BATCH, 128, 14000)
    want = T._oracle(11, True)                                                        # track_stream on the whole (resampled) recording
    chunks = [c.to(DEV) if k % 2 else c for k, c in enumerate(T._cut(w, lengths))]    # device and host chunks alike
    det_s, det_b = T._detector(), T._detector()
    session = det_s.open_stream(WIN, HOP, batch=BATCH, track=T._track_config(), ring_len=SPAN, sample_rate=rate, in_ring_len=in_ring_len)
    bank = det_b.open_bank(1, WIN, HOP, batch=BATCH, track=T._track_config(), ring_len=SPAN, sample_rates=None if rate is None else [rate],
                           in_ring_len=in_ring_len)
    assert not hasattr(session, "ticks") and bank.ticks == []
    parts = []
    for c in chunks + [None]:                                                         # None: the flush
        a, b = (session.flush(), bank.flush()) if c is None else (session.push(c), bank.push(0, c))
        assert len(b) == 4 and b[1].dtype == np.int32 and not b[1].any()              # the bank's session column: all zero
        T._same(a, (b[0], b[2], b[3]))
        assert len(bank.ticks) == session.group + (c is None) and bank.state[0][0] == session.written
        parts.append(a)
    got = tuple(np.concatenate([p[i] for p in parts]) for i in range(3))
    T._same(got, want)                                                                # and both are the stream's (it holds rows: `_oracle`)
    assert bank.ticks == [[(0, 0), (0, 1), (0, 2)], [(0, 3), (0, 4), (0, 5)], [(0, 6)]] and session.group == 2
    assert (det_s.live_captures, det_s.live_replays, det_b.bank_captures, det_b.bank_replays) == (1, 3, 1, 3)
    assert session.launches["staging_copies"] == bank.launches["staging_copies"] == 3
    if rate is not None:
        assert session.in_written == bank.in_written[0] == w.shape[1] and session.in_ring_len == bank.in_ring_len[0] == in_ring_len
        assert torch.equal(session.in_ring.view(torch.int32), bank.in_rings[0].view(torch.int32))
    ring_s, ring_b = session.chain.source, bank.chain.source
    assert ring_s.shape == (8, SPAN) and ring_b.shape == (1, 8, SPAN) and ring_s.abs().max() > 0
    assert torch.equal(ring_s.view(torch.int32), ring_b[0].view(torch.int32))         # the 44.1 kHz rings
    session.close()
    bank.close()
