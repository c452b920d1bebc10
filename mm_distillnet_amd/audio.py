"""Waveform front end of the student's audio input: mel spectrograms (power or dB, and the mix of two recordings) on the GPU.

`MultimodalDetection.merge_audios` (src/datasets/MultimodalDetection.py:329-353, called per sample from `yield_batch`, :355-367) averages
two recordings' eight microphone waveforms and runs `librosa.feature.melspectrogram(sr=44100, n_fft=1024, hop_length=256, n_mels=80)` on
each channel, then resizes with cv2.INTER_CUBIC; `Audio2Spectogram` (src/datasets/transformations.py:251-266) is the same transform for
one recording.  The student's stored input is the dB map `librosa.power_to_db(S, ref=np.max)` of each microphone's spectrogram
(mp3_to_pkl.py:31-41): `db=True`.  Here the host only builds the Slaney filter bank; the spectrogram and the dB conversion are
csrc/melspec.hip (`mmd_melspec_batch`, `mmd_power_to_db`), the resize `mmd_resize_cubic_batch`.  librosa's and cv2's arithmetic is
restated, parity with the libraries themselves is unpinned.

Upstream's `librosa.load(path, sr=44100)` (mp3_to_pkl.py:31, merge_audios :335-336) also resamples whatever rate the file has; here that
first link is `Resampler` (csrc/resample.hip: `mmd_resample_poly`, and `mmd_pcm_to_float` for a WAV's raw frames).  The rule is the
project's own, pinned to tests/resample_ref.py; parity with resampy / librosa is unpinned."""
from __future__ import annotations

from fractions import Fraction

import numpy as np
import torch

N_FFT, HOP = 1024, 256


def _hz_to_mel(f):
    # Slaney scale (htk=False): linear 200/3 Hz per mel below 1 kHz, logarithmic above with 27 mels per factor 6.4
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0), f / (200.0 / 3.0))


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), (200.0 / 3.0) * m)


def mel_filters(sr: int = 44100, n_fft: int = N_FFT, n_mels: int = 80) -> np.ndarray:
    """Dense float32 [n_mels, 1 + n_fft/2] Slaney bank (fmin = 0, fmax = sr/2): row m is the triangle that rises from 0 at edge[m] to 1
    at edge[m + 1] and falls to 0 at edge[m + 2], scaled to unit area (height 2 / (edge[m + 2] - edge[m])), sampled at the FFT bin
    frequencies.  Computed in float64 and rounded once."""
    edge = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(sr / 2.0), n_mels + 2))
    left, peak, right = edge[:-2, None], edge[1:-1, None], edge[2:, None]
    hz = np.linspace(0.0, sr / 2.0, 1 + n_fft // 2)[None, :]
    rising, falling = (hz - left) / (peak - left), (right - hz) / (right - peak)
    tri = np.clip(np.minimum(rising, falling), 0.0, None)
    return (tri * (2.0 / (right - left))).astype(np.float32)


def mel_bands(sr: int = 44100, n_fft: int = N_FFT, n_mels: int = 80):
    """The bank in band form, as `mmd_melspec_power` takes it: (start int32 [n_mels], length int32 [n_mels], weights float32
    [n_mels, Lmax]) - every row of the bank is one contiguous run of bins (997 non-zero weights, at most 50 per row, at the defaults)."""
    w = mel_filters(sr, n_fft, n_mels)
    start, length = np.zeros(n_mels, np.int32), np.zeros(n_mels, np.int32)
    for m in range(n_mels):
        nz = np.flatnonzero(w[m])
        if nz.size:
            if nz[-1] - nz[0] + 1 != nz.size:
                raise ValueError(f"mel row {m} is not one contiguous run of bins")
            start[m], length[m] = nz[0], nz.size
    band = np.zeros((n_mels, max(1, int(length.max()))), np.float32)
    for m in range(n_mels):
        band[m, :length[m]] = w[m, start[m]:start[m] + length[m]]
    return start, length, band


def stream_window_starts(n_total: int, win_len: int, hop: int) -> list:
    """Sample offsets of the windows streaming detection cuts out of a recording of n_total samples: window w starts at w * hop, for
    w = 0 .. W-1 with W = 1 + (n_total - win_len) // hop.  A tail shorter than a full window is dropped.  hop is any positive number of
    samples (it may exceed win_len: the windows then leave gaps)."""
    n_total, win_len, hop = int(n_total), int(win_len), int(hop)
    if hop < 1:
        raise ValueError(f"hop = {hop}: the windows must advance by at least one sample")
    if win_len <= N_FFT // 2:
        raise ValueError(f"a window of {win_len} samples is too short for the reflect padding (more than {N_FFT // 2} needed)")
    if n_total < win_len:
        raise ValueError(f"a recording of {n_total} samples is shorter than one window of {win_len}")
    return [w * hop for w in range(1 + (n_total - win_len) // hop)]


def live_group_span(win_len: int, hop: int, batch: int) -> int:
    """Samples from the first sample of a group of `batch` consecutive windows to its last: (batch - 1) * hop + win_len"""
    return (int(batch) - 1) * int(hop) + int(win_len)


def live_schedule(written: int, group: int, n: int, win_len: int, hop: int, batch: int, cap: int):
    """What one push of n samples does to a live session's ring (`AudioDetector.open_stream`), as a list of steps in order:
    ("write", lo, hi) - absolute samples lo .. hi-1 go into the ring (hi - lo <= cap) - and ("run", g) - group g, windows g * batch ..
    g * batch + batch - 1, runs.  written: samples pushed so far; group: the next group to run.  -> (steps, written + n, next group).

    Group g covers the samples S_g = g * batch * hop .. S_g + span - 1, span = `live_group_span`.  The rule: a group runs as soon as its
    last sample is in, and a write never goes past S_g + cap for the next group g to run - the slot of sample p is that of p - cap, so
    nothing at or behind S_g, which a pending window may still need, is overwritten (cap >= span lets every group complete).  Samples
    in front of S_g are no window's any more (hop > win_len leaves such gaps between groups): they are skipped, not written.  The
    groups and their order depend on the total pushed alone, never on how it was cut into chunks.

    This is `bank_schedule` for a bank of ONE session, whose ticks are the groups: with W complete windows at `written` the session's
    state is (written, next window W, the FIFO of windows group * batch .. W - 1), a tick is windows w0 .. w0 + batch - 1 with w0 a
    multiple of batch - group w0 // batch - and the first window not yet run is group * batch, so the write limit is S_g + cap."""
    written, group, win_len, hop, batch = int(written), int(group), int(win_len), int(hop), int(batch)
    W = 0 if written < win_len else 1 + (written - win_len) // hop
    state = (written,), (W,), tuple((0, w) for w in range(group * batch, W))
    steps, (done, nxt, fifo) = bank_schedule(state, 0, n, win_len, hop, batch, cap)
    steps = [("write",) + st[2:] if st[0] == "write" else ("run", st[1][0][1] // batch) for st in steps]
    return steps, done[0], (nxt[0] - len(fifo)) // batch


def bank_state(n_sessions: int):
    """The state `bank_schedule` starts a bank of n_sessions from: (written, next, fifo) - per session the samples written so far and
    the next window to complete, and the FIFO of ready windows (session, window) in order of completion.  Tuples: a state is a value."""
    n_sessions = int(n_sessions)
    if n_sessions < 1:
        raise ValueError(f"a bank of {n_sessions} sessions")
    return (0,) * n_sessions, (0,) * n_sessions, ()


def bank_schedule(state, session: int, n: int, win_len: int, hop: int, batch: int, cap: int):
    """`live_schedule` for a bank of sessions that push independently (`AudioDetector.open_bank`): what one push of n samples to
    `session` does, as a list of steps in order: ("write", session, lo, hi) - absolute samples lo .. hi-1 of that session go into its
    ring (hi - lo <= cap) - and ("run", [(session, window), ...]) - one tick: a forward pass over those `batch` windows.
    state: (written, next, fifo) as `bank_state` gives it.  -> (steps, state').

    The rule.  Window w of session s is ready once its last sample w * hop + win_len - 1 has been pushed.  Ready windows enter ONE
    FIFO in the order they complete - inside one push that is window order.  A tick runs exactly when the FIFO holds `batch`
    windows, and takes all of them, in FIFO order.  Ring writes and ticks alternate inside a push as they do in `live_schedule`: a write to
    session s never passes (first window of s not yet run) * hop + cap - the slot of sample p is that of p - cap, so nothing a
    window of s that has not run may still need is overwritten, whatever the chunk's length.  cap >= `live_group_span`(win_len, hop,
    batch) (ValueError below that) is enough: between ticks the FIFO holds fewer than batch windows, so the first window f of s not yet
    run has fewer than batch windows of s behind it waiting, and by sample f * hop + span session s alone has completed windows
    f .. f + batch - 1 - the FIFO reached batch and the tick with f ran before the write limit f * hop + cap.  No forced short tick is
    ever needed.  Samples in front of the first window of s not yet run are no window's any more (hop > win_len leaves such gaps):
    they are skipped, not written.  The ticks and their composition depend only on the sequence of cumulative (session, samples)
    totals: cutting one push into several consecutive pushes to the same session changes nothing."""
    written, nxt, fifo = list(state[0]), list(state[1]), list(state[2])
    s, n, win_len, hop, batch, cap = int(session), int(n), int(win_len), int(hop), int(batch), int(cap)
    if not 0 <= s < len(written):
        raise ValueError(f"session {s} of a bank of {len(written)}")
    if hop < 1 or batch < 1 or n < 0:
        raise ValueError(f"hop = {hop}, batch = {batch}, n = {n}")
    span = live_group_span(win_len, hop, batch)
    if cap < span:
        raise ValueError(f"a ring of {cap} samples is shorter than one group of {batch} windows ({span} samples)")
    steps, w, end = [], written[s], written[s] + n
    while True:
        while nxt[s] * hop + win_len <= w:      # the windows the samples so far complete, in window order
            fifo.append((s, nxt[s]))
            nxt[s] += 1
            if len(fifo) == batch:
                steps.append(("run", fifo))
                fifo = []
        if w == end:
            written[s] = w
            return steps, (tuple(written), tuple(nxt), tuple(fifo))
        first = min([q[1] for q in fifo if q[0] == s], default=nxt[s])      # the first window of s not yet run
        hi = min(end, first * hop + cap)        # > w: fewer than batch windows of s wait, so w < nxt * hop + win_len <= first * hop + span
        lo = max(w, first * hop)
        if lo < hi:
            steps.append(("write", s, lo, hi))
        w = hi


def bank_round(state, pushes, win_len: int, hop: int, batch: int, cap: int):
    """One ROUND of pushes to a bank (`LiveBank.push_all`): pushes = [(session, [n_0, n_1, ...]), ...] with the sessions ascending and
    each at most once; n_i: the 44.1 kHz samples the i-th input piece of that session's chunk hands to `bank_schedule` (a 44.1 kHz
    session: one piece, the chunk itself; a session at another rate: per piece of its input ring what `live_resample_ready` newly
    allows, possibly 0).  -> (fast, steps, state', why): steps and state' are those of the SEQUENTIAL order - `bank_schedule` for every
    piece of every session in turn - which the round's results are defined by; fast says whether all the round's ring writes may be
    done first, in one batched launch, and its ticks afterwards; why names what forbids it ("pieces", "writes", "hoist") or is None.

    The rule.  fast holds when every chunk is one piece, every session has at most one write step, and every write (s, lo, hi) has
    hi <= first_s * hop + cap, first_s the first window of s that has not run AT THE START of the round (queued in the FIFO, or the
    next to complete).  Then a write moved in front of the round's ticks overwrites only slots of samples below hi - cap <= first_s * hop,
    which no window that any of those ticks runs still needs: every tick reads from the rings what it reads in the sequential order.
    Without the third clause a tick early in the round could run a queued window of s whose first samples the hoisted write of s -
    scheduled behind that tick, where it was allowed to pass them - has already replaced."""
    hop, cap = int(hop), int(cap)
    sessions = [int(s) for s, _ in pushes]
    if sessions != sorted(set(sessions)):
        raise ValueError(f"a round names every session at most once, in ascending order: {sessions}")
    _, nxt0, fifo0 = state
    steps, pieces_of = [], {}
    for s, pieces in pushes:
        pieces_of[int(s)] = len(pieces)
        for n in pieces:
            got, state = bank_schedule(state, s, n, win_len, hop, batch, cap)
            steps += got
    why = None
    for s in sessions:
        writes = [st for st in steps if st[0] == "write" and st[1] == s]
        first = min([q[1] for q in fifo0 if q[0] == s], default=nxt0[s])
        if pieces_of[s] != 1:
            why = "pieces"
        elif len(writes) > 1:
            why = "writes"
        elif writes and writes[0][3] > first * hop + cap:
            why = "hoist"
        if why is not None:
            break
    return why is None, steps, state, why


def live_pieces(n_in: int, in_written: int, written: int, L: int, M: int, half: int, in_cap: int) -> list:
    """How a push of n_in input-rate samples to a resampling session goes through its input ring of in_cap samples: [(samples of the
    piece, 44.1 kHz samples it makes ready), ...] - pieces of at most in_cap - 2 * half - M samples (the oldest input a pending output
    needs survives the piece), each followed by the outputs `live_resample_ready` newly allows.  in_written: input samples pushed so
    far; written: outputs handed to the schedule so far."""
    piece, out = int(in_cap) - 2 * int(half) - int(M), []
    if piece < 1:
        raise ValueError(f"an input ring of {in_cap} samples leaves no room for a piece behind {2 * half} taps + M = {M}")
    for off in range(0, int(n_in), piece):
        cnt = min(piece, int(n_in) - off)
        in_written += cnt
        ready = live_resample_ready(in_written, L, M, half)
        out.append((cnt, ready - written))
        written = ready
    return out


def bank_step(state):
    """The short tick: runs NOW whatever the FIFO holds (1 .. batch-1 windows; the control row pads the tick by repeating its last
    window, and the padding is not recorded).  -> (steps, state'): one ("run", windows) step, or none with an empty FIFO."""
    written, nxt, fifo = state
    return ([("run", list(fifo))] if fifo else []), (tuple(written), tuple(nxt), ())


def bank_reset(state, session: int):
    """A new recording on `session`: its position and next window back to 0, its queued windows dropped; the others keep theirs."""
    written, nxt, fifo = list(state[0]), list(state[1]), state[2]
    written[session] = nxt[session] = 0
    return tuple(written), tuple(nxt), tuple(q for q in fifo if q[0] != session)


class MelFrontEnd:
    """Holds the band-form filter bank on `device`; every call runs on the current stream and allocates only its result."""

    def __init__(self, device):
        from . import _lib
        self.call = _lib.call
        self.frames = _lib.LIB.load().mmd_melspec_frames
        self.device = torch.device(device)
        start, length, band = mel_bands()
        self.n_mels, self.stride = band.shape
        self.start = torch.from_numpy(start).to(self.device)
        self.length = torch.from_numpy(length).to(self.device)
        self.band = torch.from_numpy(band).to(self.device)

    def n_frames(self, n_samples: int) -> int:
        T = self.frames(int(n_samples))
        if T < 0:
            raise ValueError(f"a waveform of {n_samples} samples is too short for the reflect padding (more than {N_FFT // 2} needed)")
        return T

    def _check(self, wav_a, wav_b):
        if wav_a.dim() != 3 or wav_a.dtype != torch.float32 or (wav_b is not None and (wav_b.shape != wav_a.shape or wav_b.dtype != wav_a.dtype)):
            raise ValueError("melspec takes float32 [B, C, N] waveforms (two of one shape to mix them)")

    def melspec_into(self, wav_a, wav_b, db: bool, max_ws, out):
        """`melspec` into the caller's buffers, nothing allocated (a captured graph replays it): out [B, 80, T, C]; max_ws: B * C 4-byte
        words for the per-(sample, channel) maxima of the dB conversion (needs no zeroing; None for db=False)."""
        B, C, N = wav_a.shape
        self.call("mmd_melspec_batch", wav_a, wav_b, B, C, N, self.start, self.length, self.band, self.stride, 1 if db else 0, max_ws, out)
        return out

    def melspec_windows_into(self, wav, win_start, win_len: int, db: bool, max_ws, out):
        """`melspec_into` for windows read straight out of ONE recording (`mmd_melspec_windows`): wav [C, n_total], win_start int64 [B]
        on the device (each in [0, n_total - win_len]: the caller's duty), out [B, 80, n_frames(win_len), C].  The bits are those of
        `melspec_into` on the stacked slices wav[:, s : s + win_len]."""
        C, n_total = wav.shape
        self.call("mmd_melspec_windows", wav, C, n_total, win_start, win_start.shape[0], int(win_len), self.start, self.length, self.band,
                  self.stride, 1 if db else 0, max_ws, out)
        return out

    def melspec_windows_ring_into(self, ring, win_start, win_len: int, db: bool, max_ws, out):
        """`melspec_windows_into` for a ring of samples (`mmd_melspec_windows_ring`): ring [C, cap] holds absolute sample p at slot
        p % cap, win_start int64 [B] on the device are absolute positions.  The bits are those of `melspec_windows_into` on the linear
        recording."""
        C, cap = ring.shape
        self.call("mmd_melspec_windows_ring", ring, C, cap, win_start, win_start.shape[0], int(win_len), self.start, self.length,
                  self.band, self.stride, 1 if db else 0, max_ws, out)
        return out

    def melspec_windows_rings_into(self, rings, win_sess, win_start, win_len: int, db: bool, max_ws, out):
        """`melspec_windows_ring_into` for the rings of a bank of sessions (`mmd_melspec_windows_rings`): rings [n_sessions, C, cap],
        win_sess int32 [B] and win_start int64 [B] on the device: window b comes out of rings[win_sess[b]] with the bits
        `melspec_windows_ring_into` gives it there."""
        n_sessions, C, cap = rings.shape
        self.call("mmd_melspec_windows_rings", rings, n_sessions, C, cap, win_sess, win_start, win_start.shape[0], int(win_len),
                  self.start, self.length, self.band, self.stride, 1 if db else 0, max_ws, out)
        return out

    def melspec(self, wav_a: torch.Tensor, wav_b: torch.Tensor = None, db: bool = False) -> torch.Tensor:
        """[B, C, N] float32 device waveforms (the mean of the two when wav_b is given) -> mel spectrograms [B, 80, T, C], the whole batch
        in one launch sequence (`mmd_melspec_batch`).  db=False: power, as merge_audios returns it.  db=True: the dB map of the student's
        stored input, power_to_db(S, ref=np.max) per sample and microphone (mp3_to_pkl.py:31-41)."""
        self._check(wav_a, wav_b)
        B, C, N = wav_a.shape
        out = torch.empty(B, self.n_mels, self.n_frames(N), C, device=self.device)
        ws = torch.empty(B * C, device=self.device) if db else None
        return self.melspec_into(wav_a.contiguous(), None if wav_b is None else wav_b.contiguous(), db, ws, out)

    def power_to_db(self, power: torch.Tensor) -> torch.Tensor:
        """A ready-made POWER stack [B, h, w, C] (Audio2Spectogram's output) -> its dB map, in place (`mmd_power_to_db`)."""
        if power.dim() != 4 or power.dtype != torch.float32:
            raise ValueError("power_to_db takes a float32 [B, h, w, C] stack")
        B, h, w, C = power.shape
        self.call("mmd_power_to_db", power, B, h, w, C, torch.empty(B * C, device=self.device))
        return power

    def resize_into(self, mel, S: int, out):
        B, M, T, C = mel.shape
        self.call("mmd_resize_cubic_batch", mel, B, M, T, C, S, out)
        return out

    def student_input(self, wav_a: torch.Tensor, wav_b, S: int, db: bool = False) -> torch.Tensor:
        """-> [B, C, S, S]: the mel stacks (power, or dB with db=True) resized with cv2.INTER_CUBIC's rule (`mmd_resize_cubic_batch`): at
        most four launches (one a zero fill of the maxima workspace) for the whole batch.  S is the step's image_size; upstream's merge_audios hard-codes
        common_size = 768 (:330), the image_size of its shipped cfg."""
        mel = self.melspec(wav_a, wav_b, db)
        B, M, T, C = mel.shape
        return self.resize_into(mel, S, torch.empty(B, C, S, S, device=self.device))


# ---- resampling (csrc/resample.hip): a windowed-sinc interpolator after the published design of resampy's `kaiser_best` filter, as an
# exact rational polyphase filter
RS_ZEROS, RS_ROLLOFF, RS_BETA = 64, 0.9475937167399596, 14.769656459379492
RS_MAX_FACTOR = 1024                                 # cap of L and M in mmd_resample_poly
RS_MAX_TAPS = 4096                                   # and of the taps per output: 2 * ceil(64 * max(1, M / L))
RINGS_PUSH_DESC, RINGS_RS_DESC = 64, 192             # bytes per descriptor of mmd_rings_push / mmd_rings_resample (include/mmdistill.h)


def resample_len(n_in: int, sr_in: int, sr_out: int = 44100) -> int:
    """ceil(n_in * sr_out / sr_in) in integers: the samples `Resampler.resample` returns for n_in"""
    f = Fraction(int(sr_out), int(sr_in))
    return -((-int(n_in) * f.numerator) // f.denominator)


def resample_ratio(sr_in: int, sr_out: int = 44100):
    """-> (L, M, half): L / M = sr_out / sr_in in lowest terms, half = ceil(64 / min(1, L / M)) - a filter of 2 * half taps.  Raises
    ValueError, naming the reduced ratio, for what `mmd_resample_poly` does not take: L or M above 1024, or more than 4096 taps (M / L
    above 32)."""
    if int(sr_in) < 1 or int(sr_out) < 1:
        raise ValueError(f"sample rates must be positive, found {sr_in} -> {sr_out}")
    f = Fraction(int(sr_out), int(sr_in))
    L, M = f.numerator, f.denominator
    if L > RS_MAX_FACTOR or M > RS_MAX_FACTOR:
        raise ValueError(f"{sr_in} Hz -> {sr_out} Hz reduces to the ratio {L} / {M}: factors above {RS_MAX_FACTOR} are not supported")
    half = RS_ZEROS if L >= M else -((-RS_ZEROS * M) // L)
    if 2 * half > RS_MAX_TAPS:
        raise ValueError(f"{sr_in} Hz -> {sr_out} Hz reduces to the ratio {L} / {M}: its filter has {2 * half} taps, "
                         f"more than {RS_MAX_TAPS} (a reduction by more than {RS_MAX_TAPS // (2 * RS_ZEROS)} is not supported)")
    return L, M, half


def live_resample_ready(n_pushed: int, L: int, M: int, half: int, final: bool = False) -> int:
    """Outputs 0 .. ready-1 of the resampler that a live session can compute once n_pushed input samples have arrived.  Output t reads
    the inputs (t * M) // L - half + 1 .. (t * M) // L + half.  Not final: every t whose LAST tap is in, (t * M) // L + half <= n_pushed -
    1, i.e. t * M < (n_pushed - half) * L: max(0, ceil((n_pushed - half) * L / M)).  final (the recording ends at n_pushed: `flush`):
    ceil(n_pushed * L / M) = `resample_len`, the tail of the filter reading zeros.  The count depends on the total pushed alone."""
    n_pushed, L, M, half = int(n_pushed), int(L), int(M), int(half)
    if final:
        return -((-n_pushed * L) // M)
    return max(0, -((-(n_pushed - half) * L) // M))


def live_in_ring_min(L: int, M: int, half: int) -> int:
    """The fewest input samples per channel a live session's input ring may hold: the 2 * half inputs of the oldest output still to
    come, up to M inputs the ready rule leaves between two outputs, and at least one new sample per piece - 2 * half + M + 1 - and no
    fewer than the least span one block of `mmd_ring_resample` stages (`mmd_ring_resample_span`: asked of the library, no device work;
    it is at most 2 * half + M, so the first bound decides)."""
    from . import _lib
    span = _lib.LIB.load().mmd_ring_resample_span(int(L), int(M), 2 * int(half))
    if span < 0:
        raise ValueError(f"mmd_ring_resample_span refuses L = {L}, M = {M}, taps = {2 * half}")
    return max(2 * int(half) + int(M) + 1, span)


def resample_bank(sr_in: int, sr_out: int = 44100):
    """-> (L, M, half, bank float32 [L, 2 * half], phase_off int32 [L]) for sr_in -> sr_out.

    L / M = sr_out / sr_in in lowest terms, scale = min(1, L / M), half = ceil(64 / scale).  bank[p][j] = h(p / L - k) at k = j - half + 1
    with h(tau) = scale * rolloff * sinc(scale * rolloff * tau) * kaiser(tau * scale / 64), computed in float64 (the argument as the one
    quotient (p - k L) / L) and rounded once: output t is sum_j bank[(t M) % L][j] * x[(t M) // L + j - half + 1].  phase_off[r] =
    (r * M) // L is the input offset of output phase r = t % L inside its period.  Raises ValueError as `resample_ratio` does."""
    L, M, half = resample_ratio(sr_in, sr_out)
    scale = 1.0 if L >= M else L / M
    p = np.arange(L, dtype=np.int64)[:, None]
    k = np.arange(-half + 1, half + 1, dtype=np.int64)[None, :]
    tau = (p - k * L).astype(np.float64) / L
    u = tau * scale / RS_ZEROS
    inside = np.abs(u) < 1.0
    window = np.where(inside, np.i0(RS_BETA * np.sqrt(np.where(inside, 1.0 - u * u, 0.0))) / np.i0(RS_BETA), 0.0)
    bank = (scale * RS_ROLLOFF * np.sinc(scale * RS_ROLLOFF * tau) * window).astype(np.float32)
    phase_off = ((np.arange(L, dtype=np.int64) * M) // L).astype(np.int32)
    return L, M, half, bank, phase_off


class Resampler:
    """Sample-rate conversion and PCM decoding on `device`.  The filter banks are built on the host once per (sr_in, sr_out) and kept
    on the device; every call runs on the current stream and allocates only its result."""

    def __init__(self, device):
        from . import _lib
        self.call = _lib.call
        self.device = torch.device(device)
        self._banks = {}

    def _on_device(self, t: torch.Tensor, what: str):
        if not t.is_cuda or (self.device.index is not None and t.device.index != self.device.index):
            raise ValueError(f"{what}: the tensor is on {t.device}, this Resampler on {self.device}")

    def _bank(self, sr_in: int, sr_out: int):
        key = (int(sr_in), int(sr_out))
        if key not in self._banks:
            L, M, half, bank, phase_off = resample_bank(*key)
            # the kernel's layout: [taps, L] with the columns in OUTPUT-phase order r = t % L (filter phase (r M) % L), so that the lanes
            # of a wave - neighbouring outputs - read neighbouring addresses for a fixed tap
            by_out_phase = bank[(np.arange(L, dtype=np.int64) * M) % L]
            self._banks[key] = (L, M, 2 * half, torch.from_numpy(np.ascontiguousarray(by_out_phase.T)).to(self.device),
                                torch.from_numpy(phase_off).to(self.device))
        return self._banks[key]

    def resample(self, wav: torch.Tensor, sr_in: int, sr_out: int = 44100) -> torch.Tensor:
        """contiguous float32 device waveforms [..., N] at sr_in -> [..., ceil(N * sr_out / sr_in)] at sr_out (`mmd_resample_poly`, one
        launch).  sr_in == sr_out returns `wav` itself: no bank, no launch."""
        if int(sr_in) == int(sr_out):
            return wav
        if wav.dtype != torch.float32 or wav.dim() < 1 or wav.shape[-1] < 1 or not wav.is_contiguous():
            raise ValueError("resample takes contiguous float32 [..., N] waveforms")
        self._on_device(wav, "resample")
        L, M, taps, bank, phase_off = self._bank(sr_in, sr_out)
        n_in = wav.shape[-1]
        n_out = -((-n_in * L) // M)
        out = torch.empty(*wav.shape[:-1], n_out, device=self.device)
        self.call("mmd_resample_poly", wav, wav.numel() // n_in, n_in, bank, phase_off, L, M, taps, out, n_out)
        return out

    def ring_resample_into(self, in_ring: torch.Tensor, n_valid: int, sr_in: int, out_ring: torch.Tensor, t_lo: int, t_hi: int,
                           sr_out: int = 44100):
        """`resample` for a recording that arrives (`mmd_ring_resample`, one launch, nothing allocated): in_ring float32 [C, in_cap]
        holds absolute input sample p < n_valid at slot p % in_cap; the outputs t_lo .. t_hi-1 go to out_ring [C, out_cap] at slot
        t % out_cap, with the bits `resample` gives them on the whole recording (`live_resample_ready` says which are computable)."""
        L, M, taps, bank, phase_off = self._bank(sr_in, sr_out)
        self.call("mmd_ring_resample", in_ring, in_ring.shape[1], in_ring.shape[0], int(n_valid), bank, phase_off, L, M, taps, out_ring,
                  out_ring.shape[1], int(t_lo), int(t_hi))

    def rings_resample_plan(self, h_desc: np.ndarray, k: int, in_ring: torch.Tensor, n_valid: int, sr_in: int, out_ring: torch.Tensor,
                            t_lo: int, t_hi: int, sr_out: int = 44100):
        """Entry k of a host table for `rings_resample_into` (`mmd_rings_resample_plan`, host only): what `ring_resample_into` takes.
        h_desc: uint8 [>= (k + 1) * RINGS_RS_DESC] numpy memory (a view of the pinned buffer that is uploaded).  RuntimeError, the entry
        untouched, on a range `ring_resample_into` refuses."""
        if h_desc.dtype != np.uint8 or h_desc.ndim != 1 or h_desc.size < (int(k) + 1) * RINGS_RS_DESC or not h_desc.flags.c_contiguous:
            raise ValueError(f"rings_resample_plan: entry {k} needs {(int(k) + 1) * RINGS_RS_DESC} contiguous uint8 bytes")
        L, M, taps, bank, phase_off = self._bank(sr_in, sr_out)
        self.call("mmd_rings_resample_plan", h_desc.ctypes.data, int(k), in_ring, in_ring.shape[1], in_ring.shape[0], int(n_valid), bank,
                  phase_off, L, M, taps, out_ring, out_ring.shape[1], int(t_lo), int(t_hi))

    def rings_resample_into(self, h_desc: np.ndarray, d_desc: torch.Tensor, n_desc: int, channels: int):
        """`ring_resample_into` for the n_desc entries of a table in ONE launch (`mmd_rings_resample`; sessions at different rates
        share it): h_desc as `rings_resample_plan` filled it, d_desc its copy on the device (uint8; the upload is queued on the
        current stream in front of this call).  Every output has the bits `ring_resample_into` gives it."""
        self.call("mmd_rings_resample", h_desc.ctypes.data, d_desc, int(n_desc), int(channels))

    def pcm_to_float(self, raw: torch.Tensor, frames: int, channels: int, width: int) -> torch.Tensor:
        """interleaved little-endian signed PCM, raw uint8 [frames * channels * width] on the device (a WAV's frames as read) ->
        float32 [channels, frames] in [-1, 1) (`mmd_pcm_to_float`): 16-bit / 2^15, 24-bit / 2^23, 32-bit rounded to float32 then / 2^31."""
        if raw.dtype != torch.uint8 or raw.numel() != int(frames) * int(channels) * int(width) or not raw.is_contiguous():
            raise ValueError(f"pcm_to_float takes {frames} * {channels} * {width} contiguous uint8 bytes, found {raw.numel()} of {raw.dtype}")
        self._on_device(raw, "pcm_to_float")
        out = torch.empty(int(channels), int(frames), device=self.device)
        self.call("mmd_pcm_to_float", raw, int(frames), int(channels), int(width), out)
        return out


# ---- one round of ring writes in one launch (csrc/live.hip: `mmd_rings_push`), beside `Resampler.ring_resample_into` / `rings_resample_into`
def rings_push_entry(h_desc: np.ndarray, k: int, src_off: int, src_stride: int, n: int, kind: int, ring: torch.Tensor, cap: int, pos: int):
    """Entry k of a host table for `rings_push_into`: h_desc int64 [>= k + 1, 8].  The chunk lies src_off bytes behind the launch's base:
    kind 0, float32 rows src_stride floats apart; kind 2 / 3 / 4, interleaved PCM frames of that width.  Its n samples per channel go
    to ring (float32 [C, cap] on the device, or the address of one) at the absolute position pos, reduced modulo cap here."""
    ptr = ring.data_ptr() if isinstance(ring, torch.Tensor) else int(ring)
    h_desc[k] = (int(src_off), int(src_stride), int(n), int(kind), ptr, int(cap), int(pos) % int(cap), 0)


def rings_push_into(src_base, h_desc: np.ndarray, d_desc, n_desc: int, channels: int):
    """The n_desc ring writes of a host table in ONE launch (`mmd_rings_push`): src_base, a device tensor or address the entries'
    src_off count from; h_desc int64 [>= n_desc, 8] as `rings_push_entry` filled it; d_desc its copy on the device (the upload is queued
    on the current stream in front of this call).  Every ring gets the bits `mmd_ring_push` / `mmd_ring_push_pcm` give it."""
    from . import _lib
    if h_desc.dtype != np.int64 or h_desc.ndim != 2 or h_desc.shape[1] != 8 or h_desc.shape[0] < int(n_desc) or not h_desc.flags.c_contiguous:
        raise ValueError("rings_push_into takes a contiguous int64 [>= n_desc, 8] host table")
    _lib.call("mmd_rings_push", src_base, h_desc.ctypes.data, d_desc, int(n_desc), int(channels))
