#!/usr/bin/env python3
"""Audio-only detection with the trained student: a checkpoint plus microphone waveforms in, boxes out.

    python detect.py --config_file F --checkpoint P --input X --output out.csv [--overwrite JSON]
                     [--window_s SECONDS [--hop_s SECONDS] [--batch N]
                      [--track [--track_iou X] [--track_beta X] [--track_max_age N] [--track_max N]]]
                     [--resample | --sample_rate R] [--chunk_s SECONDS | --live_s SECONDS]
    python detect.py --config_file F --checkpoint P --input X0 --input X1 [--input X2 ...] --output out.csv
                     --window_s SECONDS --chunk_s SECONDS [--any_rate] [--hop_s SECONDS] [--batch N] [--track ...]

X is a `.npy` holding float32 waveforms `[8, N]` (one clip) or `[B, 8, N]`, or an 8-channel 16-bit PCM `.wav` at 44.1 kHz (one clip;
samples / 32768).  The waveforms go through the device front end (mel spectrogram, power_to_db per microphone, cubic resize to
image_size: what mp3_to_pkl.py:31-41, `MultimodalDetection.__getitem__` and `Resizer` make of a recording upstream), the student's
eval-mode forward and the post-processing of the reference's evaluation (score > conf_threshold, class filter, NMS).  The detection
settings (image_size, conf_threshold, nms_threshold, valid_labels, precision, compound_coef) are read from the cfg file like train.py
and evaluate.py read them.  No teacher is built or loaded.  Output: one CSV row per box, columns clip,x1,y1,x2,y2,score,label.

With --window_s the input is ONE recording (a `.wav`, or a `.npy` of shape [8, N]) and the detector slides over it on the device
(`AudioDetector.detect_stream`): windows of round(window_s * 44100) samples every round(hop_s * 44100) samples (hop_s defaults to
window_s), --batch windows per launch sequence; a tail shorter than a window is dropped.  The CSV then has the columns
window,t_start_s,x1,y1,x2,y2,score,label with t_start_s = window * hop / 44100.

With --track (only with --window_s) the boxes of consecutive windows are linked into tracks on the device
(`AudioDetector.track_stream`: greedy IoU association with a constant-velocity model) and the CSV gains a last column `track`: the id of
the row's track - ids start at 0 and rise in order of birth - or -1.  --track_iou: smallest IoU of a pairing (0.3); --track_beta: velocity
gain (0.5); --track_max_age: windows a track survives without a box (2); --track_max: live tracks at a time (64, at most 256).

With --resample a `.wav` may have any sample rate and 16-, 24- or 32-bit PCM samples (8 channels): its frames go to the device as they
are in the file, are decoded there and resampled to 44.1 kHz (`mm_distillnet_amd.audio.Resampler`: what `librosa.load(path, sr=44100)`
does upstream, by this project's own windowed-sinc rule).  With --sample_rate R a `.npy` is taken to be at R Hz and resampled when
R != 44100.  Everything behind that - the clip, --window_s and --track paths - runs unchanged on the 44.1 kHz waveforms; window and hop
sizes and the CSV's times stay in seconds of the recording.  Without these two flags every input is read as described above.

With --chunk_s X (only with --window_s) the recording is never whole in host or device memory: it is read X seconds at a time - a
`.wav` with `wave.readframes`, its frames decoded on the device; a `.npy` through a memory map - and fed to a live session
(`AudioDetector.open_stream`), which keeps a bounded ring of samples on the device and runs each group of --batch windows as soon as
its last sample has arrived.  The CSV is byte for byte the one the same command writes without --chunk_s, with or without --track.
--chunk_s does not go with --resample / --sample_rate: it reads 44.1 kHz input only.

With --live_s X (only with --window_s, not with --chunk_s) a recording of ANY rate is read X seconds - round(X * R) frames - at a time
at its own rate R and fed to a live session that resamples as the chunks arrive (`AudioDetector.open_stream(sample_rate=R)`: the
resampler's filter history is carried across chunks in a ring of input samples on the device).  A `.wav`: 8 channels of 16-, 24- or
32-bit PCM, R from its header (--resample alongside is allowed and changes nothing); a `.npy` of shape [8, N]: through a memory map, at
--sample_rate R (default 44100).  Window count and CSV times are those of the ceil(N * 44100 / R) resampled samples, and the CSV is
byte for byte the one --resample --window_s ... (for a `.npy`: --sample_rate R --window_s ...) writes for the same file, with or
without --track.

With several --input (only with --window_s and --chunk_s) every file is one recording of its own - several microphone arrays side by
side - and they go through ONE bank of live sessions (`AudioDetector.open_bank`), session k = the k-th --input.  The files are read
--chunk_s at a time in round robin, exhausted files drop out of the rotation, and one forward pass serves --batch ready windows of
whichever recordings completed them (--batch defaults to the number of files: one fresh window of each).  The CSV gains a first column:
session,window,t_start_s,x1,y1,x2,y2,score,label[,track]; window and track ids count per session, and the rows come in the order the
bank ran them.  Several inputs do not go with --resample / --sample_rate / --live_s: without --any_rate the bank reads 44.1 kHz input only.

With --any_rate (only with several --input, --window_s and --chunk_s) every file is a `.wav` of 8 channels of 16-, 24- or 32-bit PCM at
ANY rate, each session at the rate R in its file's header (`AudioDetector.open_bank(sample_rates=...)`: the session resamples to 44.1 kHz
as its chunks arrive).  The files are read round by round, round(chunk_s * R) frames of every file that still has some, and each
round is ONE `LiveBank.push_all_pcm`: one staging copy and one launch for the ring writes of all sessions, one for their resampling.  The
CSV has the same columns; window counts and times are those of the ceil(N * 44100 / R) resampled samples, in seconds of the recording.
A `.npy` is refused under --any_rate (it holds no rate).
"""
import argparse
import csv
import os
import sys
import wave

import numpy as np

if os.environ.get("MMD_HW_QUEUES"):       # as train.py / evaluate.py: must be set before the HIP runtime starts
    os.environ.setdefault("GPU_MAX_HW_QUEUES", os.environ["MMD_HW_QUEUES"])
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import train as T  # noqa: E402
from mm_distillnet_amd.detector import AudioDetector  # noqa: E402

CHANNELS, SAMPLE_RATE = 8, 44100
COLUMNS = ("clip", "x1", "y1", "x2", "y2", "score", "label")
STREAM_COLUMNS = ("window", "t_start_s", "x1", "y1", "x2", "y2", "score", "label")
TRACK_COLUMNS = STREAM_COLUMNS + ("track",)
BANK_COLUMNS = ("session",) + STREAM_COLUMNS


def read_npy(path: str) -> np.ndarray:
    a = np.load(path, allow_pickle=False)
    if a.dtype != np.float32:
        raise ValueError(f"{path}: waveforms must be float32, found {a.dtype}")
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or a.shape[1] != CHANNELS:
        raise ValueError(f"{path}: expected [{CHANNELS}, N] or [B, {CHANNELS}, N] waveforms, found shape {a.shape}")
    return np.ascontiguousarray(a)


def _check_wav(path: str, w, any_rate: bool):
    """The header rules of an open `wave` reader -> (bytes per sample, rate in Hz).  any_rate False: 8 channels of 16-bit PCM at 44.1 kHz,
    what the front end takes as it is; True: 8 channels of 16-, 24- or 32-bit PCM at any rate, what the device decodes and resamples."""
    width, rate, channels = w.getsampwidth(), w.getframerate(), w.getnchannels()
    if not any_rate and rate != SAMPLE_RATE:
        raise ValueError(f"{path}: sample rate {rate} Hz is not supported (the front end is built for {SAMPLE_RATE} Hz; resample first)")
    if w.getcomptype() != "NONE" or width not in ((2, 3, 4) if any_rate else (2,)):
        bits = "16-, 24- or 32-bit" if any_rate else "16-bit"
        raise ValueError(f"{path}: only {bits} PCM is supported, found {8 * width}-bit {w.getcomptype()}")
    if channels != CHANNELS:
        raise ValueError(f"{path}: expected {CHANNELS} microphone channels, found {channels}")
    if rate < 1:
        raise ValueError(f"{path}: sample rate {rate} Hz")
    return width, rate


def _wav_chunks(w, chunk: int, width: int):
    """(raw whole frames, bytes per sample) of an open `wave` reader, `chunk` frames at a time; closes the reader behind the last"""
    with w:
        while True:
            raw = w.readframes(chunk)
            if len(raw) < width * CHANNELS:
                return
            yield raw[:len(raw) - len(raw) % (width * CHANNELS)], width


def read_wav(path: str) -> np.ndarray:
    with wave.open(path, "rb") as w:
        _check_wav(path, w, any_rate=False)
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").reshape(-1, CHANNELS)
    return np.ascontiguousarray((pcm.astype(np.float32) / np.float32(32768.0)).T)[None]


def read_input(path: str) -> np.ndarray:
    """-> float32 [B, 8, N]"""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npy":
        return read_npy(path)
    if ext == ".wav":
        return read_wav(path)
    raise ValueError(f"{path}: unsupported input (a .npy of float32 waveforms or an 8-channel 16-bit PCM .wav at 44.1 kHz)")


def read_recording(path: str):
    """A PCM `.wav` of 8 channels at ANY rate, 16-, 24- or 32-bit -> (its frames as a uint8 array, just as they are in the file:
    interleaved little-endian signed samples; frames; channels; bytes per sample; rate in Hz).  Nothing is decoded on the host:
    `Resampler.pcm_to_float` and `Resampler.resample` take it from there (--resample)."""
    with wave.open(path, "rb") as w:
        width, rate = _check_wav(path, w, any_rate=True)
        raw = np.frombuffer(w.readframes(w.getnframes()), dtype=np.uint8)
    frames = raw.size // (CHANNELS * width)
    if frames < 1:
        raise ValueError(f"{path}: no frames")
    return raw[:frames * CHANNELS * width].copy(), frames, CHANNELS, width, rate


def load_resampled(a, dev):
    """--resample / --sample_rate: -> float32 DEVICE waveforms [B, 8, N] at 44.1 kHz"""
    from mm_distillnet_amd.audio import Resampler
    ext = os.path.splitext(a.input)[1].lower()
    if a.resample:
        if ext != ".wav" or a.sample_rate is not None:
            raise ValueError(f"{a.input}: --resample reads a .wav, whose header holds the rate (for a .npy give --sample_rate R alone)")
        raw, frames, channels, width, rate = read_recording(a.input)
        rs = Resampler(dev)
        wav = rs.pcm_to_float(torch.from_numpy(raw).to(dev), frames, channels, width)[None]
    else:
        if ext != ".npy":
            raise ValueError(f"{a.input}: --sample_rate R says at which rate a .npy was recorded (a .wav holds its rate: --resample)")
        if a.sample_rate < 1:
            raise ValueError(f"--sample_rate {a.sample_rate}: a positive number of Hz")
        rs = Resampler(dev)
        wav, rate = torch.from_numpy(read_npy(a.input)).to(dev), a.sample_rate
    return rs.resample(wav, rate, SAMPLE_RATE)


def write_csv(path: str, rows_per_clip) -> int:
    n = 0
    with open(path, "w", newline="") as f:
        out = csv.writer(f)
        out.writerow(COLUMNS)
        for clip, rows in enumerate(rows_per_clip):
            for r in np.asarray(rows, np.float32).reshape(-1, 6):
                out.writerow([clip] + ["%.9g" % float(v) for v in r])      # 9 digits: float32 round-trips
                n += 1
    return n


def _write_windows_csv(path: str, columns, rows, window, hop: int, track=None) -> int:
    """one row per box: window, its start in seconds, the box[, its track id]"""
    rows, window = np.asarray(rows, np.float32).reshape(-1, 6), np.asarray(window).reshape(-1)
    last = [[]] * len(rows)
    if track is not None:
        track = np.asarray(track).reshape(-1)
        if len(track) != len(rows) or len(window) != len(rows):
            raise ValueError("write_track_csv: %d rows, %d windows, %d track ids" % (len(rows), len(window), len(track)))
        last = [[t] for t in track.tolist()]
    with open(path, "w", newline="") as f:
        out = csv.writer(f)
        out.writerow(columns)
        for w, r, t in zip(window.tolist(), rows, last):
            out.writerow([w, "%.9g" % (w * hop / SAMPLE_RATE)] + ["%.9g" % float(v) for v in r] + t)
    return len(rows)


def write_stream_csv(path: str, rows, window, hop: int) -> int:
    """rows [R, 6] / window [R] of `AudioDetector.detect_stream` at a hop of `hop` samples"""
    return _write_windows_csv(path, STREAM_COLUMNS, rows, window, hop)


def write_track_csv(path: str, rows, window, track, hop: int) -> int:
    """rows [R, 6] / window [R] / track [R] of `AudioDetector.track_stream` at a hop of `hop` samples"""
    return _write_windows_csv(path, TRACK_COLUMNS, rows, window, hop, track)


def write_bank_csv(path: str, rows, session, window, hop: int, track=None) -> int:
    """rows [R, 6] / session [R] / window [R][ / track [R]] of a `LiveBank` at a hop of `hop` samples"""
    rows, session, window = np.asarray(rows, np.float32).reshape(-1, 6), np.asarray(session).reshape(-1), np.asarray(window).reshape(-1)
    last = [[]] * len(rows) if track is None else [[t] for t in np.asarray(track).reshape(-1).tolist()]
    if not (len(session) == len(window) == len(last) == len(rows)):
        raise ValueError("write_bank_csv: %d rows, %d sessions, %d windows, %d track ids" % (len(rows), len(session), len(window), len(last)))
    with open(path, "w", newline="") as f:
        out = csv.writer(f)
        out.writerow(BANK_COLUMNS + (("track",) if track is not None else ()))
        for q, w, r, t in zip(session.tolist(), window.tolist(), rows, last):
            out.writerow([q, w, "%.9g" % (w * hop / SAMPLE_RATE)] + ["%.9g" % float(v) for v in r] + t)
    return len(rows)


def stream_sizes(window_s: float, hop_s, n_total: int):
    """-> (win_len, hop, number of windows) in samples; raises ValueError as `stream_window_starts` does"""
    from mm_distillnet_amd.audio import stream_window_starts
    win_len = int(round(window_s * SAMPLE_RATE))
    hop = win_len if hop_s is None else int(round(hop_s * SAMPLE_RATE))
    return win_len, hop, len(stream_window_starts(n_total, win_len, hop))


def check_chunk_flags(a):
    """--chunk_s: what can be refused from the flags alone, before any device work"""
    if a.chunk_s is None:
        return
    if a.window_s is None:
        raise ValueError("--chunk_s feeds a live session that slides a window over the recording: it needs --window_s")
    if a.resample or a.sample_rate is not None:
        raise ValueError("--chunk_s does not go with --resample / --sample_rate: it reads 44.1 kHz input only "
                         "(--live_s reads a recording of any rate a chunk at a time and resamples it as it arrives)")
    if not a.chunk_s > 0 or int(round(a.chunk_s * SAMPLE_RATE)) < 1:
        raise ValueError(f"--chunk_s {a.chunk_s}: a positive number of seconds (at least one sample)")
    if os.path.splitext(a.input)[1].lower() not in (".npy", ".wav"):
        raise ValueError(f"{a.input}: unsupported input (a .npy of float32 waveforms or an 8-channel 16-bit PCM .wav at 44.1 kHz)")


def check_bank_flags(a):
    """several --input: what can be refused from the flags alone, before any device work"""
    if len(a.inputs) < 2:
        if a.any_rate:
            raise ValueError("--any_rate is for several --input, each session at its file's rate (one recording of any rate: --live_s)")
        return
    if a.window_s is None or a.chunk_s is None:
        raise ValueError("several --input are read side by side into a bank of live sessions: they need --window_s and --chunk_s")
    if a.any_rate and (a.resample or a.sample_rate is not None or a.live_s is not None):
        raise ValueError("--any_rate does not go with --resample / --sample_rate / --live_s: every .wav is read at the rate in its header")
    if a.resample or a.sample_rate is not None or a.live_s is not None:
        raise ValueError("several --input do not go with --resample / --sample_rate / --live_s: the bank reads 44.1 kHz input only")
    if not a.chunk_s > 0 or int(round(a.chunk_s * SAMPLE_RATE)) < 1:
        raise ValueError(f"--chunk_s {a.chunk_s}: a positive number of seconds (at least one sample)")
    for path in a.inputs:
        if a.any_rate and os.path.splitext(path)[1].lower() != ".wav":
            raise ValueError(f"{path}: --any_rate reads 8-channel PCM .wav files, whose headers hold their rates (a .npy holds none)")
        if os.path.splitext(path)[1].lower() not in (".npy", ".wav"):
            raise ValueError(f"{path}: unsupported input (a .npy of float32 waveforms or an 8-channel 16-bit PCM .wav at 44.1 kHz)")
    if a.batch is not None and a.batch < 1:
        raise ValueError(f"--batch {a.batch}")


def check_live_flags(a):
    """--live_s: what can be refused from the flags alone, before any device work"""
    if a.live_s is None:
        return
    if a.window_s is None:
        raise ValueError("--live_s feeds a live session that slides a window over the recording: it needs --window_s")
    if a.chunk_s is not None:
        raise ValueError("--live_s does not go with --chunk_s: one of the two says how the recording is cut into chunks")
    if not a.live_s > 0:
        raise ValueError(f"--live_s {a.live_s}: a positive number of seconds (at least one frame)")
    ext = os.path.splitext(a.input)[1].lower()
    if ext not in (".npy", ".wav"):
        raise ValueError(f"{a.input}: unsupported input (a .npy of float32 waveforms at --sample_rate, or an 8-channel PCM .wav of any rate)")
    if ext == ".wav" and a.sample_rate is not None:
        raise ValueError(f"{a.input}: a .wav holds its rate: --live_s reads it from the header (--sample_rate R is for a .npy)")
    if ext == ".npy" and a.resample:
        raise ValueError(f"{a.input}: --resample reads a .wav; --live_s takes a .npy at --sample_rate R")
    rate = SAMPLE_RATE if a.sample_rate is None else a.sample_rate
    if rate < 1:
        raise ValueError(f"--sample_rate {a.sample_rate}: a positive number of Hz")
    if ext == ".npy" and int(round(a.live_s * rate)) < 1:
        raise ValueError(f"--live_s {a.live_s}: a positive number of seconds (at least one frame)")


def open_live(path: str, live_s: float, sample_rate=None):
    """-> (n_frames, rate, chunks): the recording's length in frames at its own rate in Hz and an iterator over it round(live_s * rate)
    frames at a time - (raw frames, bytes per sample) of a 16-, 24- or 32-bit PCM `.wav` of any rate (for `LiveSession.push_pcm`; the
    checks are `read_recording`'s), (float32 [8, n], None) of a `.npy` taken to be at sample_rate (default 44100; for `push`).  Only
    one chunk is in host memory at a time."""
    if os.path.splitext(path)[1].lower() == ".wav":
        w = wave.open(path, "rb")
        try:
            width, rate = _check_wav(path, w, any_rate=True)
            chunk = int(round(live_s * rate))
            if chunk < 1:
                raise ValueError(f"--live_s {live_s}: a positive number of seconds (at least one frame at {rate} Hz)")
        except ValueError:
            w.close()
            raise
        return w.getnframes(), rate, _wav_chunks(w, chunk, width)
    rate = SAMPLE_RATE if sample_rate is None else int(sample_rate)
    n_total, chunks = open_chunked(path, int(round(live_s * rate)))
    return n_total, rate, chunks


def open_chunked(path: str, chunk: int):
    """-> (n_total, chunks): the recording's length in samples and an iterator over it `chunk` samples at a time - (raw frames, 2) of a
    16-bit `.wav` (for `LiveSession.push_pcm`), (float32 [8, n], None) of a `.npy` (for `push`).  The checks are `read_wav`'s and
    `read_npy`'s; only one chunk is in host memory at a time."""
    if os.path.splitext(path)[1].lower() == ".wav":
        w = wave.open(path, "rb")
        try:
            width, _ = _check_wav(path, w, any_rate=False)
        except ValueError:
            w.close()
            raise
        return w.getnframes(), _wav_chunks(w, chunk, width)
    m = np.load(path, mmap_mode="r", allow_pickle=False)
    if m.dtype != np.float32:
        raise ValueError(f"{path}: waveforms must be float32, found {m.dtype}")
    if m.ndim == 3 and m.shape[0] == 1:
        m = m[0]
    if m.ndim != 2 or m.shape[0] != CHANNELS:
        raise ValueError(f"{path}: --window_s takes ONE recording (a .wav, or a .npy of shape [{CHANNELS}, N]), found shape {m.shape}")
    return m.shape[1], ((np.ascontiguousarray(m[:, i:i + chunk]), None) for i in range(0, m.shape[1], chunk))


def run_chunked(det, chunks, win_len: int, hop: int, batch: int, track, sample_rate=None):
    """Feeds the chunks of `open_chunked` / `open_live` (those at sample_rate) to a live session -> what `detect_stream` /
    `track_stream` return for the whole recording (resampled to 44.1 kHz)"""
    session = det.open_stream(win_len, hop, batch=batch, track=track, sample_rate=sample_rate)
    parts = [session.push(c) if width is None else session.push_pcm(c, width) for c, width in chunks]
    parts.append(session.flush())
    session.close()
    return session.concat(parts)


def run_bank(det, sources: list, win_len: int, hop: int, batch: int, track):
    """sources: the chunk iterators of `open_chunked`, one per session -> what the bank returns for the round robin over them: one chunk
    of every file that still has one, in file order, again and again; `flush` at the end"""
    bank = det.open_bank(len(sources), win_len, hop, batch=batch, track=track)
    parts, live = [], list(enumerate(iter(src) for src in sources))
    while live:
        still = []
        for k, it in live:
            got = next(it, None)
            if got is None:
                continue
            c, width = got
            parts.append(bank.push(k, c) if width is None else bank.push_pcm(k, c, width))
            still.append((k, it))
        live = still
    parts.append(bank.flush())
    bank.close()
    return bank.concat(parts)


def run_bank_rounds(det, sources: list, rates: list, win_len: int, hop: int, batch: int, track):
    """sources: the chunk iterators of `open_live`, one per session at rates[k] -> what the bank returns for the rounds over them:
    one `push_all_pcm` per round with a chunk of every file that still has one; `flush` at the end"""
    bank = det.open_bank(len(sources), win_len, hop, batch=batch, track=track, sample_rates=rates)
    parts, live = [], list(enumerate(iter(src) for src in sources))
    while live:
        got = [(k, it, next(it, None)) for k, it in live]
        live = [(k, it) for k, it, c in got if c is not None]
        if live:
            parts.append(bank.push_all_pcm({k: c[0] for k, _, c in got if c is not None}, {k: c[1] for k, _, c in got if c is not None}))
    parts.append(bank.flush())
    bank.close()
    return bank.concat(parts)


def parse_args(argv=None):
    """-> the arguments; a.input is the one --input (as it always was) or, with several, the first, and a.inputs lists them all.
    --batch: None when not given - 8 with one input, the number of inputs with several."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--config_file", required=True)
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--input", required=True, action="append", help="a recording; several (with --window_s --chunk_s): one bank session each")
    ap.add_argument("--output", required=True)
    ap.add_argument("--overwrite", type=str, default=None)
    ap.add_argument("--window_s", type=float, default=None, help="slide a window of this many seconds over ONE recording")
    ap.add_argument("--hop_s", type=float, default=None, help="seconds between window starts (default: --window_s)")
    ap.add_argument("--batch", type=int, default=None, help="windows per launch sequence (with --window_s; default 8, with several --input their number)")
    ap.add_argument("--track", action="store_true", help="link the boxes of consecutive windows into tracks (with --window_s)")
    ap.add_argument("--track_iou", type=float, default=0.3, help="smallest IoU at which a track and a box are paired")
    ap.add_argument("--track_beta", type=float, default=0.5, help="velocity gain of the constant-velocity model")
    ap.add_argument("--track_max_age", type=int, default=2, help="windows a track survives without a box")
    ap.add_argument("--track_max", type=int, default=64, help="live tracks at a time (1 .. 256)")
    ap.add_argument("--resample", action="store_true", help="a .wav of any rate, 16/24/32-bit PCM: decode and resample to 44.1 kHz on the device")
    ap.add_argument("--sample_rate", type=int, default=None, help="the rate in Hz of a .npy input; resampled to 44.1 kHz on the device")
    ap.add_argument("--chunk_s", type=float, default=None, help="read the recording this many seconds at a time into a live session (with --window_s)")
    ap.add_argument("--any_rate", action="store_true", help="several .wav inputs, each at the rate in its header (with --window_s --chunk_s)")
    ap.add_argument("--live_s", type=float, default=None, help="read a recording of any rate this many seconds at a time into a live session that resamples (with --window_s)")
    a = ap.parse_args(argv)
    a.inputs, a.input = a.input, a.input[0]
    check_bank_flags(a)
    if len(a.inputs) == 1 and a.batch is None:
        a.batch = 8
    check_chunk_flags(a)
    check_live_flags(a)
    return a


def main_bank(a, cfg, track):
    """several --input through one bank"""
    if a.any_rate:
        from mm_distillnet_amd.audio import resample_len, resample_ratio
        opened = [open_live(path, a.chunk_s) for path in a.inputs]
        rates = [rate for _, rate, _ in opened]
        for rate in rates:
            resample_ratio(rate)                  # an unsupported ratio is refused before any device work
        opened = [(resample_len(n_frames, rate, SAMPLE_RATE), chunks) for n_frames, rate, chunks in opened]
    else:
        chunk = int(round(a.chunk_s * SAMPLE_RATE))
        opened = [open_chunked(path, chunk) for path in a.inputs]
    sizes = [stream_sizes(a.window_s, a.hop_s, n_total) for n_total, _ in opened]
    win_len, hop, n_win = sizes[0][0], sizes[0][1], sum(z[2] for z in sizes)
    torch.cuda.set_device(0)
    sspec, _ = T.load_student_state(int(cfg.get("compound_coef", 2)))
    c = torch.load(a.checkpoint, map_location="cpu", weights_only=False)
    det = AudioDetector.from_step_config(sspec, "cuda:0", T.step_config(cfg))
    det.load(c["state_dict"] if "state_dict" in c else c)
    batch = len(a.inputs) if a.batch is None else a.batch
    if a.any_rate:
        got = run_bank_rounds(det, [chunks for _, chunks in opened], rates, win_len, hop, batch, track)
    else:
        got = run_bank(det, [chunks for _, chunks in opened], win_len, hop, batch, track)
    n = write_bank_csv(a.output, *got[:3], hop, got[3] if track is not None else None)
    print("%d sessions, %d windows, %d boxes -> %s" % (len(a.inputs), n_win, n, a.output))
    return got


def main(argv=None):
    a = parse_args(argv)
    track = None
    if a.track:
        if a.window_s is None:
            raise ValueError("--track links the boxes of consecutive windows: it needs --window_s")
        from mm_distillnet_amd.tracker import TrackConfig
        track = TrackConfig(iou_min=a.track_iou, beta=a.track_beta, max_age=a.track_max_age, max_tracks=a.track_max)
    cfg, _ = T.parse_config(["--config_file", a.config_file] + (["--overwrite", a.overwrite] if a.overwrite else []))
    if len(a.inputs) > 1:
        return main_bank(a, cfg, track)
    dev = "cuda:0"
    resampled = a.resample or a.sample_rate is not None
    chunked, rate = a.chunk_s is not None or a.live_s is not None, None
    if a.live_s is not None:
        from mm_distillnet_amd.audio import resample_len
        n_frames, rate, chunks = open_live(a.input, a.live_s, a.sample_rate)
        win_len, hop, n_win = stream_sizes(a.window_s, a.hop_s, resample_len(n_frames, rate, SAMPLE_RATE))
    elif a.chunk_s is not None:
        n_total, chunks = open_chunked(a.input, int(round(a.chunk_s * SAMPLE_RATE)))
        win_len, hop, n_win = stream_sizes(a.window_s, a.hop_s, n_total)
    elif resampled:                           # the waveforms are made on the device: it is needed before the sizes are known
        torch.cuda.set_device(0)
        waves = load_resampled(a, dev)
    else:
        waves = read_input(a.input)
    if a.window_s is not None and not chunked:
        if waves.shape[0] != 1:
            raise ValueError(f"{a.input}: --window_s takes ONE recording (a .wav, or a .npy of shape [{CHANNELS}, N]), "
                             f"found {waves.shape[0]} clips of shape {tuple(waves.shape)}")
        win_len, hop, n_win = stream_sizes(a.window_s, a.hop_s, waves.shape[2])
    torch.cuda.set_device(0)
    sspec, _ = T.load_student_state(int(cfg.get("compound_coef", 2)))
    c = torch.load(a.checkpoint, map_location="cpu", weights_only=False)
    det = AudioDetector.from_step_config(sspec, dev, T.step_config(cfg))
    det.load(c["state_dict"] if "state_dict" in c else c)
    if chunked:
        streamed = run_chunked(det, chunks, win_len, hop, a.batch, track, rate)
    elif not resampled:
        waves = torch.from_numpy(waves).to(dev)
    if track is not None:
        rows, window, ids = streamed if chunked else det.track_stream(waves[0], win_len, hop, batch=a.batch, track=track)
        n = write_track_csv(a.output, rows, window, ids, hop)
        print("%d windows, %d boxes, %d tracks -> %s" % (n_win, n, len(np.unique(ids[ids >= 0])), a.output))
        return rows, window, ids
    if a.window_s is not None:
        rows, window = streamed if chunked else det.detect_stream(waves[0], win_len, hop, batch=a.batch)
        n = write_stream_csv(a.output, rows, window, hop)
        print("%d windows, %d boxes -> %s" % (n_win, n, a.output))
        return rows, window
    rows = det.detect(waves)
    det.check_overflow()
    n = write_csv(a.output, rows)
    print("%d clips, %d boxes -> %s" % (len(rows), n, a.output))
    return rows


if __name__ == "__main__":
    main()
