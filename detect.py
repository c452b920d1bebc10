#!/usr/bin/env python3
"""Audio-only detection with the trained student: a checkpoint plus microphone waveforms in, boxes out.

    python detect.py --config_file F --checkpoint P --input X --output out.csv [--overwrite JSON]
                     [--window_s SECONDS [--hop_s SECONDS] [--batch N]
                      [--track [--track_iou X] [--track_beta X] [--track_max_age N] [--track_max N]
                               [--track_assign greedy|optimal]]]
                     [--resample | --sample_rate R] [--chunk_s SECONDS | --live_s SECONDS] [--ema]
    python detect.py --config_file F --checkpoint P --input X0 --input X1 [--input X2 ...] --output out.csv
                     --window_s SECONDS --chunk_s SECONDS [--any_rate] [--hop_s SECONDS] [--batch N] [--track ...]

X is a `.npy` holding float32 waveforms `[8, N]` (one clip) or `[B, 8, N]`, or an 8-channel 16-bit PCM `.wav` at 44.1 kHz (one clip;
samples / 32768).  The waveforms go through the device front end (mel spectrogram, power_to_db per microphone, cubic resize to
image_size: what mp3_to_pkl.py:31-41, `MultimodalDetection.__getitem__` and `Resizer` make of a recording upstream), the student's
eval-mode forward and the post-processing of the reference's evaluation (score > conf_threshold, class filter, NMS).  The detection
settings (image_size, conf_threshold, nms_threshold, valid_labels, precision, compound_coef) are read from the cfg file like train.py
and evaluate.py read them.  No teacher is built or loaded.  With --ema the student gets the checkpoint's averaged weights
(`state_dict_ema`, written by a training run with cfg ema_decay) instead of its raw ones; a checkpoint without them is refused.  Output: one CSV row per box, columns
clip,x1,y1,x2,y2,score,label.

With --window_s the input is ONE recording (a `.wav`, or a `.npy` of shape [8, N]) and the detector slides over it on the device
(`AudioDetector.detect_stream`): windows of round(window_s * 44100) samples every round(hop_s * 44100) samples (hop_s defaults to
window_s), --batch windows per launch sequence; a tail shorter than a window is dropped.  The CSV then has the columns
window,t_start_s,x1,y1,x2,y2,score,label with t_start_s = window * hop / 44100.

With --track (only with --window_s) the boxes of consecutive windows are linked into tracks on the device
(`AudioDetector.track_stream`: greedy IoU association with a constant-velocity model) and the CSV gains a last column `track`: the id of
the row's track - ids start at 0 and rise in order of birth - or -1.  --track_iou: smallest IoU of a pairing (0.3); --track_beta: velocity
gain (0.5); --track_max_age: windows a track survives without a box (2); --track_max: live tracks at a time (64, at most 256).
--track_assign: how tracks and boxes are paired in a window - greedy (the default: the largest IoU first) or optimal (the matching of
maximum IoU sum: two vehicles that pass each other keep their ids where the greedy step would leave one of them without a box).

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

The files are read by `mm_distillnet_amd.recording`: `read_input` and `read_recording` a whole file, `open_chunks` a chunk at a time.
"""
import argparse
import csv
import os
import sys

import numpy as np

if os.environ.get("MMD_HW_QUEUES"):       # as train.py / evaluate.py: must be set before the HIP runtime starts
    os.environ.setdefault("GPU_MAX_HW_QUEUES", os.environ["MMD_HW_QUEUES"])
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import train as T  # noqa: E402
from mm_distillnet_amd.detector import AudioDetector  # noqa: E402
from mm_distillnet_amd.recording import CHANNELS, SAMPLE_RATE, open_chunks, read_input, read_npy, read_recording  # noqa: E402

DEVICE = "cuda:0"
COLUMNS = ("clip", "x1", "y1", "x2", "y2", "score", "label")
STREAM_COLUMNS = ("window", "t_start_s", "x1", "y1", "x2", "y2", "score", "label")
BANK_COLUMNS = ("session",) + STREAM_COLUMNS
INPUT_44K = "a .npy of float32 waveforms or an 8-channel 16-bit PCM .wav at 44.1 kHz"
LIVE_FEED = "feeds a live session that slides a window over the recording"


# ---------------------------------------------------------------------------------------------- flags
def check_flags(a):
    """Every refusal that the flags alone decide, before a file is opened or the device touched.  Where several apply, the first one
    below wins."""
    several = len(a.inputs) > 1

    def ext(path):
        return os.path.splitext(path)[1].lower()

    def needs_window(flag, why):
        if a.window_s is None:
            raise ValueError(f"{flag} {why}: it needs --window_s")

    def not_with_rates(who, why, live_too=True):
        if a.resample or a.sample_rate is not None or (live_too and a.live_s is not None):
            raise ValueError(f"{who} not go with --resample / --sample_rate{' / --live_s' if live_too else ''}: {why}")

    def positive_seconds(flag, seconds, rate, unit):
        """rate: Hz, at which `seconds` must hold one sample at least; None: only the sign is known yet"""
        if not seconds > 0 or (rate is not None and int(round(seconds * rate)) < 1):
            raise ValueError(f"{flag} {seconds}: a positive number of seconds (at least one {unit})")

    def supported(path, what):
        if ext(path) not in (".npy", ".wav"):
            raise ValueError(f"{path}: unsupported input ({what})")

    if a.any_rate and not several:
        raise ValueError("--any_rate is for several --input, each session at its file's rate (one recording of any rate: --live_s)")
    if several:
        if a.window_s is None or a.chunk_s is None:
            raise ValueError("several --input are read side by side into a bank of live sessions: they need --window_s and --chunk_s")
        if a.any_rate:
            not_with_rates("--any_rate does", "every .wav is read at the rate in its header")
        not_with_rates("several --input do", "the bank reads 44.1 kHz input only")
    elif a.chunk_s is not None:
        needs_window("--chunk_s", LIVE_FEED)
        not_with_rates("--chunk_s does", "it reads 44.1 kHz input only (--live_s reads a recording of any rate a chunk at a time and "
                       "resamples it as it arrives)", live_too=False)
    if a.chunk_s is not None:
        positive_seconds("--chunk_s", a.chunk_s, SAMPLE_RATE, "sample")
        for path in a.inputs:
            if a.any_rate and ext(path) != ".wav":
                raise ValueError(f"{path}: --any_rate reads 8-channel PCM .wav files, whose headers hold their rates (a .npy holds none)")
            supported(path, INPUT_44K)
    if several and a.batch is not None and a.batch < 1:
        raise ValueError(f"--batch {a.batch}")
    if a.live_s is not None:                  # one --input: several were refused above
        needs_window("--live_s", LIVE_FEED)
        if a.chunk_s is not None:
            raise ValueError("--live_s does not go with --chunk_s: one of the two says how the recording is cut into chunks")
        positive_seconds("--live_s", a.live_s, None, "frame")
        supported(a.input, "a .npy of float32 waveforms at --sample_rate, or an 8-channel PCM .wav of any rate")
        if ext(a.input) == ".wav" and a.sample_rate is not None:
            raise ValueError(f"{a.input}: a .wav holds its rate: --live_s reads it from the header (--sample_rate R is for a .npy)")
        if ext(a.input) == ".npy" and a.resample:
            raise ValueError(f"{a.input}: --resample reads a .wav; --live_s takes a .npy at --sample_rate R")
        rate = SAMPLE_RATE if a.sample_rate is None else a.sample_rate
        if rate < 1:
            raise ValueError(f"--sample_rate {a.sample_rate}: a positive number of Hz")
        if ext(a.input) == ".npy":
            positive_seconds("--live_s", a.live_s, rate, "frame")
    if a.track:
        needs_window("--track", "links the boxes of consecutive windows")


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
    ap.add_argument("--track_assign", type=str, default="greedy", help="pairing of tracks and boxes: greedy, or optimal (maximum IoU sum)")
    ap.add_argument("--resample", action="store_true", help="a .wav of any rate, 16/24/32-bit PCM: decode and resample to 44.1 kHz on the device")
    ap.add_argument("--sample_rate", type=int, default=None, help="the rate in Hz of a .npy input; resampled to 44.1 kHz on the device")
    ap.add_argument("--chunk_s", type=float, default=None, help="read the recording this many seconds at a time into a live session (with --window_s)")
    ap.add_argument("--any_rate", action="store_true", help="several .wav inputs, each at the rate in its header (with --window_s --chunk_s)")
    ap.add_argument("--live_s", type=float, default=None, help="read a recording of any rate this many seconds at a time into a live session that resamples (with --window_s)")
    ap.add_argument("--ema", action="store_true", help="load the checkpoint's averaged weights (state_dict_ema: cfg ema_decay), not its raw ones")
    a = ap.parse_args(argv)
    a.inputs, a.input = a.input, a.input[0]
    a.ema_state = None                    # main(): the averaged state dict, with --ema
    check_flags(a)
    if len(a.inputs) == 1 and a.batch is None:
        a.batch = 8
    return a


# ---------------------------------------------------------------------------------------------- output
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


def write_windows_csv(path: str, rows, window, hop: int, track=None, session=None) -> int:
    """One row per box: [its session,] its window, the window's start in seconds at a hop of `hop` samples, the box[, its track id].
    rows [R, 6] / window [R][ / track [R]] of `detect_stream` / `track_stream` or a `LiveSession`; with session [R], of a `LiveBank`."""
    rows, window = np.asarray(rows, np.float32).reshape(-1, 6), np.asarray(window).reshape(-1)

    def column(ids):
        return [[]] * len(rows) if ids is None else [[i] for i in np.asarray(ids).reshape(-1).tolist()]

    first, last = column(session), column(track)
    if (session is not None or track is not None) and not (len(first) == len(window) == len(last) == len(rows)):
        if session is None:               # (both texts name the writer this one replaced: they are what callers match)
            raise ValueError("write_track_csv: %d rows, %d windows, %d track ids" % (len(rows), len(window), len(last)))
        raise ValueError("write_bank_csv: %d rows, %d sessions, %d windows, %d track ids" % (len(rows), len(first), len(window), len(last)))
    with open(path, "w", newline="") as f:
        out = csv.writer(f)
        out.writerow((STREAM_COLUMNS if session is None else BANK_COLUMNS) + (("track",) if track is not None else ()))
        for q, w, r, t in zip(first, window.tolist(), rows, last):
            out.writerow(q + [w, "%.9g" % (w * hop / SAMPLE_RATE)] + ["%.9g" % float(v) for v in r] + t)
    return len(rows)


def report_windows(a, got, hop: int, n_win: int, track):
    """CSV and summary line of ONE recording's windows -> (rows, window[, track ids])"""
    ids = got[2] if track is not None else None
    n = write_windows_csv(a.output, got[0], got[1], hop, ids)
    tracks = "" if ids is None else ", %d tracks" % len(np.unique(ids[ids >= 0]))
    print("%d windows, %d boxes%s -> %s" % (n_win, n, tracks, a.output))
    return tuple(got)


# ---------------------------------------------------------------------------------------------- input and detector
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


def read_waves(a):
    """-> the waveforms [B, 8, N] at 44.1 kHz: a numpy array, or with --resample / --sample_rate a device tensor (they are made on the
    device: it is needed before the sizes are known)"""
    if a.resample or a.sample_rate is not None:
        torch.cuda.set_device(0)
        return load_resampled(a, DEVICE)
    return read_input(a.input)


def stream_sizes(window_s: float, hop_s, n_total: int):
    """-> (win_len, hop, number of windows) in samples; raises ValueError as `stream_window_starts` does"""
    from mm_distillnet_amd.audio import stream_window_starts
    win_len = int(round(window_s * SAMPLE_RATE))
    hop = win_len if hop_s is None else int(round(hop_s * SAMPLE_RATE))
    return win_len, hop, len(stream_window_starts(n_total, win_len, hop))


def load_detector(a, cfg) -> AudioDetector:
    """The student of the cfg file with the checkpoint's weights, on the device.  Every mode calls it behind its last host-side refusal."""
    torch.cuda.set_device(0)
    sspec, _ = T.load_student_state(int(cfg.get("compound_coef", 2)))
    state = getattr(a, "ema_state", None)      # --ema: read in main(), in front of every mode's first device work
    if state is None:
        state = T.TR.checkpoint_student_state(torch.load(a.checkpoint, map_location="cpu", weights_only=False), False, a.checkpoint)
    det = AudioDetector.from_step_config(sspec, DEVICE, T.step_config(cfg))
    det.load(state)
    return det


# ---------------------------------------------------------------------------------------------- the feed loop
def push_session(session, k: int, chunk, width):
    return session.push(chunk) if width is None else session.push_pcm(chunk, width)


def push_bank(bank, k: int, chunk, width):
    return bank.push(k, chunk) if width is None else bank.push_pcm(k, chunk, width)


def feed(target, sources: list, push=None):
    """sources: the chunk iterators of `open_chunks`, source k for session k of `target`, a `LiveSession` (one source) or a `LiveBank`.
    Walks them in round robin - one chunk of every source that still has one, in source order, again and again; exhausted sources drop
    out - then `flush` and `close` -> what the target returns for the whole recordings.  push(target, k, chunk, width) hands a chunk
    over as soon as it is read, before the next source is touched: one chunk in host memory.  push None: a round is collected and goes
    over as ONE `push_all_pcm`."""
    parts, live = [], list(enumerate(iter(src) for src in sources))
    while live:
        still, chunks, widths = [], {}, {}
        for k, it in live:
            got = next(it, None)
            if got is None:
                continue
            still.append((k, it))
            if push is not None:
                parts.append(push(target, k, *got))
            else:
                chunks[k], widths[k] = got
        if chunks:
            parts.append(target.push_all_pcm(chunks, widths))
        live = still
    parts.append(target.flush())
    target.close()
    return target.concat(parts)


# ---------------------------------------------------------------------------------------------- the modes
def run_clips(a, cfg, track):
    """every clip of the input on its own"""
    waves = read_waves(a)
    det = load_detector(a, cfg)
    rows = det.detect(torch.as_tensor(waves).to(DEVICE))
    det.check_overflow()
    n = write_csv(a.output, rows)
    print("%d clips, %d boxes -> %s" % (len(rows), n, a.output))
    return rows


def run_stream(a, cfg, track):
    """--window_s: ONE recording, whole on the device"""
    waves = read_waves(a)
    if waves.shape[0] != 1:
        raise ValueError(f"{a.input}: --window_s takes ONE recording (a .wav, or a .npy of shape [{CHANNELS}, N]), "
                         f"found {waves.shape[0]} clips of shape {tuple(waves.shape)}")
    win_len, hop, n_win = stream_sizes(a.window_s, a.hop_s, waves.shape[2])
    det = load_detector(a, cfg)
    rec = torch.as_tensor(waves).to(DEVICE)[0]
    got = det.detect_stream(rec, win_len, hop, batch=a.batch) if track is None else det.track_stream(rec, win_len, hop, batch=a.batch, track=track)
    return report_windows(a, got, hop, n_win, track)


def run_session(a, cfg, track, n_total: int, chunks, sample_rate):
    """one recording of n_total samples at 44.1 kHz, its chunks pushed at sample_rate into a live session"""
    win_len, hop, n_win = stream_sizes(a.window_s, a.hop_s, n_total)
    session = load_detector(a, cfg).open_stream(win_len, hop, batch=a.batch, track=track, sample_rate=sample_rate)
    return report_windows(a, feed(session, [chunks], push_session), hop, n_win, track)


def run_chunked(a, cfg, track):
    """--chunk_s: a 44.1 kHz recording, a chunk at a time"""
    n_total, _, chunks = open_chunks(a.input, a.chunk_s, any_rate=False)
    return run_session(a, cfg, track, n_total, chunks, None)


def run_live(a, cfg, track):
    """--live_s: a recording of any rate, a chunk at a time into a session that resamples"""
    from mm_distillnet_amd.audio import resample_len
    n_frames, rate, chunks = open_chunks(a.input, a.live_s, True, a.sample_rate)
    return run_session(a, cfg, track, resample_len(n_frames, rate, SAMPLE_RATE), chunks, rate)


def run_sessions(a, cfg, track, n_totals: list, sources: list, rates, push):
    """several recordings of n_totals[k] samples at 44.1 kHz, their chunks pushed at rates[k] into one bank"""
    sizes = [stream_sizes(a.window_s, a.hop_s, n_total) for n_total in n_totals]
    win_len, hop, n_win = sizes[0][0], sizes[0][1], sum(z[2] for z in sizes)
    det = load_detector(a, cfg)
    bank = det.open_bank(len(sources), win_len, hop, batch=len(a.inputs) if a.batch is None else a.batch, track=track, sample_rates=rates)
    got = feed(bank, sources, push)
    n = write_windows_csv(a.output, got[0], got[2], hop, got[3] if track is not None else None, got[1])
    print("%d sessions, %d windows, %d boxes -> %s" % (len(a.inputs), n_win, n, a.output))
    return got


def run_bank(a, cfg, track):
    """several --input at 44.1 kHz: every chunk is pushed as it is read"""
    opened = [open_chunks(path, a.chunk_s, any_rate=False) for path in a.inputs]
    return run_sessions(a, cfg, track, [n for n, _, _ in opened], [chunks for _, _, chunks in opened], None, push_bank)


def run_bank_any_rate(a, cfg, track):
    """--any_rate: every file at its own rate, one `push_all_pcm` per round"""
    from mm_distillnet_amd.audio import resample_len, resample_ratio
    opened = [open_chunks(path, a.chunk_s, any_rate=True) for path in a.inputs]
    rates = [rate for _, rate, _ in opened]
    for rate in rates:
        resample_ratio(rate)                  # an unsupported ratio is refused before any device work
    return run_sessions(a, cfg, track, [resample_len(n, rate, SAMPLE_RATE) for n, rate, _ in opened], [chunks for _, _, chunks in opened], rates, None)


def main(argv=None):
    a = parse_args(argv)
    track = None
    if a.track:
        from mm_distillnet_amd.tracker import TrackConfig
        track = TrackConfig(iou_min=a.track_iou, beta=a.track_beta, max_age=a.track_max_age, max_tracks=a.track_max,
                            assign=a.track_assign)
    cfg, _ = T.parse_config(["--config_file", a.config_file] + (["--overwrite", a.overwrite] if a.overwrite else []))
    if a.ema:
        # a checkpoint without averaged weights is refused here, on the host: some modes touch the device before they load the detector
        a.ema_state = T.TR.checkpoint_student_state(torch.load(a.checkpoint, map_location="cpu", weights_only=False), True, a.checkpoint)
    if len(a.inputs) > 1:
        mode = run_bank_any_rate if a.any_rate else run_bank
    elif a.live_s is not None:
        mode = run_live
    elif a.chunk_s is not None:
        mode = run_chunked
    elif a.window_s is not None:
        mode = run_stream
    else:
        mode = run_clips
    return mode(a, cfg, track)


if __name__ == "__main__":
    main()
