"""detect.py's flags: which command lines `parse_args` refuses, with which words, and which refusal wins where several apply.  The
table is literal: its strings were printed by the tool before its flag checks became one function, one row per refusal and one per pair
of refusals that a command line can earn together and tell apart (where a third one always wins, no row can).  No config file,
checkpoint or input file is read: the flags alone decide."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["--config_file", "c.cfg", "--checkpoint", "p.pth", "--output", "o.csv"]

ANY_RATE_ONE = "--any_rate is for several --input, each session at its file's rate (one recording of any rate: --live_s)"
ANY_RATE_RATES = "--any_rate does not go with --resample / --sample_rate / --live_s: every .wav is read at the rate in its header"
ANY_RATE_WAV = "{}: --any_rate reads 8-channel PCM .wav files, whose headers hold their rates (a .npy holds none)"
BANK_NEEDS = "several --input are read side by side into a bank of live sessions: they need --window_s and --chunk_s"
BANK_RATES = "several --input do not go with --resample / --sample_rate / --live_s: the bank reads 44.1 kHz input only"
BATCH = "--batch {}"
CHUNK_POSITIVE = "--chunk_s {}: a positive number of seconds (at least one sample)"
CHUNK_RATES = ("--chunk_s does not go with --resample / --sample_rate: it reads 44.1 kHz input only "
               "(--live_s reads a recording of any rate a chunk at a time and resamples it as it arrives)")
CHUNK_WINDOW = "--chunk_s feeds a live session that slides a window over the recording: it needs --window_s"
LIVE_CHUNK = "--live_s does not go with --chunk_s: one of the two says how the recording is cut into chunks"
LIVE_NPY_RESAMPLE = "{}: --resample reads a .wav; --live_s takes a .npy at --sample_rate R"
LIVE_POSITIVE = "--live_s {}: a positive number of seconds (at least one frame)"
LIVE_UNSUPPORTED = "{}: unsupported input (a .npy of float32 waveforms at --sample_rate, or an 8-channel PCM .wav of any rate)"
LIVE_WAV_RATE = "{}: a .wav holds its rate: --live_s reads it from the header (--sample_rate R is for a .npy)"
LIVE_WINDOW = "--live_s feeds a live session that slides a window over the recording: it needs --window_s"
RATE_POSITIVE = "--sample_rate {}: a positive number of Hz"
TRACK_WINDOW = "--track links the boxes of consecutive windows: it needs --window_s"
UNSUPPORTED = "{}: unsupported input (a .npy of float32 waveforms or an 8-channel 16-bit PCM .wav at 44.1 kHz)"

# (the command line behind BASE: the leading words are the --input files; the message, or None where the flags are accepted)
TABLE = [
    # ---- accepted: clips, stream, tracking, resampled, chunked, live, bank, any-rate bank
    ("a.wav", None),
    ("a.txt", None),                                                        # the extension is the reader's to refuse
    ("a.npy --window_s 1.0 --batch 0", None),                               # one input: --batch is the library's to refuse
    ("a.wav --window_s 1.0 --track", None),
    ("a.npy --resample", None),                                             # --resample / --sample_rate mix-ups: refused behind the flags
    ("a.wav --window_s 1.0 --sample_rate 0", None),
    ("a.wav --window_s 1.0 --chunk_s 0.5 --track", None),
    ("a.wav --window_s 1.0 --live_s 0.5 --resample", None),
    ("a.wav --window_s 1.0 --live_s 1e-9", None),                           # a .wav's rate is in its header: the chunk is sized there
    ("a.npy --window_s 1.0 --live_s 0.5 --sample_rate 48000 --track", None),
    ("a.wav b.npy --window_s 1.0 --chunk_s 0.5", None),
    ("a.wav b.wav c.wav --window_s 1.0 --chunk_s 0.5 --batch 4 --any_rate --track", None),
    # ---- every refusal on its own
    ("a.wav --any_rate", ANY_RATE_ONE),
    ("a.wav b.wav --window_s 1.0 --chunk_s 0.5 --resample --any_rate", ANY_RATE_RATES),      # (never alone: the bank's own applies too)
    ("a.wav b.wav --window_s 1.0 --chunk_s 0.5 --sample_rate 48000 --any_rate", ANY_RATE_RATES),
    ("a.wav b.wav --window_s 1.0 --chunk_s 0.5 --live_s 0.5 --any_rate", ANY_RATE_RATES),
    ("a.wav b.npy --window_s 1.0 --chunk_s 0.5 --any_rate", ANY_RATE_WAV.format("b.npy")),
    ("a.wav b.wav", BANK_NEEDS),
    ("a.wav b.wav --window_s 1.0", BANK_NEEDS),
    ("a.wav b.wav --chunk_s 0.5", BANK_NEEDS),
    ("a.wav b.wav --window_s 1.0 --chunk_s 0.5 --resample", BANK_RATES),
    ("a.wav b.wav --window_s 1.0 --chunk_s 0.5 --sample_rate 48000", BANK_RATES),
    ("a.wav b.wav --window_s 1.0 --chunk_s 0.5 --live_s 0.5", BANK_RATES),
    ("a.wav b.wav --window_s 1.0 --chunk_s 0.5 --batch 0", BATCH.format("0")),
    ("a.wav b.wav --window_s 1.0 --chunk_s 0.5 --batch -1", BATCH.format("-1")),
    ("a.wav --window_s 1.0 --chunk_s 0.0", CHUNK_POSITIVE.format("0.0")),
    ("a.wav --window_s 1.0 --chunk_s -1", CHUNK_POSITIVE.format("-1.0")),
    ("a.wav --window_s 1.0 --chunk_s 1e-9", CHUNK_POSITIVE.format("1e-09")),                 # round(1e-9 * 44100) = 0 samples
    ("a.wav --window_s 1.0 --chunk_s nan", CHUNK_POSITIVE.format("nan")),
    ("a.wav b.wav --window_s 1.0 --chunk_s 0.0", CHUNK_POSITIVE.format("0.0")),
    ("a.wav --window_s 1.0 --chunk_s 0.5 --resample", CHUNK_RATES),
    ("a.npy --window_s 1.0 --chunk_s 0.5 --sample_rate 48000", CHUNK_RATES),
    ("a.wav --chunk_s 0.5", CHUNK_WINDOW),
    ("a.wav --window_s 1.0 --chunk_s 0.5 --live_s 0.5", LIVE_CHUNK),
    ("a.npy --window_s 1.0 --live_s 0.5 --resample", LIVE_NPY_RESAMPLE.format("a.npy")),
    ("a.wav --window_s 1.0 --live_s 0.0", LIVE_POSITIVE.format("0.0")),
    ("a.npy --window_s 1.0 --live_s 1e-9", LIVE_POSITIVE.format("1e-09")),                   # round(1e-9 * 44100) = 0 frames of a .npy
    ("a.npy --window_s 1.0 --live_s 1e-5 --sample_rate 48000", LIVE_POSITIVE.format("1e-05")),    # round(0.48) = 0 frames at --sample_rate
    ("a.txt --window_s 1.0 --live_s 0.5", LIVE_UNSUPPORTED.format("a.txt")),
    ("a.wav --window_s 1.0 --live_s 0.5 --sample_rate 48000", LIVE_WAV_RATE.format("a.wav")),
    ("a.wav --live_s 0.5", LIVE_WINDOW),
    ("a.npy --window_s 1.0 --live_s 0.5 --sample_rate 0", RATE_POSITIVE.format("0")),
    ("a.wav --track", TRACK_WINDOW),
    ("a.txt --window_s 1.0 --chunk_s 0.5", UNSUPPORTED.format("a.txt")),
    ("A.WAV b.NPY c.mp3 --window_s 1.0 --chunk_s 0.5", UNSUPPORTED.format("c.mp3")),
    # ---- two or more apply: which one wins.  One input:
    ("a.wav --window_s 1.0 --chunk_s 0.0 --any_rate", ANY_RATE_ONE),
    ("a.wav --window_s 1.0 --chunk_s 0.5 --resample --any_rate", ANY_RATE_ONE),
    ("a.wav --chunk_s 0.5 --any_rate", ANY_RATE_ONE),
    ("a.wav --window_s 1.0 --chunk_s 0.5 --live_s 0.5 --any_rate", ANY_RATE_ONE),
    ("a.npy --window_s 1.0 --live_s 0.5 --resample --any_rate", ANY_RATE_ONE),
    ("a.wav --window_s 1.0 --live_s 0.0 --any_rate", ANY_RATE_ONE),
    ("a.txt --window_s 1.0 --live_s 0.5 --any_rate", ANY_RATE_ONE),
    ("a.wav --window_s 1.0 --live_s 0.5 --sample_rate 48000 --any_rate", ANY_RATE_ONE),
    ("a.wav --live_s 0.5 --any_rate", ANY_RATE_ONE),
    ("a.npy --window_s 1.0 --live_s 0.5 --sample_rate 0 --any_rate", ANY_RATE_ONE),
    ("a.wav --any_rate --track", ANY_RATE_ONE),
    ("a.txt --window_s 1.0 --chunk_s 0.5 --any_rate", ANY_RATE_ONE),
    ("a.wav --window_s 1.0 --chunk_s 0.0 --resample", CHUNK_RATES),
    ("a.wav --chunk_s 0.0", CHUNK_WINDOW),
    ("a.wav --window_s 1.0 --chunk_s 0.0 --live_s 0.5", CHUNK_POSITIVE.format("0.0")),
    ("a.wav --window_s 1.0 --chunk_s 0.0 --live_s 0.0", CHUNK_POSITIVE.format("0.0")),
    ("a.txt --window_s 1.0 --chunk_s 0.0 --live_s 0.5", CHUNK_POSITIVE.format("0.0")),
    ("a.txt --window_s 1.0 --chunk_s 0.0", CHUNK_POSITIVE.format("0.0")),
    ("a.wav --chunk_s 0.5 --resample", CHUNK_WINDOW),
    ("a.wav --window_s 1.0 --chunk_s 0.5 --live_s 0.5 --resample", CHUNK_RATES),
    ("a.npy --window_s 1.0 --chunk_s 0.5 --live_s 0.5 --resample", CHUNK_RATES),
    ("a.wav --window_s 1.0 --chunk_s 0.5 --live_s 0.0 --resample", CHUNK_RATES),
    ("a.txt --window_s 1.0 --chunk_s 0.5 --live_s 0.5 --resample", CHUNK_RATES),
    ("a.wav --window_s 1.0 --chunk_s 0.5 --live_s 0.5 --sample_rate 48000", CHUNK_RATES),
    ("a.npy --window_s 1.0 --chunk_s 0.5 --live_s 0.5 --sample_rate 0", CHUNK_RATES),
    ("a.txt --window_s 1.0 --chunk_s 0.5 --resample", CHUNK_RATES),
    ("a.wav --chunk_s 0.5 --live_s 0.5", CHUNK_WINDOW),
    ("a.npy --chunk_s 0.5 --live_s 0.5 --resample", CHUNK_WINDOW),
    ("a.wav --chunk_s 0.5 --live_s 0.0", CHUNK_WINDOW),
    ("a.txt --chunk_s 0.5 --live_s 0.5", CHUNK_WINDOW),
    ("a.wav --chunk_s 0.5 --live_s 0.5 --sample_rate 48000", CHUNK_WINDOW),
    ("a.npy --chunk_s 0.5 --live_s 0.5 --sample_rate 0", CHUNK_WINDOW),
    ("a.wav --chunk_s 0.5 --track", CHUNK_WINDOW),
    ("a.txt --chunk_s 0.5", CHUNK_WINDOW),
    ("a.wav --window_s 1.0 --chunk_s 0.5 --live_s 0.0", LIVE_CHUNK),
    ("a.txt --window_s 1.0 --chunk_s 0.5 --live_s 0.5", UNSUPPORTED.format("a.txt")),        # --chunk_s's wording, not --live_s's
    ("a.txt --window_s 1.0 --chunk_s 0.5 --live_s 0.0", UNSUPPORTED.format("a.txt")),
    ("a.npy --window_s 1.0 --live_s 0.0 --resample", LIVE_POSITIVE.format("0.0")),
    ("a.npy --live_s 0.5 --resample", LIVE_WINDOW),
    ("a.npy --window_s 1.0 --live_s 0.5 --sample_rate 0 --resample", LIVE_NPY_RESAMPLE.format("a.npy")),
    ("a.txt --window_s 1.0 --live_s 0.0", LIVE_POSITIVE.format("0.0")),
    ("a.wav --window_s 1.0 --live_s 0.0 --sample_rate 48000", LIVE_POSITIVE.format("0.0")),
    ("a.wav --live_s 0.0", LIVE_WINDOW),
    ("a.npy --window_s 1.0 --live_s 0.0 --sample_rate 0", LIVE_POSITIVE.format("0.0")),
    ("a.txt --live_s 0.5", LIVE_WINDOW),
    ("a.txt --window_s 1.0 --live_s 0.5 --sample_rate 0", LIVE_UNSUPPORTED.format("a.txt")),
    ("a.wav --live_s 0.5 --sample_rate 48000", LIVE_WINDOW),
    ("a.wav --window_s 1.0 --live_s 0.5 --sample_rate 0", LIVE_WAV_RATE.format("a.wav")),
    ("a.npy --live_s 0.5 --sample_rate 0", LIVE_WINDOW),
    ("a.wav --live_s 0.5 --track", LIVE_WINDOW),
    # (a chunk below one frame of a .npy is the LAST of --live_s's refusals, its sign one of the first)
    ("a.npy --window_s 1.0 --live_s 1e-9 --resample", LIVE_NPY_RESAMPLE.format("a.npy")),
    ("a.npy --window_s 1.0 --live_s 1e-9 --sample_rate 0", RATE_POSITIVE.format("0")),
    ("a.txt --window_s 1.0 --live_s 1e-9", LIVE_UNSUPPORTED.format("a.txt")),
    # several inputs:
    ("a.wav b.npy --window_s 1.0 --chunk_s 0.5 --resample --any_rate", ANY_RATE_RATES),
    ("a.wav b.wav --resample --any_rate", BANK_NEEDS),
    ("a.wav b.wav --window_s 1.0 --chunk_s 0.5 --batch 0 --resample --any_rate", ANY_RATE_RATES),
    ("a.wav b.wav --window_s 1.0 --chunk_s 0.0 --resample --any_rate", ANY_RATE_RATES),
    ("a.wav b.txt --window_s 1.0 --chunk_s 0.5 --resample --any_rate", ANY_RATE_RATES),
    ("a.wav b.npy --any_rate", BANK_NEEDS),
    ("a.wav b.npy --window_s 1.0 --chunk_s 0.5 --batch 0 --any_rate", ANY_RATE_WAV.format("b.npy")),
    ("a.wav b.npy --window_s 1.0 --chunk_s 0.0 --any_rate", CHUNK_POSITIVE.format("0.0")),
    ("a.wav b.txt --window_s 1.0 --chunk_s 0.5 --any_rate", ANY_RATE_WAV.format("b.txt")),
    ("a.npy b.txt --window_s 1.0 --chunk_s 0.5 --any_rate", ANY_RATE_WAV.format("a.npy")),   # the first file that offends
    ("a.txt b.mp3 --window_s 1.0 --chunk_s 0.5", UNSUPPORTED.format("a.txt")),
    ("a.wav b.wav --resample", BANK_NEEDS),
    ("a.wav b.wav --window_s 1.0 --live_s 0.5", BANK_NEEDS),
    ("a.wav b.wav --batch 0", BANK_NEEDS),
    ("a.wav b.wav --track", BANK_NEEDS),
    ("a.wav b.wav --window_s 1.0 --chunk_s 0.5 --batch 0 --resample", BANK_RATES),
    ("a.wav b.wav --window_s 1.0 --chunk_s 0.0 --resample", BANK_RATES),
    ("a.wav b.txt --window_s 1.0 --chunk_s 0.5 --resample", BANK_RATES),
    ("a.wav b.wav --window_s 1.0 --chunk_s 0.0 --batch 0", CHUNK_POSITIVE.format("0.0")),
    ("a.wav b.txt --window_s 1.0 --chunk_s 0.5 --batch 0", UNSUPPORTED.format("b.txt")),
]


def _detect():
    sys.path.insert(0, ROOT)
    import detect
    return detect


def _split(line: str):
    """-> (the --input files, the flags behind them)"""
    words = line.split()
    n = next((i for i, w in enumerate(words) if w.startswith("--")), len(words))
    return words[:n], words[n:]


def _argv(line: str) -> list:
    inputs, flags = _split(line)
    return BASE + [x for p in inputs for x in ("--input", p)] + flags


def test_the_table_names_every_command_line_once():
    assert len({line for line, _ in TABLE}) == len(TABLE)
    assert _argv("a.wav b.npy --window_s 1.0 --track") == BASE + ["--input", "a.wav", "--input", "b.npy", "--window_s", "1.0", "--track"]


@pytest.mark.parametrize("line,message", TABLE, ids=[line for line, _ in TABLE])
def test_parse_args_refuses_with_the_same_words(line, message):
    det = _detect()
    if message is None:
        a = det.parse_args(_argv(line))
        assert a.inputs == _split(line)[0] and a.input == a.inputs[0]
    else:
        with pytest.raises(ValueError) as e:
            det.parse_args(_argv(line))
        assert str(e.value) == message
