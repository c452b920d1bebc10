"""Streaming detection, CPU side: the window arithmetic (`audio.stream_window_starts`), detect.py's --window_s checks and its two CSV
writers, and the C ABI of mmd_melspec_windows / mmd_det_record_append without a GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mmd_melspec_windows", "mmd_det_record_append")


def _detect():
    sys.path.insert(0, ROOT)
    import detect
    return detect


# ---------------------------------------------------------------------------------------------- window arithmetic
def test_window_starts():
    from mm_distillnet_amd.audio import stream_window_starts as starts
    assert starts(4096, 4096, 100) == [0]                                  # n_total = win_len: one window
    assert starts(4096 + 3 * 1531, 4096, 1531) == [0, 1531, 3062, 4593]    # exact fit at the end keeps the last window
    assert starts(4096 + 3 * 1531 - 1, 4096, 1531) == [0, 1531, 3062]      # one sample short drops it
    assert starts(20000, 4096, 5000) == [0, 5000, 10000, 15000]            # a hop larger than the window
    assert starts(20000, 4096, 15904) == [0, 15904] and starts(20000, 4096, 15905) == [0]
    assert starts(1000, 513, 1) == list(range(488))                        # the shortest legal window, hop 1
    for s in starts(16000, 4096, 1531):
        assert 0 <= s <= 16000 - 4096


def test_window_starts_refuses_bad_arguments():
    from mm_distillnet_amd.audio import stream_window_starts as starts
    for hop in (0, -5):
        with pytest.raises(ValueError, match="hop"):
            starts(16000, 4096, hop)
    for win in (512, 0, -1):
        with pytest.raises(ValueError, match="too short for the reflect padding"):
            starts(16000, win, 100)
    with pytest.raises(ValueError, match="shorter than one window"):
        starts(4095, 4096, 100)


# ---------------------------------------------------------------------------------------------- control table
def test_control_table_lays_out_starts_padding_and_the_two_int32_halves():
    """One control row per group, as csrc/stream.hip and the front end read it: int64 starts[batch], a short group padded with its last
    real window, then n_valid in the low and first_window in the high int32 of the last (little-endian) word.  No device."""
    from mm_distillnet_amd.detector import _GroupChain
    cases = ((3, [([0, 1531, 3062], 0), ([4593, 6124, 7655], 3), ([9186, 10717], 6)]),          # two full groups, a short last one
             (4, [([7, 2 ** 40 + 5], 2 ** 31 - 3)]),                                           # a start past 2^32, a large window index
             (1, [([0], 0), ([1531], 1), ([3062], 2)]))                                        # batch = 1: never padded
    for batch, groups in cases:
        table = _GroupChain.control_table(groups, batch)
        assert table.dtype == np.int64 and table.shape == (len(groups), batch + 1) and table.flags.c_contiguous
        for row, (real, first) in zip(table, groups):
            assert row[:batch].tolist() == real + [real[-1]] * (batch - len(real))
            assert row[batch:].view("<i4").tolist() == [len(real), first]
            assert int(row[batch]) == len(real) + (first << 32)
        # into a provided table (a session's pinned one, longer than needed and dirty): the same bytes, the other rows untouched
        given = np.full((len(groups) + 2, batch + 1), -1, np.int64)
        got = _GroupChain.control_table(groups, batch, given)
        assert got.tobytes() == table.tobytes() and np.shares_memory(got, given)
        assert np.array_equal(given[:len(groups)], table) and (given[len(groups):] == -1).all()


# ---------------------------------------------------------------------------------------------- detect.py
def test_window_option_refuses_a_stack_of_clips_before_any_gpu_call(tmp_path, monkeypatch):
    det = _detect()
    import torch

    def refuse(*a, **k):
        raise AssertionError("the GPU was reached")

    monkeypatch.setattr(torch.cuda, "set_device", refuse)
    monkeypatch.setattr(torch, "load", refuse)
    np.save(tmp_path / "two.npy", np.zeros((2, 8, 9000), np.float32))
    cfgf = os.path.join(ROOT, "configs", "mm-distillnet.cfg")
    argv = ["--config_file", cfgf, "--checkpoint", str(tmp_path / "none.pth"), "--input", str(tmp_path / "two.npy"),
            "--output", str(tmp_path / "o.csv"), "--window_s", "0.1"]
    with pytest.raises(ValueError, match="ONE recording"):
        det.main(argv)
    assert not os.path.exists(tmp_path / "o.csv")
    # one recording, but shorter than a window: refused by the shared arithmetic, again before the GPU
    np.save(tmp_path / "one.npy", np.zeros((8, 4000), np.float32))
    argv[5] = str(tmp_path / "one.npy")
    with pytest.raises(ValueError, match="shorter than one window"):
        det.main(argv)


def test_stream_sizes_round_seconds_to_samples():
    det = _detect()
    assert det.stream_sizes(1.0, None, 44100 * 3) == (44100, 44100, 3)
    assert det.stream_sizes(1.0, 0.1, 44100 * 60) == (44100, 4410, 591)
    assert det.stream_sizes(0.05, 0.0333, 8000) == (2205, 1469, 4)        # 1468.53 rounds up: no multiple of 256 or 4


def test_stream_csv_writer(tmp_path):
    det = _detect()
    rows = np.array([[1, 2, 30, 40, 0.1 + 0.2, 6], [0, 0, 128, 127, np.float32(1) / 3, 6], [5, 6, 7, 8, 0.999999, 14]], np.float32)
    window = np.array([0, 0, 7], np.int32)
    assert det.write_windows_csv(str(tmp_path / "s.csv"), rows, window, 1531) == 3
    lines = open(tmp_path / "s.csv").read().strip().split("\n")
    assert lines[0] == "window,t_start_s,x1,y1,x2,y2,score,label" and len(lines) == 4
    assert [ln.split(",")[0] for ln in lines[1:]] == ["0", "0", "7"]
    assert [ln.split(",")[1] for ln in lines[1:]] == ["0", "0", "%.9g" % (7 * 1531 / 44100)] and lines[3].split(",")[1] == "0.243015873"
    got = np.array([[float(v) for v in ln.split(",")[2:]] for ln in lines[1:]])
    assert np.array_equal(got.astype(np.float32), rows)
    # no boxes: the header alone
    assert det.write_windows_csv(str(tmp_path / "e.csv"), np.zeros((0, 6), np.float32), np.zeros(0, np.int32), 100) == 0
    assert open(tmp_path / "e.csv", "rb").read() == b"window,t_start_s,x1,y1,x2,y2,score,label\r\n"


def test_clip_csv_writer_is_unchanged(tmp_path):
    det = _detect()
    rows = [np.array([[1, 2, 30, 40, 0.1 + 0.2, 6], [0, 0, 128, 127, np.float32(1) / 3, 6]], np.float32), np.zeros((0, 6), np.float32),
            np.array([[5, 6, 7, 8, 0.999999, 14]], np.float32)]
    assert det.write_csv(str(tmp_path / "o.csv"), rows) == 3
    assert open(tmp_path / "o.csv", "rb").read() == (b"clip,x1,y1,x2,y2,score,label\r\n"
                                                     b"0,1,2,30,40,0.300000012,6\r\n"
                                                     b"0,0,0,128,127,0.333333343,6\r\n"
                                                     b"2,5,6,7,8,0.999998987,14\r\n")
    assert det.COLUMNS == ("clip", "x1", "y1", "x2", "y2", "score", "label")


# ---------------------------------------------------------------------------------------------- C ABI without a GPU
def test_header_declares_and_library_exports_the_entry_points():
    import __graft_entry__ as ge
    ge.build()
    from mm_distillnet_amd import _lib
    sigs = _lib.LIB.symbols()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in sigs and hasattr(dll, name), name
    assert len(sigs["mmd_melspec_windows"]) == 14 and len(sigs["mmd_det_record_append"]) == 11
    text = open(_lib.HEADER).read()
    head = text[:text.index("int mmd_melspec_windows(")]
    comment = head[head.rindex("\n\n"):].replace("\n// ", " ")
    assert "CALLER'S ERROR" in comment and "bit for bit" in comment and "need no zeroing" in comment


def test_bad_arguments_are_rejected_without_gpu():
    import __graft_entry__ as ge
    ge.build()
    from mm_distillnet_amd import _lib
    dll = _lib.LIB.load()
    p = ctypes.c_void_p(4096)            # never dereferenced: validation precedes any launch
    mw = dll.mmd_melspec_windows
    assert mw(None, 8, 16000, None, 4, 512, None, None, None, 50, 1, None, None, None) == -22     # win_len too short for the padding
    assert mw(None, 8, 16000, None, 0, 4096, None, None, None, 50, 1, None, None, None) == -22    # B = 0
    assert mw(None, 8, 16000, None, 4, 16001, None, None, None, 50, 1, None, None, None) == -22   # win_len > n_total
    # the same three with every pointer given: it is the size that is refused
    assert mw(p, 8, 16000, p, 4, 512, p, p, p, 50, 1, p, p, None) == -22
    assert mw(p, 8, 16000, p, 0, 4096, p, p, p, 50, 1, p, p, None) == -22
    assert mw(p, 8, 16000, p, 4, 16001, p, p, p, 50, 1, p, p, None) == -22
    assert mw(p, 0, 16000, p, 4, 4096, p, p, p, 50, 1, p, p, None) == -22                         # C = 0
    assert mw(p, 8, 16000, None, 4, 4096, p, p, p, 50, 1, p, p, None) == -22                      # no start table
    assert mw(p, 8, 16000, p, 4, 4096, p, p, p, 50, 1, None, p, None) == -22                      # the dB conversion needs its workspace
    assert mw(p, 8, 16000, p, 4, 4096, p, p, p, 50, 2, p, p, None) == -22                         # db is 0 or 1
    ra = dll.mmd_det_record_append
    assert ra(None, p, 3, 4, p, p, p, 6, p, p, None) == -22
    assert ra(p, p, 3, 4, None, p, p, 6, p, p, None) == -22
    assert ra(p, p, 3, 4, p, p, p, 6, None, p, None) == -22
    for bad in ((0, 4, 6), (1025, 4, 6), (3, 0, 6), (3, 4, 0), (-3, 4, 6)):
        assert ra(p, p, bad[0], bad[1], p, p, p, bad[2], p, p, None) == -22, bad
