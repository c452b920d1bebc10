"""detect.py's window-CSV writer and its feed loop, without a GPU.  The writer: the bytes of the stream, track, bank and bank + track
forms against literal strings - those the tool's three earlier writers gave for the same arrays - and the two length-mismatch errors.
The feed loop: the calls it makes on a stand-in session and a stand-in bank that write them down."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _detect():
    sys.path.insert(0, ROOT)
    import detect
    return detect


# ---------------------------------------------------------------------------------------------- the writer
ROWS = np.array([[1, 2, 30, 40, 0.1 + 0.2, 6], [0, 0, 128, 127, np.float32(1) / 3, 6], [5, 6, 7, 8, 0.999999, 14]], np.float32)
WINDOW, TRACK, SESSION = np.array([0, 3, 7], np.int32), np.array([0, -1, 12], np.int32), np.array([1, 0, 1], np.int32)
HOP = 1531


def test_window_csv_bytes_of_the_four_forms(tmp_path):
    det = _detect()
    f = str(tmp_path / "w.csv")
    assert det.write_windows_csv(f, ROWS, WINDOW, HOP) == 3
    assert open(f, "rb").read() == (b"window,t_start_s,x1,y1,x2,y2,score,label\r\n"
                                    b"0,0,1,2,30,40,0.300000012,6\r\n"
                                    b"3,0.10414966,0,0,128,127,0.333333343,6\r\n"
                                    b"7,0.243015873,5,6,7,8,0.999998987,14\r\n")
    assert det.write_windows_csv(f, ROWS, WINDOW, HOP, TRACK) == 3
    assert open(f, "rb").read() == (b"window,t_start_s,x1,y1,x2,y2,score,label,track\r\n"
                                    b"0,0,1,2,30,40,0.300000012,6,0\r\n"
                                    b"3,0.10414966,0,0,128,127,0.333333343,6,-1\r\n"
                                    b"7,0.243015873,5,6,7,8,0.999998987,14,12\r\n")
    assert det.write_windows_csv(f, ROWS, WINDOW, HOP, session=SESSION) == 3
    assert open(f, "rb").read() == (b"session,window,t_start_s,x1,y1,x2,y2,score,label\r\n"
                                    b"1,0,0,1,2,30,40,0.300000012,6\r\n"
                                    b"0,3,0.10414966,0,0,128,127,0.333333343,6\r\n"
                                    b"1,7,0.243015873,5,6,7,8,0.999998987,14\r\n")
    assert det.write_windows_csv(f, ROWS, WINDOW, HOP, TRACK, SESSION) == 3
    assert open(f, "rb").read() == (b"session,window,t_start_s,x1,y1,x2,y2,score,label,track\r\n"
                                    b"1,0,0,1,2,30,40,0.300000012,6,0\r\n"
                                    b"0,3,0.10414966,0,0,128,127,0.333333343,6,-1\r\n"
                                    b"1,7,0.243015873,5,6,7,8,0.999998987,14,12\r\n")


@pytest.mark.parametrize("window,track,session,message", [
    (WINDOW, TRACK[:2], None, "write_track_csv: 3 rows, 3 windows, 2 track ids"),
    (WINDOW[:1], TRACK, None, "write_track_csv: 3 rows, 1 windows, 3 track ids"),
    (WINDOW, None, SESSION[:2], "write_bank_csv: 3 rows, 2 sessions, 3 windows, 3 track ids"),
    (WINDOW, TRACK[:1], SESSION, "write_bank_csv: 3 rows, 3 sessions, 3 windows, 1 track ids"),
    (WINDOW[:2], TRACK, SESSION, "write_bank_csv: 3 rows, 3 sessions, 2 windows, 3 track ids")])
def test_window_csv_refuses_columns_of_unequal_length(tmp_path, window, track, session, message):
    det = _detect()
    with pytest.raises(ValueError) as e:
        det.write_windows_csv(str(tmp_path / "x.csv"), ROWS, window, HOP, track, session)
    assert str(e.value) == message
    assert not os.path.exists(tmp_path / "x.csv")


# ---------------------------------------------------------------------------------------------- the feed loop
class _Fake:
    """a session or a bank that writes its calls into `log` and returns a part that names the call"""

    def __init__(self, log):
        self.log = log

    def _call(self, *call):
        self.log.append(call)
        return [call]

    def push(self, *a):
        return self._call("push", *a)

    def push_pcm(self, *a):
        return self._call("push_pcm", *a)

    def push_all_pcm(self, chunks, widths):
        return self._call("push_all_pcm", dict(chunks), dict(widths))

    def flush(self):
        return self._call("flush")

    def close(self):
        self.log.append(("close",))

    def concat(self, parts):
        return [call for p in parts for call in p]


def _sources(log, lengths=(3, 1, 2), width=2):
    """source k yields ("c<k><i>", width) for i < lengths[k] and writes ("pull", k, i) into log when chunk i is asked for"""
    def source(k, n):
        for i in range(n):
            log.append(("pull", k, i))
            yield "c%d%d" % (k, i), width
        log.append(("end", k))
    return [source(k, n) for k, n in enumerate(lengths)]


def test_feed_pushes_each_chunk_before_the_next_source_is_touched():
    det = _detect()
    log = []
    got = det.feed(_Fake(log), _sources(log), det.push_bank)
    pushes = [("push_pcm", 0, "c00", 2), ("push_pcm", 1, "c10", 2), ("push_pcm", 2, "c20", 2), ("push_pcm", 0, "c01", 2),
              ("push_pcm", 2, "c21", 2), ("push_pcm", 0, "c02", 2)]
    assert [c for c in log if c[0] not in ("pull", "end")] == pushes + [("flush",), ("close",)]
    assert got == pushes + [("flush",)]                                     # concat of what the pushes and the flush returned
    # chunk i of source k is pulled, then pushed, and only then is another source asked: one chunk in host memory
    for n, c in enumerate(log):
        if c[0] == "pull":
            assert log[n + 1] == ("push_pcm", c[1], "c%d%d" % (c[1], c[2]), 2), (n, log)
    assert [c for c in log if c[0] in ("pull", "end")] == [("pull", 0, 0), ("pull", 1, 0), ("pull", 2, 0), ("pull", 0, 1), ("end", 1), ("pull", 2, 1),
                                                           ("pull", 0, 2), ("end", 2), ("end", 0)]


def test_feed_hands_a_bank_float_chunks_as_push():
    det = _detect()
    log = []
    det.feed(_Fake(log), _sources([], (1, 2), None), det.push_bank)
    assert log == [("push", 0, "c00"), ("push", 1, "c10"), ("push", 1, "c11"), ("flush",), ("close",)]


def test_feed_collects_a_round_for_one_push_all_pcm():
    det = _detect()
    log = []
    sources = [iter([("c00", 2), ("c01", 2), ("c02", 2)]), iter([("c10", 3)]), iter([("c20", 4), ("c21", 4)])]
    got = det.feed(_Fake(log), sources)
    rounds = [("push_all_pcm", {0: "c00", 1: "c10", 2: "c20"}, {0: 2, 1: 3, 2: 4}), ("push_all_pcm", {0: "c01", 2: "c21"}, {0: 2, 2: 4}),
              ("push_all_pcm", {0: "c02"}, {0: 2})]
    assert log == rounds + [("flush",), ("close",)]                         # no empty round behind the last chunk
    assert [list(c[1]) for c in log[:3]] == [[0, 1, 2], [0, 2], [0]]        # ascending sessions, as they were read
    assert got == rounds + [("flush",)]


@pytest.mark.parametrize("width,calls", [(None, [("push", "c00"), ("push", "c01")]), (3, [("push_pcm", "c00", 3), ("push_pcm", "c01", 3)])])
def test_feed_pushes_one_source_into_a_session(width, calls):
    det = _detect()
    log = []
    got = det.feed(_Fake(log), _sources([], (2,), width), det.push_session)
    assert log == calls + [("flush",), ("close",)] and got == calls + [("flush",)]


def test_feed_of_no_chunks_flushes_and_closes():
    det = _detect()
    log = []
    assert det.feed(_Fake(log), [iter(())], det.push_session) == [("flush",)] and log == [("flush",), ("close",)]
    log.clear()
    assert det.feed(_Fake(log), [iter(()), iter(())]) == [("flush",)] and log == [("flush",), ("close",)]
