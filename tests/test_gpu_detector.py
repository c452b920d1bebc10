"""Audio-only detection on the GPU (mm_distillnet_amd/detector.py, detect.py): the student alone, D2 at 128 x 128, B = 2 - the size of
tests/test_gpu_net.py::test_net_eval_golden - against the CPU oracle's forward and post-processing; graph replay against eager bits;
the waveform path; isolation from the teachers; overflow; the command-line tool."""
import os
import sys

import numpy as np
import pytest
import torch

from helpers import make_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, COEF = 128, 2
_STATE = {}


def _inputs(seed, batch=2):
    from mm_distillnet_amd.synth import synth_inputs
    return synth_inputs(batch, S, seed=seed)["audio"]


def _state(kind="spec"):
    """(spec, state): the audio student of test_net_eval_golden with its classifier bias shifted so that detections come out of the
    inputs the test feeds it: the synthetic spectrogram stacks ("spec") or the dB front end's maps of the synthetic waveforms ("wave")"""
    if kind not in _STATE:
        from mm_distillnet_amd.audio import MelFrontEnd
        from mm_distillnet_amd.synth import tune_teacher_bias
        spec, st = make_state(COEF, 8, 13, "audio")
        x = _inputs(24) if kind == "spec" else MelFrontEnd(DEV).student_input(_waves().to(DEV), None, S, db=True).cpu()
        tune_teacher_bias(spec, st, x, DEV, 40)
        _STATE[kind] = (spec, st)
    spec, st = _STATE[kind]
    return spec, {k: v.clone() for k, v in st.items()}


def _detector(kind="spec", **kw):
    from mm_distillnet_amd.detector import AudioDetector
    spec, st = _state(kind)
    det = AudioDetector(spec, DEV, image_size=S, **kw)
    det.load(st)
    return det


def _waves(batch=2, n=8000):
    from mm_distillnet_amd.data import synthetic_waveforms
    return torch.stack([synthetic_waveforms(24, i, n) for i in range(batch)])


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == np.float32 and x.shape == y.shape and x.shape[1:] == (6,), (x.shape, y.shape)
        np.testing.assert_array_equal(x.view(np.int32), y.view(np.int32))


def test_rows_and_head_outputs_against_the_oracle():
    from oracle import effdet_ref as O
    from oracle import postproc_ref as P

    def relerr(a, b):
        a, b = a.detach().cpu().double(), b.detach().cpu().double()
        return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)

    spec, st = _state()
    det = _detector()
    x = _inputs(24)
    rows = det.detect_spectrogram(x.to(DEV))
    det.check_overflow()
    print("detections per image:", [len(r) for r in rows])
    assert len(rows) == 2 and all(5 <= len(r) <= 100 for r in rows), [len(r) for r in rows]
    with torch.no_grad():
        (c, r, a), _ = O.forward(st, x, COEF, False)
    assert det.last_cls.shape == c.shape and det.last_reg.shape == r.shape
    assert relerr(det.last_cls, c) < 1e-3 and relerr(det.last_reg, r) < 1e-3
    # the rows are exactly what the oracle's post-processing makes of the detector's OWN head outputs (the device's logits keep the
    # +-1 px of an int()-truncated edge out of the comparison)
    want = P.logits_to_ground_truth((det.last_cls.cpu(), det.last_reg.cpu(), a), S, 0.3, 0.5)
    for got, w in zip(rows, want):
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got.view(np.int32), np.asarray(w, np.float32).reshape(-1, 6).view(np.int32))
        assert set(got[:, 5].tolist()) == {6.0}


def test_graph_replay_equals_eager_bits():
    xs = [_inputs(24).to(DEV), _inputs(31).to(DEV), _inputs(32).to(DEV)]
    det = _detector()
    first = det.detect_spectrogram(xs[0])
    assert det.graph_replays == 0
    second, third = det.detect_spectrogram(xs[1]), det.detect_spectrogram(xs[2])
    assert det.graph_replays == 2
    _same(first, _detector().detect_spectrogram(xs[0]))
    _same(second, _detector().detect_spectrogram(xs[1]))
    _same(third, _detector().detect_spectrogram(xs[2]))
    assert any(len(a) != len(b) or not np.array_equal(a, b) for a, b in zip(second, third))       # different inputs, different rows
    # another batch size captures anew; the first graph stays usable
    one = det.detect_spectrogram(xs[1][:1])
    assert det.graph_replays == 2
    _same(one, _detector().detect_spectrogram(xs[1][:1]))
    _same(det.detect_spectrogram(xs[2][:1]), _detector().detect_spectrogram(xs[2][:1]))       # replayed B = 1 graph against eager
    _same(det.detect_spectrogram(xs[0]), first)
    assert det.graph_replays == 4
    det.check_overflow()


def test_waveforms_end_to_end_equal_the_front_end_plus_detect_spectrogram():
    det, ref = _detector("wave"), _detector("wave")
    w = _waves().to(DEV)
    want = ref.detect_spectrogram(ref.front.student_input(w, None, S, db=True))
    print("detections per clip:", [len(r) for r in want])
    assert all(5 <= len(r) <= 100 for r in want), [len(r) for r in want]          # the comparison cannot pass on empty lists
    _same(det.detect(w), want)            # eager
    _same(det.detect(w), want)            # replayed
    assert det.graph_replays == 1
    with pytest.raises(ValueError):
        det.detect(w[:, :, :512])         # too short for the reflect padding
    with pytest.raises(ValueError):
        det.detect(w[:, :4])


def test_no_engine_no_teachers_no_oracle(monkeypatch):
    import subprocess
    from mm_distillnet_amd import step

    def refuse(self, *a, **k):
        raise AssertionError("AudioDetector must not build a DistillEngine")

    monkeypatch.setattr(step.DistillEngine, "__init__", refuse)
    det = _detector("wave")
    assert sum(len(r) for r in det.detect(_waves().to(DEV))) > 0
    assert not hasattr(det, "teachers") and not det.net.trainable and det.net.ps.grad is None
    # importing the detector module pulls in neither the oracle nor the distillation step (host-only child process: no GPU use)
    code = ("import sys; sys.path.insert(0, %r); import mm_distillnet_amd.detector; "
            "bad = [m for m in sys.modules if m == 'oracle' or m.startswith('oracle.') or m == 'mm_distillnet_amd.step']; "
            "assert not bad, bad" % ROOT)
    subprocess.run([sys.executable, "-c", code], check=True, timeout=120)


def test_row_capacity_overflow_raises():
    x = _inputs(24).to(DEV)
    full = _detector()
    n = max(len(r) for r in full.detect_spectrogram(x))
    det = _detector(cand_cap=max(1, n // 2))
    det.detect_spectrogram(x)
    assert int(det.overflow.item()) == 1
    with pytest.raises(RuntimeError, match="capacity exceeded"):
        det.check_overflow()
    full.check_overflow()


def test_command_line_tool_writes_the_rows_of_detect(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    sys.path.insert(0, ROOT)
    import detect
    from mm_distillnet_amd import step

    def refuse(self, *a, **k):
        raise AssertionError("detect.py must not build a DistillEngine")

    monkeypatch.setattr(step.DistillEngine, "__init__", refuse)
    spec, st = _state("wave")
    torch.save({"state_dict": st, "epoch": 3}, tmp_path / "student.pth")
    w = _waves()
    np.save(tmp_path / "clips.npy", w.numpy())
    cfgf = os.path.join(ROOT, "configs", "mm-distillnet.cfg")
    rows = detect.main(["--config_file", cfgf, "--checkpoint", str(tmp_path / "student.pth"), "--input", str(tmp_path / "clips.npy"),
                        "--output", str(tmp_path / "out.csv"), "--overwrite", '{"image_size": %d}' % S])
    want = _detector("wave").detect(w.to(DEV))
    _same(rows, want)
    assert sum(len(r) for r in want) > 0
    lines = open(tmp_path / "out.csv").read().strip().split("\n")
    assert lines[0] == "clip,x1,y1,x2,y2,score,label" and len(lines) == 1 + sum(len(r) for r in want)
    got = np.array([[float(v) for v in ln.split(",")] for ln in lines[1:]]).reshape(-1, 7)
    for i, r in enumerate(want):
        np.testing.assert_array_equal(got[got[:, 0] == i][:, 1:].astype(np.float32).view(np.int32), r.view(np.int32))
