"""dB mel front end and audio-only detection, CPU side: the C ABI of the three new entry points without a GPU, closed forms of the
power_to_db restatement (tests/melspec_db_ref.py), detect.py's input readers and the cfg key audio_db."""
import ctypes
import os
import sys
import wave

import numpy as np
import pytest
import torch

import melspec_db_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mmd_melspec_batch", "mmd_power_to_db", "mmd_resize_cubic_batch")


def _detect():
    sys.path.insert(0, ROOT)
    import detect
    return detect


# ---------------------------------------------------------------------------------------------- C ABI without a GPU
def test_header_declares_the_new_entry_points():
    import __graft_entry__ as ge
    ge.build()
    from mm_distillnet_amd import _lib
    sigs = _lib.LIB.symbols()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    text = open(_lib.HEADER).read()
    for name in NEW:
        assert name in sigs and hasattr(dll, name), name
        head = text[:text.index("int %s(" % name)]
        comment = head[head.rindex("\n\n"):]
        assert "src/datasets/" in comment or "transformations.py" in comment, name           # the reference lines it restates
    for name in ("mmd_melspec_batch", "mmd_power_to_db"):
        head = text[:text.index("int %s(" % name)]
        comment = head[head.rindex("\n\n"):]
        assert "mp3_to_pkl.py:31-41" in comment and "UNPINNED" in comment and "need no zeroing" in comment.replace("needs", "need"), name
    assert len(sigs["mmd_melspec_batch"]) == 13 and len(sigs["mmd_power_to_db"]) == 7 and len(sigs["mmd_resize_cubic_batch"]) == 8


def test_bad_arguments_are_rejected_without_gpu():
    import __graft_entry__ as ge
    ge.build()
    from mm_distillnet_amd import _lib
    dll = _lib.LIB.load()
    p = ctypes.c_void_p(4096)            # never dereferenced: validation precedes any launch
    mb = dll.mmd_melspec_batch
    assert mb(None, None, 3, 8, 44100, p, p, p, 50, 0, None, p, None) == -22
    assert mb(p, None, 3, 8, 44100, None, p, p, 50, 0, None, p, None) == -22
    assert mb(p, None, 3, 8, 44100, p, None, p, 50, 0, None, p, None) == -22
    assert mb(p, None, 3, 8, 44100, p, p, None, 50, 0, None, p, None) == -22
    assert mb(p, None, 3, 8, 44100, p, p, p, 50, 0, None, None, None) == -22
    assert mb(p, p, 0, 8, 44100, p, p, p, 50, 0, p, p, None) == -22
    assert mb(p, p, -1, 8, 44100, p, p, p, 50, 1, p, p, None) == -22
    assert mb(p, p, 3, 0, 44100, p, p, p, 50, 1, p, p, None) == -22
    assert mb(p, p, 3, 8, 512, p, p, p, 50, 1, p, p, None) == -22
    assert mb(p, p, 3, 8, 44100, p, p, p, 0, 1, p, p, None) == -22
    assert mb(p, p, 3, 8, 44100, p, p, p, 52, 1, p, p, None) == -22       # 80 * 52 floats do not fit the kernel's LDS table
    assert mb(p, p, 3, 8, 44100, p, p, p, 50, 2, p, p, None) == -22       # db is 0 or 1
    assert mb(p, p, 3, 8, 44100, p, p, p, 50, 1, None, p, None) == -22    # the dB conversion needs its workspace
    pd = dll.mmd_power_to_db
    assert pd(None, 3, 80, 9, 8, p, None) == -22
    assert pd(p, 3, 80, 9, 8, None, None) == -22
    for bad in ((0, 80, 9, 8), (3, 0, 9, 8), (3, 80, 0, 8), (3, 80, 9, 0), (3, 80, -9, 8), (3, 80, 9, 1025)):
        assert pd(p, *bad, p, None) == -22, bad
    rb = dll.mmd_resize_cubic_batch
    assert rb(None, 3, 80, 9, 8, 96, p, None) == -22
    assert rb(p, 3, 80, 9, 8, 96, None, None) == -22
    for bad in ((0, 80, 9, 8, 96), (3, 0, 9, 8, 96), (3, 80, 0, 8, 96), (3, 80, 9, 0, 96), (3, 80, 9, 8, 0), (-3, 80, 9, 8, 96)):
        assert rb(p, *bad, p, None) == -22, bad


# ---------------------------------------------------------------------------------------------- closed forms of the restatement
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_power_to_db_closed_forms(dtype):
    assert np.array_equal(D.power_to_db_ref(np.zeros((80, 5)), dtype), np.zeros((80, 5), dtype))            # silence: 0 dB everywhere
    tiny = np.random.default_rng(0).random((80, 5)) * 9e-11                                                  # maximum below amin
    assert np.array_equal(D.power_to_db_ref(tiny, dtype), np.zeros((80, 5), dtype))
    S = np.random.default_rng(1).random((80, 9)) ** 8 * 3e4
    S[3, 4] = 0.0
    db = D.power_to_db_ref(S, dtype)
    assert db.dtype == dtype and db.max() == 0.0 and db.min() >= -80.0 and db[np.unravel_index(S.argmax(), S.shape)] == 0.0
    assert db[3, 4] == -80.0                                                                                 # clipped at top_db
    # decades: S = max * 10^-k -> -10 k dB, the floor at -80
    dec = D.power_to_db_ref(np.array([7.0 * 10.0 ** -k for k in range(12)]), np.float64)
    np.testing.assert_allclose(dec, np.maximum(-10.0 * np.arange(12), -80.0), atol=1e-12)
    # ref = the map's own maximum: a scaled map has the same dB map
    np.testing.assert_allclose(D.power_to_db_ref(S * 1e-3, np.float64)[S > 1e-3], D.power_to_db_ref(S, np.float64)[S > 1e-3], atol=1e-9)


def test_stack_takes_one_maximum_per_microphone():
    from mm_distillnet_amd.data import synthetic_waveforms
    w = synthetic_waveforms(24, 0, 2100).numpy()
    w[2] *= 30.0
    w[5] = 0.0
    st = D.stack_db_ref(w)
    assert st.shape == (80, 9, 8)
    for c in range(8):
        assert st[:, :, c].max() == 0.0 and st[:, :, c].min() >= -80.0
    assert np.array_equal(st[:, :, 5], np.zeros((80, 9)))
    assert np.array_equal(st[:, :, 2], D.melspec_db_ref(w[2]))


# ---------------------------------------------------------------------------------------------- detect.py's readers
def _write_wav(path, pcm, rate=44100, width=2):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(pcm.shape[1]); w.setsampwidth(width); w.setframerate(rate)
        w.writeframes(pcm.astype("<i2" if width == 2 else "u1").tobytes())


def test_detect_reads_npy_waveforms(tmp_path):
    from mm_distillnet_amd import recording as det
    rng = np.random.default_rng(3)
    one, two = rng.standard_normal((8, 700)).astype(np.float32), rng.standard_normal((2, 8, 700)).astype(np.float32)
    np.save(tmp_path / "one.npy", one); np.save(tmp_path / "two.npy", two)
    a, b = det.read_input(str(tmp_path / "one.npy")), det.read_input(str(tmp_path / "two.npy"))
    assert a.dtype == np.float32 and a.shape == (1, 8, 700) and np.array_equal(a[0], one)
    assert b.dtype == np.float32 and b.shape == (2, 8, 700) and np.array_equal(b, two)
    np.save(tmp_path / "f64.npy", one.astype(np.float64)); np.save(tmp_path / "six.npy", one[:6])
    with pytest.raises(ValueError, match="float32"):
        det.read_input(str(tmp_path / "f64.npy"))
    with pytest.raises(ValueError, match="shape"):
        det.read_input(str(tmp_path / "six.npy"))
    with pytest.raises(ValueError, match="unsupported input"):
        det.read_input(str(tmp_path / "clip.mp3"))


def test_detect_reads_pcm16_wav_and_refuses_other_formats(tmp_path):
    from mm_distillnet_amd import recording as det
    pcm = np.random.default_rng(4).integers(-32768, 32768, (900, 8)).astype(np.int16)
    pcm[0, 0], pcm[1, 0] = -32768, 32767
    _write_wav(tmp_path / "ok.wav", pcm)
    a = det.read_input(str(tmp_path / "ok.wav"))
    assert a.dtype == np.float32 and a.shape == (1, 8, 900) and a.flags["C_CONTIGUOUS"]
    assert np.array_equal(a[0], pcm.T.astype(np.float32) / np.float32(32768.0))
    assert a[0, 0, 0] == -1.0 and a[0, 0, 1] == np.float32(32767.0 / 32768.0)
    _write_wav(tmp_path / "slow.wav", pcm, rate=22050)
    with pytest.raises(ValueError, match="22050 Hz is not supported"):
        det.read_input(str(tmp_path / "slow.wav"))
    _write_wav(tmp_path / "narrow.wav", (pcm >> 8) + 128, width=1)
    with pytest.raises(ValueError, match="16-bit PCM"):
        det.read_input(str(tmp_path / "narrow.wav"))
    _write_wav(tmp_path / "stereo.wav", pcm[:, :2])
    with pytest.raises(ValueError, match="8 microphone channels"):
        det.read_input(str(tmp_path / "stereo.wav"))


def test_detect_writes_one_csv_row_per_box(tmp_path):
    det = _detect()
    rows = [np.array([[1, 2, 30, 40, 0.1 + 0.2, 6], [0, 0, 128, 127, np.float32(1) / 3, 6]], np.float32), np.zeros((0, 6), np.float32),
            np.array([[5, 6, 7, 8, 0.999999, 14]], np.float32)]
    assert det.write_csv(str(tmp_path / "o.csv"), rows) == 3
    lines = open(tmp_path / "o.csv").read().strip().split("\n")
    assert lines[0] == "clip,x1,y1,x2,y2,score,label" and len(lines) == 4
    got = np.array([[float(v) for v in ln.split(",")] for ln in lines[1:]])
    assert got[:, 0].tolist() == [0, 0, 2]
    assert np.array_equal(got[:, 1:].astype(np.float32), np.concatenate([rows[0], rows[2]]))


# ---------------------------------------------------------------------------------------------- cfg key audio_db
def test_audio_db_key_is_accepted_and_leaves_samples_unchanged(tmp_path):
    from mm_distillnet_amd.data import RawSyntheticMultimodalDetection, DeviceInputPipeline
    import inspect
    cfg = {"seed": 24, "image_size": 64, "synthetic_wave_samples": 2100, "audio_format": "waveform"}
    plain = RawSyntheticMultimodalDetection(cfg, length=2, frame_hw=(54, 72))
    assert plain.audio_db is False
    for v in (True, "True", "true"):
        ds = RawSyntheticMultimodalDetection(dict(cfg, audio_db=v), length=2, frame_hw=(54, 72))
        assert ds.audio_db is True
        for k in ("rgb", "thermal", "depth", "audio_wave"):
            assert torch.equal(ds[1][k], plain[1][k]), k
    assert RawSyntheticMultimodalDetection(dict(cfg, audio_db="False"), length=2).audio_db is False
    with pytest.raises(Exception, match="Unsupported audio_db"):
        RawSyntheticMultimodalDetection(dict(cfg, audio_db="maybe"), length=2)
    with pytest.raises(Exception, match="audio_format = waveform"):
        RawSyntheticMultimodalDetection({"seed": 24, "image_size": 64, "audio_db": True}, length=2)
    assert inspect.signature(DeviceInputPipeline.__init__).parameters["audio_db"].default is False
    # through the cfg file parser, as train.py reads it
    sys.path.insert(0, ROOT)
    import train
    cfgf = os.path.join(ROOT, "configs", "mm-distillnet.cfg")
    c0, _ = train.parse_config(["--config_file", cfgf])
    c1, _ = train.parse_config(["--config_file", cfgf, "--overwrite", '{"audio_db": "True", "audio_format": "waveform"}'])
    assert c0.getboolean("audio_db", False) is False and c1.getboolean("audio_db", False) is True
    assert RawSyntheticMultimodalDetection(c1, length=2).audio_db is True and RawSyntheticMultimodalDetection(c0, length=2).audio_db is False
