"""Helper (not a test): numpy restatement of the dB step behind the mel spectrogram, `librosa.power_to_db(S, ref=np.max)` as
mp3_to_pkl.py:31-41 calls it on each microphone's [80, T] map (defaults amin = 1e-10, top_db = 80).  librosa is neither part of the
reference tree nor installed here, so the published rule is restated:

  ls = 10 log10(max(amin, S)) - 10 log10(max(amin, max S))
  ls = max(ls, max(ls) - top_db)

PARITY UNPINNED against librosa itself; pinned by the closed forms in tests/test_melspec_db_cpu.py.  `dtype=np.float32` runs the
same three array operations in single precision (what librosa does with a float32 spectrogram): with melspec_ref(..., np.float32)
in front of it, its distance from the float64 chain is the yardstick of tests/test_gpu_melspec_db.py."""
import numpy as np

import melspec_ref as R

AMIN, TOP_DB = 1e-10, 80.0


def power_to_db_ref(S, dtype=np.float64):
    """One channel map [80, T] (any shape: the maximum is over the whole array) of power -> dB in `dtype` arithmetic."""
    S = np.asarray(S, dtype=dtype)
    amin, ten = dtype(AMIN), dtype(10.0)
    ls = ten * np.log10(np.maximum(amin, S))
    ls = ls - ten * np.log10(np.maximum(amin, S.max()))
    assert ls.dtype == dtype
    return np.maximum(ls, ls.max() - dtype(TOP_DB))


def melspec_db_ref(y_a, y_b=None, dtype=np.float64):
    """One channel: float32 waveform(s) [N] -> dB mel spectrogram [80, T], the whole chain in `dtype` arithmetic."""
    return power_to_db_ref(R.melspec_ref(y_a, y_b, dtype=dtype), dtype)


def stack_db_ref(wa, wb=None, dtype=np.float64):
    """[C, N] float32 waveform(s) -> [80, T, C]: one map, and one maximum, per microphone."""
    return np.stack([melspec_db_ref(wa[c], None if wb is None else wb[c], dtype) for c in range(wa.shape[0])], axis=2)
