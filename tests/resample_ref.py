"""Restatement of the project's resampling rule (csrc/resample.hip), numpy only.

A band-limited windowed-sinc interpolator after the published design of resampy's `kaiser_best` filter (64 zero crossings, roll-off
0.9475937167399596, Kaiser beta 14.769656459379492), evaluated as an EXACT rational polyphase filter: resampy's interpolated table is
not used, and parity with resampy / librosa themselves is UNPINNED.

    L / M = Fraction(sr_out, sr_in),  scale = min(1, L / M),  half = ceil(Z / scale),  taps = 2 * half
    h(tau) = scale * rolloff * sinc(scale * rolloff * tau) * w(tau * scale / Z)            tau in input samples
    w(u)   = I0(beta * sqrt(1 - u^2)) / I0(beta) for |u| < 1, else 0
    n_out  = ceil(n_in * L / M)
    y[t]   = sum_{k = -half+1 .. half} bank[p][k] * x[n + k],   n = (t * M) // L,  p = (t * M) % L,  bank[p][k] = h(p / L - k)

x is zero outside 0 .. n_in - 1.  The bank is computed in float64 and rounded ONCE to float32; those float32 values are the contract -
the float64 mode below multiplies the same rounded taps and only accumulates wider.  The argument of h is formed as the single quotient
(p - k * L) / L, so bank[p][k] is bit for bit the prototype filter's sample h(m / L) at m = p - k * L.
"""
from fractions import Fraction

import numpy as np

Z, ROLLOFF, BETA = 64, 0.9475937167399596, 14.769656459379492


def ratio(sr_in: int, sr_out: int):
    f = Fraction(int(sr_out), int(sr_in))
    return f.numerator, f.denominator


def n_out(n_in: int, L: int, M: int) -> int:
    return -((-int(n_in) * L) // M)


def half_len(L: int, M: int) -> int:
    return Z if L >= M else -((-Z * M) // L)            # ceil(Z / scale) in integers


def h(m, L: int, M: int):
    """the filter at tau = m / L input samples (m: integer array), float64"""
    scale = 1.0 if L >= M else L / M
    tau = np.asarray(m, np.float64) / L
    u = tau * scale / Z
    inside = np.abs(u) < 1.0
    w = np.where(inside, np.i0(BETA * np.sqrt(np.where(inside, 1.0 - u * u, 0.0))) / np.i0(BETA), 0.0)
    return scale * ROLLOFF * np.sinc(scale * ROLLOFF * tau) * w


def bank(L: int, M: int) -> np.ndarray:
    """float32 [L, 2 * half]: column j holds k = j - half + 1"""
    half = half_len(L, M)
    p = np.arange(L, dtype=np.int64)[:, None]
    k = np.arange(-half + 1, half + 1, dtype=np.int64)[None, :]
    return h(p - k * L, L, M).astype(np.float32)


def resample_ref(x, sr_in: int, sr_out: int = 44100, dtype=np.float64) -> np.ndarray:
    """x [..., n_in] -> [..., n_out] in `dtype`.  float64: the float32 bank times x, accumulated in float64.  float32: every product
    and every sum rounded to float32, the products added one by one in tap order (what a plain kernel loop does: the host-float32
    yardstick of the GPU test)."""
    x = np.asarray(x)
    L, M = ratio(sr_in, sr_out)
    half, b = half_len(L, M), bank(L, M)
    n_in = x.shape[-1]
    t = np.arange(n_out(n_in, L, M), dtype=np.int64)
    n, p = (t * M) // L, (t * M) % L
    pad = [(0, 0)] * (x.ndim - 1) + [(half - 1, half)]
    xp = np.pad(x.astype(dtype), pad)                                                           # xp[n + j] = x[n + k], j = k + half - 1
    bt = b[p].astype(dtype)                                                                     # [n_out, taps]
    acc = np.zeros(x.shape[:-1] + (len(t),), dtype)
    for j in range(2 * half):                                                                   # tap order; numpy rounds each product and sum to `dtype`
        acc = acc + xp[..., n + j] * bt[:, j]
    return acc


def direct_ref(x, sr_in: int, sr_out: int = 44100) -> np.ndarray:
    """The definition the polyphase form restates, float64, 1-D x: zero-stuff by L, convolve with the prototype filter (the float32
    bank's values, h(m / L) for |m| <= half * L), keep every M-th sample."""
    x = np.asarray(x, np.float64)
    L, M = ratio(sr_in, sr_out)
    half = half_len(L, M)
    g = h(np.arange(-half * L, half * L + 1, dtype=np.int64), L, M).astype(np.float32).astype(np.float64)
    up = np.zeros(len(x) * L)
    up[::L] = x
    full = np.convolve(up, g)                                                                   # full[i + half * L] = sum_m g[m] up[i - m]
    t = np.arange(n_out(len(x), L, M), dtype=np.int64)
    return full[t * M + half * L]
