"""The old cacophony index restated for the tests (reference
src/cacophony_index.py:53-97): the seeded inputs, the float64 band energies
through ``scipy.fftpack.dct`` (the reference's own transform), an independent
float64 route to the same energies (numpy's FFT through Makhoul's reordering)
and the points.  tests/test_cacophony_host.py pins ``bins`` and ``points``
against the recorded reference results (tests/golden/cacophony_index.json), so
the GPU tests can use them for inputs the fixture does not hold.
"""
from __future__ import annotations

import math

import numpy as np

SR = 16000
N = 2048
HOP = 1024

# n_samples of the fixture's cases; "silence" is the 336000-sample clip with
# its middle third zeroed
CASES = {"n4096": 4096, "n4097": 4097, "n5121": 5121, "n287999": 16000 * 18 - 1, "n320000": 320000,
         "n336000": 336000, "n720000": 720000, "n960000": 960000, "silence": 336000}
SEEDS = {name: 100 + i for i, name in enumerate(CASES)}


def clip(seed: int, n: int, sr: int = SR) -> np.ndarray:
    """int16-quantised white noise at -30 dBFS plus tone bursts at -12 dBFS
    (one per 1.5 s, 0.1-0.6 s long, Hann-shaped), scaled by 1/32768 like a
    decoded PCM16 file."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n) * 10 ** (-30 / 20)
    for _ in range(1 + n // (3 * sr // 2)):
        dur = int(rng.uniform(0.1, 0.6) * sr)
        i0 = int(rng.integers(0, max(n - dur, 1)))
        i1 = min(n, i0 + dur)
        f = rng.uniform(0.0125, 0.45) * sr
        x[i0:i1] += 10 ** (-12 / 20) * np.sin(2 * np.pi * f * np.arange(i1 - i0) / sr) * np.hanning(i1 - i0)
    q = np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)
    return q.astype(np.float32) / np.float32(32768.0)


def case_clip(name: str) -> np.ndarray:
    x = clip(SEEDS[name], CASES[name])
    if name == "silence":
        x[len(x) // 3: 2 * len(x) // 3] = 0.0
    return x


def edges() -> np.ndarray:
    cut = 100 * 2 * N // SR
    return np.logspace(math.log10(cut), math.log10(N), num=11, dtype=int)


def n_frames(n: int) -> int:
    return len(range(HOP, n - 3 * HOP, HOP))


def _band_sums(y: np.ndarray, e) -> np.ndarray:
    # the reference's sum(x * x): a left-to-right float64 sum (cumsum's order)
    out = np.zeros(len(e) - 1)
    for b in range(len(e) - 1):
        sq = y[e[b]:e[b + 1]] ** 2
        out[b] = np.cumsum(sq)[-1] if len(sq) else 0.0
    return out


def bins(x: np.ndarray, frames=None) -> np.ndarray:
    """float64 [F][10]: the reference's band energies of every frame (or of
    the frame indices in ``frames``)."""
    import scipy.fftpack
    w = np.hanning(N)
    e = edges()
    idx = range(n_frames(len(x))) if frames is None else frames
    out = np.zeros((len(idx), 10))
    for i, f in enumerate(idx):
        o = HOP * (f + 1)
        out[i] = _band_sums(scipy.fftpack.dct(w * x[o:o + N]), e)
    return out


def bins_makhoul(x: np.ndarray) -> np.ndarray:
    """The same energies by another float64 algorithm: the DCT-II as the FFT
    of the even/odd reordered frame (Makhoul 1980), all frames at once."""
    F = n_frames(len(x))
    if F == 0:
        return np.zeros((0, 10))
    w = np.hanning(N)
    s = np.stack([w * x[HOP * (f + 1): HOP * (f + 1) + N] for f in range(F)])
    v = np.concatenate([s[:, 0::2], s[:, 1::2][:, ::-1]], axis=1)
    V = np.fft.fft(v, axis=1)
    k = np.arange(N)
    y = 2.0 * (V.real * np.cos(np.pi * k / (2 * N)) + V.imag * np.sin(np.pi * k / (2 * N)))
    e = edges()
    sq = y * y
    return np.stack([sq[:, e[b]:e[b + 1]].sum(axis=1) for b in range(10)], axis=1)


def points(b: np.ndarray) -> np.ndarray:
    """int [F - 1]: bands that more than halved plus bands that more than doubled."""
    if len(b) < 2:
        return np.zeros(0, np.int64)
    cur, prev = b[1:], b[:-1]
    return ((cur * 2 < prev).sum(axis=1) + (cur > prev * 2).sum(axis=1)).astype(np.int64)


def near_decisions(b: np.ndarray, rel: float = 1e-9) -> np.ndarray:
    """bool [F - 1][10]: comparisons whose ratio cur / prev is within ``rel``
    (relative) of 2 or 1/2, where a float64 rounding could flip the decision.
    A zero on either side is never near: 0 against anything is decided by the
    zero alone."""
    if len(b) < 2:
        return np.zeros((0, 10), bool)
    cur, prev = b[1:], b[:-1]
    live = (cur != 0) & (prev != 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(live, cur / np.where(live, prev, 1.0), 1.0)
    return live & ((np.abs(r - 2.0) <= 2.0 * rel) | (np.abs(r - 0.5) <= 0.5 * rel))
