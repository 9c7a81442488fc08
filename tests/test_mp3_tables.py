"""The restated tables of ISO/IEC 11172-3 Layer III (csrc/aa_mp3_tables.h, read
through aa_mp3_table: the decoder's own single copy) held to structure, since
nothing the project can read holds the standard's tables: every Huffman table
prefix-free with Kraft sum exactly 1 (none of the standard's tables is
incomplete), dimensions, linbits, band edges, the synthesis window's
integrality and peak, and perfect reconstruction through the standard's
analysis filterbank followed by the decoder's synthesis."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import mp3_writer as mw
from aa_amd import _lib

TABLES = [t for t in range(1, 34) if t not in (4, 14)]
DIMS = {1: 2, 2: 3, 3: 3, 5: 4, 6: 4, 7: 6, 8: 6, 9: 6, 10: 8, 11: 8, 12: 8, 13: 16, 15: 16}


@pytest.mark.parametrize("t", TABLES)
def test_huffman_table_is_a_complete_prefix_code(t):
    code, ln = mw.table(0, t), mw.table(1, t)
    assert len(code) == len(ln) == (16 if t >= 32 else DIMS.get(t, 16) ** 2)
    assert (ln >= 1).all() and (ln <= 19).all() and (code < (1 << ln.astype(np.int64))).all()
    assert sum(Fraction(1, 1 << int(n)) for n in ln) == 1
    words = sorted(format(int(c), "b").zfill(int(n)) for c, n in zip(code, ln))
    assert all(not b.startswith(a) for a, b in zip(words, words[1:]))  # (sorted: a prefix sorts right before)


def test_tables_that_do_not_exist():
    n = C.c_int64()
    for t in (0, 4, 14, 34):
        assert _lib.lib().aa_mp3_table(0, t, None, 0, C.byref(n)) == _lib.AA_ERR_INVALID


def test_shared_code_sets_and_linbits():
    for t in range(17, 24):
        assert np.array_equal(mw.table(0, t), mw.table(0, 16)) and np.array_equal(mw.table(1, t), mw.table(1, 16))
    for t in range(25, 32):
        assert np.array_equal(mw.table(0, t), mw.table(0, 24)) and np.array_equal(mw.table(1, t), mw.table(1, 24))
    lb = mw.table(2)
    assert lb[:16].tolist() == [0] * 16
    assert lb[16:24].tolist() == [1, 2, 3, 4, 6, 8, 10, 13] and lb[24:].tolist() == [4, 5, 6, 7, 8, 9, 11, 13]
    assert mw.table(0, 33).tolist() == list(range(15, -1, -1)) and mw.table(1, 33).tolist() == [4] * 16


def test_slen_and_pretab():
    assert mw.table(3, 0).tolist() == [0, 0, 0, 0, 3, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4]
    assert mw.table(3, 1).tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 1, 2, 3, 1, 2, 3, 2, 3]
    p = mw.table(4)
    assert len(p) == 22 and p[:11].tolist() == [0] * 11 and p.max() == 3 and p[21] == 0


@pytest.mark.parametrize("sr", [0, 1, 2])
def test_band_edges(sr):
    lo, sh = mw.table(5, sr), mw.table(6, sr)
    assert len(lo) == 23 and lo[0] == 0 and lo[-1] == 576 and (np.diff(lo) > 0).all()
    assert len(sh) == 14 and sh[0] == 0 and sh[-1] == 192 and (np.diff(sh) > 0).all()
    assert lo[8] == 36 and sh[3] == 12  # a mixed block's long part ends where its short bands begin
    assert (lo % 2 == 0).all()          # region boundaries fall between pairs


def test_synthesis_window_shape():
    d = mw.table(7)
    assert len(d) == 512 and d.dtype == np.int32  # D * 65536 is integral by construction of the accessor
    assert d[0] == 0 and np.abs(d).max() == 75038 == d[256]
    assert abs(75038 / 65536 - 1.144989014) < 5e-10  # the standard prints 1.144989014
    h = d * np.array([(-1) ** (n // 64) for n in range(512)])  # the prototype behind the sign flips
    assert np.array_equal(h[1:], h[1:][::-1])                  # is symmetric about 256


def _analysis(x, d):
    """The standard's analysis filterbank (C.1.3): subband samples [slots][32]."""
    c = d / 65536.0 / 32.0
    i64 = np.arange(64)
    m = np.cos((2 * np.arange(32)[:, None] + 1) * (i64[None, :] - 16) * np.pi / 64)
    buf, out = np.zeros(512), []
    for b in range(len(x) // 32):
        buf[32:] = buf[:-32].copy()
        buf[:32] = x[b * 32:b * 32 + 32][::-1]
        out.append(m @ (c * buf).reshape(8, 64).sum(0))
    return np.array(out)


@pytest.mark.parametrize("freq", [1000.0, 9000.0])
def test_analysis_then_core_synthesis_reconstructs(freq):
    """60 dB is a condition, not a measurement: below it a misprinted window
    coefficient would show above about 32 LSB of s16.  Measured: 95.6 dB at
    1 kHz and 86.9 dB at 9 kHz (the filterbank's own reconstruction error)."""
    n = 32 * 200
    x = 0.5 * np.sin(2 * np.pi * freq * np.arange(n) / 44100.0)
    sb = np.ascontiguousarray(_analysis(x, mw.table(7)))
    y = np.zeros(n)
    _lib.check(_lib.lib().aa_mp3_synth_host(sb.ctypes.data, len(sb), y.ctypes.data), "aa_mp3_synth_host")
    delay = 481
    a, b = x[1024:n - delay], y[1024 + delay:]
    snr = 10 * np.log10(np.mean(a ** 2) / np.mean((b - a) ** 2))
    print(freq, "Hz: SNR", snr, "dB")
    assert snr >= 60.0
