"""aa_mp3_decode (the decoder core as host loops) against the numpy float64
oracle (tests/mp3_oracle.py) on the writer's stream table (tests/mp3_cases.py).

The float output is within 2^-24 of the oracle on every case: the decoder
computes in float64 and rounds once to float32, and one float32 rounding of a
value below 1 is at most 2^-25; the float64 paths differ by ~1e-15.  The s16
values equal round(oracle * 32768) except where the oracle lies within 1e-6 of
a rounding tie, and such samples may be at most 0.1 % of a case.

Measured: max |float - oracle| is 4.6e-10 .. 9.3e-10 over the eight cases
(peaks 0.011 .. 0.029), and no s16 sample differs.  The s16 criterion is the
reason the cases are written at a low level: the decoder's one float32
rounding moves a sample by up to |x| * 2^-25, which is |x| * 1e-3 of an s16
step, far more than the 1e-6 window around a tie.  With the same cases written
near full scale (peaks 0.29 .. 0.77; float error 1.4e-8 .. 3.0e-8, still below
2^-24) 7 of 49,840 s16 samples differ from round(oracle * 32768), each within
4.1e-4 of a tie -- the float32 rounding, not the decoder's arithmetic."""
import numpy as np
import pytest

import mp3_cases as mc
import mp3_oracle as mo
from aa_amd import audio
from aa_amd import mp3_gpu as mg


@pytest.fixture(scope="module")
def oracle():
    cache = {}

    def get(name):
        if name not in cache:
            c = mc.case(name)
            pcm = mo.decode(c["frames"], c["sr_index"], c["channels"], c["silent"])
            pcm = pcm[c["skip"]:c["skip"] + c["n_out"]]
            pcm.setflags(write=False)
            cache[name] = pcm
        return cache[name]
    return get


@pytest.mark.parametrize("name", mc.NAMES)
def test_decode_matches_oracle(name, oracle):
    c = mc.case(name)
    ref = oracle(name)
    assert np.abs(ref).max() < 1.0 and np.abs(ref).max() > 1e-4
    f, channels, sr = audio.decode_mp3(c["data"])
    assert channels == c["channels"] and sr == (44100, 48000, 32000)[c["sr_index"]]
    assert len(f) == c["n_out"] * channels
    got = f.reshape(-1, channels).astype(np.float64)
    err = np.abs(got - ref).max()
    print(name, "max |float - oracle| =", err, "peak", np.abs(ref).max())
    assert err <= 2.0 ** -24
    s16 = audio._float_to_s16(f).reshape(-1, channels)
    x = ref * 32768.0
    near_tie = np.abs(np.abs(x - np.floor(x)) - 0.5) < 1e-6
    assert near_tie.mean() <= 1e-3
    np.testing.assert_array_equal(s16[~near_tie], np.rint(x)[~near_tie])


@pytest.mark.parametrize("name", mc.NAMES)
def test_statuses(name):
    c = mc.case(name)
    ix = mg.index(c["data"])
    assert ix is not None and len(ix.frames) == len(c["frames"])
    _, _, st = mg.decode_frames_host(ix.payload, ix.frames, ix.stream)
    want = np.zeros_like(st)
    for (f, gr, ch) in c["silent"]:
        want[f, gr, ch] = 1 if name == "nodata_first" else 2
    np.testing.assert_array_equal(st, want)
