"""MP3 decode on a real file: tests/golden/mp3/invalid_keypress.mp3
(libmp3lame through ffmpeg; provenance in tests/golden/mp3/README.md), the
decoder's pin against an encoder it shares nothing with.  The file uses every
block type, scfsi, MS stereo, the bit reservoir and every Huffman code set but
table 10's, so a wrong code word, band edge or window desynchronises it: the
granules would stop ending on part2_3_length and the cross-codec SNR against
the libVorbis encode of the same sound would fall to about 0 dB."""
import ctypes as C
import hashlib
import time
from pathlib import Path

import numpy as np
import pytest

import mp3_cases as mc
import mp3_writer as mw
from aa_amd import _lib, audio
from aa_amd import identify_tracks as it
from aa_amd import mp3_gpu as mg

GOLDEN = Path(__file__).resolve().parent / "golden"
REAL = GOLDEN / "mp3" / "invalid_keypress.mp3"
OGG = GOLDEN / "vorbis" / "invalid_keypress.ogg"


def test_fixture_is_the_file_described():
    data = REAL.read_bytes()
    assert len(data) == 9030
    assert hashlib.sha256(data).hexdigest() == "209e658a7ee725011f7d41e077f7170074da9d8123ac739a7326fa41ba1dbbe0"
    assert audio._is_mp3(data)
    info = _lib.Mp3Info()
    buf = np.frombuffer(data, np.uint8)
    _lib.check(_lib.lib().aa_mp3_info(buf.ctypes.data, buf.size, C.byref(info)), "aa_mp3_info")
    assert (info.sample_rate, info.channels, info.n_frames, info.delay, info.padding) == (44100, 2, 21, 576, 0)
    assert info.total_frames == 21 * 1152 - 1105 == 23087


def test_real_file_decodes_clean():
    ix = mg.index(REAL.read_bytes())
    f = ix.frames
    assert len(f) == 21 and bool(f["ms"].all())
    assert {0, 1, 2, 3} <= set(f["block_type"].reshape(-1).tolist()) and f["scfsi"].any()
    assert int(f["main_at"][0]) == 0 and (np.diff(f["main_end"]) > 0).all()
    used = set(f["table_select"].reshape(-1).tolist()) - {0}
    assert 10 not in used and {1, 2, 3, 5, 6, 7, 8, 9, 11, 12, 13, 15, 19, 24} <= used
    f32, s16, st = mg.decode_frames_host(ix.payload, f, ix.stream)
    assert not st.any()  # every granule OK: no big-values region overran its part2_3_length
    assert len(f32) == 23087 * 2 and np.abs(f32).max() < 1.0
    x, sr = audio.decode(str(REAL))
    assert sr == 44100 and x.dtype == np.float32 and x.shape == (23087,)
    assert np.array_equal(x, audio._to_mono(s16, 2))


def test_granules_end_on_part2_3_length():
    """Where each granule's Huffman data stop against part2_3_length: a
    desynchronised decode stops anywhere, a right one on the last bit (or short
    of it by stuffing bits) and never beyond.  Recorded: of the file's 84
    granules 47 are empty (part2_3_length 0); of the other 37, all 37 (100 %) end
    exactly on part2_3_length, none overshoots (no dropped quadruple)."""
    ix = mg.index(REAL.read_bytes())
    _, _, st, left = mg.decode_frames_host(ix.payload, ix.frames, ix.stream, want_left=True)
    used = ix.frames["part2_3_length"].reshape(-1, 2, 2) > 0
    print("granules:", used.size, "non-empty:", int(used.sum()), "ending exactly:", int((left[used] == 0).sum()),
          "left bits:", sorted(set(left[used].tolist())))
    assert not st.any() and used.sum() == 37 and (left >= 0).all()
    assert (left[used] == 0).sum() >= 30


def _mono(path):
    x, sr = it.load_recording(str(path), resample=None)
    assert sr == 44100
    return x.astype(np.float64)


def test_cross_codec_snr_against_the_vorbis_fixture():
    """The same sound through libmp3lame and through libVorbis: aligned by
    cross-correlation within +-3000 samples, gain fitted by least squares, the
    SNR of the mono mix must be >= 10 dB (a desynchronised decode gives about
    0 dB).  Measured: 74.6 dB at lag 0 with gain 1.053 -- lag 0 also pins the
    start trim (delay + 529)."""
    a, b = _mono(REAL), _mono(OGG)
    n = min(len(a), len(b))
    spec = np.fft.irfft(np.fft.rfft(a, 1 << 16) * np.conj(np.fft.rfft(b, 1 << 16)))
    lags = np.concatenate([np.arange(0, 3001), np.arange(-3000, 0)])
    lag = int(lags[np.argmax(np.concatenate([spec[:3001], spec[-3000:]]))])
    x, y = a[max(0, lag):], b[max(0, -lag):]
    m = min(len(x), len(y))
    x, y = x[:m], y[:m]
    gain = (x @ y) / (x @ x)
    snr = 10 * np.log10((y @ y) / ((y - gain * x) @ (y - gain * x)))
    print("lag", lag, "gain", gain, "SNR", snr, "dB")
    assert m >= 20000 and snr >= 10.0


def _hdr(version=3, layer=1, br=9, sr=0, mode=0, ext=0):
    return bytes([0xFF, 0xE0 | (version << 3) | (layer << 1) | 1, (br << 4) | (sr << 2), (mode << 6) | (ext << 4)])


@pytest.mark.parametrize("what,hdr", [("mpeg2", _hdr(version=2)), ("mpeg2.5", _hdr(version=0)),
                                      ("layer2", _hdr(layer=2)), ("layer1", _hdr(layer=3)),
                                      ("free_format", _hdr(br=0))])
def test_declined_formats_raise(tmp_path, what, hdr):
    data = (hdr + bytes(413)) * 4
    buf = np.frombuffer(data, np.uint8)
    info = _lib.Mp3Info()
    assert _lib.lib().aa_mp3_info(buf.ctypes.data, buf.size, C.byref(info)) == _lib.AA_ERR_UNSUPPORTED
    p = tmp_path / f"{what}.mp3"
    p.write_bytes(data)
    with pytest.raises(Exception, match="Could not load"):
        it.load_recording(str(p))


def test_intensity_stereo_is_declined(tmp_path):
    data = bytearray(mc.case("malformed_granule")["data"])
    at = [i for i in range(len(data) - 4) if data[i] == 0xFF and data[i + 1] == 0xFB]
    data[at[1] + 3] = (1 << 6) | (1 << 4)  # the second frame: joint stereo with intensity on
    buf = np.frombuffer(bytes(data), np.uint8)
    info = _lib.Mp3Info()
    assert _lib.lib().aa_mp3_info(buf.ctypes.data, buf.size, C.byref(info)) == _lib.AA_ERR_UNSUPPORTED
    assert b"intensity" in _lib.lib().aa_last_error()
    p = tmp_path / "is.mp3"
    p.write_bytes(bytes(data))
    with pytest.raises(Exception, match="Could not load"):
        it.load_recording(str(p))


def test_not_an_mp3(tmp_path):
    assert not audio._is_mp3(b"ID3" + b"\0" * 64) and not audio._is_mp3(b"RIFF" + b"\0" * 64)
    assert not audio._is_mp3(_hdr() + bytes(60))  # one header, no second one where its frame ends
    buf = np.zeros(512, np.uint8)
    info = _lib.Mp3Info()
    assert _lib.lib().aa_mp3_info(buf.ctypes.data, buf.size, C.byref(info)) == _lib.AA_ERR_INVALID


def test_container_details():
    """ID3v2 in front, the Info frame, CRC words, padding, VBR, junk and an
    ID3v1 tag behind: five audio frames, trimmed by the tag's delay and padding."""
    c = mc.case("reservoir_vbr_32k")
    assert c["data"][:3] == b"ID3" and c["data"][-128:-125] == b"TAG" and audio._is_mp3(c["data"])
    ix = mg.index(c["data"])
    s = ix.stream[0]
    assert (int(s["n_frames"]), int(s["skip"]), int(s["frames"])) == (5, 576 + 529, 5 * 1152 - 1000 + 529 - 1105)
    assert (ix.frames["main_at"] < np.concatenate([[0], ix.frames["main_end"][:-1]])).any()  # the reservoir is used
    # the same frames without a tag: nothing is trimmed
    plain = mw.stream(c["frames"], c["sr_index"], c["channels"])
    assert int(mg.index(plain).stream["frames"][0]) == 5 * 1152


def test_damaged_streams_return_in_bounded_time():
    t0 = time.perf_counter()
    seen = set()
    for name, bad in mc.fuzz():
        rc, ix = mg.index_rc(bad)
        assert rc in (_lib.AA_OK, _lib.AA_ERR_INVALID, _lib.AA_ERR_UNSUPPORTED), name
        if ix is None:
            continue
        f32, s16, st = mg.decode_frames_host(ix.payload, ix.frames, ix.stream)
        assert set(np.unique(st).tolist()) <= {0, 1, 2} and np.isfinite(f32).all(), name
        assert len(f32) == int(ix.stream["frames"][0] * ix.stream["channels"][0])  # damage never moves the timeline
        seen |= set(np.unique(st).tolist())
    assert len(mc.fuzz()) == 200 and seen == {0, 1, 2}
    assert time.perf_counter() - t0 < 60.0
