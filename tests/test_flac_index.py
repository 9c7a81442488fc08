"""aa_flac_index (csrc/aa_flac_index.h): the frame table of a FLAC stream,
found without decoding, is exactly what the test encoder (tests/flac_writer.py)
knows it wrote; a sync pattern planted inside a frame's payload is not taken
for a frame start; and anything that would make the table less than certain
is refused with AA_ERR_UNSUPPORTED (the caller then decodes on the host)."""
import ctypes as C

import numpy as np
import pytest

import flac_cases as fc
import flac_writer as fw
from aa_amd import _lib, flac_gpu


def _index_rc(data, cap=None, query=False):
    buf = np.frombuffer(data, np.uint8)
    info, n = _lib.FlacInfo(), C.c_int64(-1)
    tab = np.zeros(cap if cap is not None else 4096, flac_gpu.FRAME)
    rc = _lib.lib().aa_flac_index(buf.ctypes.data, buf.size, C.byref(info), None if query else tab.ctypes.data,
                                  len(tab), C.byref(n))
    return rc, info, tab, n.value


def _check_table(data, frames, block, channels, bits, total):
    rc, info, tab, n = _index_rc(data)
    assert rc == _lib.AA_OK, _lib.lib().aa_last_error()
    assert n == len(frames)
    tab = tab[:n]
    sp = fc.spans(data, frames)
    assert tab["offset"].tolist() == [a for a, _ in sp]
    assert tab["nbytes"].tolist() == [s for _, s in sp]
    blocks = block if isinstance(block, list) else [block] * n
    assert tab["block"].tolist() == blocks
    starts = np.concatenate([[0], np.cumsum(blocks)[:-1]])
    keep = [min(b, total - s) if total else b for b, s in zip(blocks, starts)]
    assert tab["keep"].tolist() == keep
    assert tab["out_at"].tolist() == (starts * channels).tolist()
    assert set(tab["channels"].tolist()) == {channels} and set(tab["bits"].tolist()) == {bits}
    assert set(tab["stream"].tolist()) == {0}
    assert (info.channels, info.bits_per_sample, info.total_frames) == (channels, bits, total)
    # and the public wrapper agrees
    pinfo, ptab = flac_gpu.index(data)
    assert ptab.tobytes() == tab.tobytes() and pinfo.total_frames == sum(keep)
    return tab


# 16: the 8-bit block size code; 1000 and 4608 ("16"): the 16-bit code; the rest: table codes
@pytest.mark.parametrize("block,bs_mode", [(16, "table"), (192, "table"), (576, "table"), (1000, "table"),
                                           (4096, "table"), (4608, "table"), (4608, "16"), (256, "8")])
def test_offsets_block_sizes(block, bs_mode):
    rng = np.random.default_rng(block)
    kind = ("lpc8", {"kind": "lpc", "order": 8, "porder": 3}) if block >= 192 else fc.KINDS[3]
    data, frames, _ = fc.make_stream(rng, 16, [kind], block=block, bs_mode=bs_mode)
    _check_table(data, frames, block, 1, 16, 3 * block)


def test_last_block_cut_by_total():
    rng = np.random.default_rng(1)
    data, frames, _ = fc.make_stream(rng, 16, [fc.KINDS[4]], block=576, cut=100)
    tab = _check_table(data, frames, 576, 1, 16, 3 * 576 - 100)
    assert tab["keep"][-1] == 476


def test_unknown_total_trailing_tag_and_id3():
    rng = np.random.default_rng(2)
    id3 = b"ID3\x04\x00\x00\x00\x00\x00\x05" + b"\x00" * 5
    data, frames, _ = fc.make_stream(rng, 16, [fc.KINDS[8]], block=192, total=0, id3=id3, tag=True, channels=2)
    _check_table(data, frames, 192, 2, 16, 0)


def test_variable_blocksize_sample_numbers():
    rng = np.random.default_rng(3)
    sizes = [17, 192, 300, 4608, 256]
    frames, pos = [], 0
    for bsz in sizes:
        frames.append(fw.frame([fc.signal(rng, bsz, 12)], 12, 32000, pos, variable=True,
                               kinds=[{"kind": "fixed", "order": 1}]))
        pos += bsz
    data = fw.stream(frames, 32000, 1, 12, pos, max(sizes))
    _check_table(data, frames, sizes, 1, 12, pos)


@pytest.mark.parametrize("channels", range(1, 9))
def test_channels(channels):
    rng = np.random.default_rng(channels)
    data, frames, _ = fc.make_stream(rng, 12, [fc.KINDS[1], fc.KINDS[4], fc.KINDS[7]], channels=channels, block=64)
    _check_table(data, frames, 64, channels, 12, 3 * 64)


def _planted(number):
    """Three mono 16-bit frames; frame 1 is VERBATIM and its samples spell a
    whole frame header (sync, codes, `number`, CRC-8) of the stream's shape."""
    rng = np.random.default_rng(9)
    head = bytes([0xFF, 0xF8, 0x19, 0x08, number])  # block code 1 (192), 44.1 kHz code, mono, 16-bit
    head += bytes([fw.crc8(head)])
    x = fc.signal(rng, 192, 16, "noise")
    x[10:13] = np.frombuffer(head, ">i2").astype(np.int64)
    chans = [fc.signal(rng, 192, 16), x, fc.signal(rng, 192, 16)]
    kinds = [{"kind": "fixed", "order": 2}, {"kind": "verbatim"}, {"kind": "fixed", "order": 2}]
    frames = [fw.frame([c], 16, 44100, i, kinds=[k]) for i, (c, k) in enumerate(zip(chans, kinds))]
    data = fw.stream(frames, 44100, 1, 16, 3 * 192, 192)
    assert head in frames[1][6:]
    return data, frames


def test_planted_header_with_wrong_number_is_skipped():
    data, frames = _planted(7)
    _check_table(data, frames, 192, 1, 16, 3 * 192)


def test_planted_header_with_expected_number_keeps_the_core_exact():
    """The planted header carries the number the indexer expects next (2).
    Whatever table comes back, decoding through it gives the host decoder's
    samples or a non-OK status, frame by frame."""
    data, frames = _planted(2)
    q, _, _ = fc.oracle(data)
    ix = flac_gpu.index(data)
    if ix is None:
        return  # refused: the caller decodes on the host
    _, tab = ix
    i32, s16, st = flac_gpu.decode_frames_host(data, tab)
    for f, s in zip(tab, st):
        a, b = int(f["out_at"]), int(f["out_at"]) + int(f["keep"])
        if s == _lib.AA_FLAC_OK:
            np.testing.assert_array_equal(i32[a:b], q[a:b])
            np.testing.assert_array_equal(s16[a:b], fc.to_s16(q[a:b], 16))
    # here the CRC-16 in the index tells the planted header from a frame start
    _check_table(data, frames, 192, 1, 16, 3 * 192)


def test_size_query_and_short_cap():
    rng = np.random.default_rng(4)
    data, frames, _ = fc.make_stream(rng, 16, [fc.KINDS[3]], block=16, n_frames=9)
    rc, _, _, n = _index_rc(data, query=True)
    assert (rc, n) == (_lib.AA_OK, 9)
    rc, _, tab, n = _index_rc(data, cap=4)
    assert (rc, n) == (_lib.AA_ERR_WORKSPACE, 9)
    assert tab["offset"].tolist() == [a for a, _ in fc.spans(data, frames)[:4]]
    rc, _, _, n = _index_rc(data, cap=9)
    assert (rc, n) == (_lib.AA_OK, 9)
    # zero frames: an unknown-length stream that ends after its metadata
    rc, _, _, n = _index_rc(fw.stream([], 48000, 1, 16, 0, 16))
    assert (rc, n) == (_lib.AA_OK, 0)
    # metadata errors are aa_flac_info's
    rc, _, _, _ = _index_rc(b"RIFF" + bytes(64))
    assert rc == _lib.AA_ERR_INVALID


def test_refusals():
    rng = np.random.default_rng(5)
    x = [fc.signal(rng, 192, 16) for _ in range(3)]
    kind = [{"kind": "fixed", "order": 2}]

    def refused(data):
        rc, _, _, _ = _index_rc(data)
        assert rc == _lib.AA_ERR_UNSUPPORTED, rc
        assert flac_gpu.index(data) is None

    # first frame numbered 5 (the host decoder never looks at the number)
    frames = [fw.frame([c], 16, 48000, 5 + i, kinds=kind) for i, c in enumerate(x)]
    data = fw.stream(frames, 48000, 1, 16, 3 * 192, 192)
    assert fc.oracle(data) is not None
    refused(data)
    # headers at odds with STREAMINFO: depth, channels
    frames = [fw.frame([c], 16, 48000, i, kinds=kind) for i, c in enumerate(x)]
    refused(fw.stream(frames, 48000, 1, 24, 3 * 192, 192))
    refused(fw.stream(frames, 48000, 2, 16, 3 * 192, 192))
    # garbage between frames, total known
    good = fw.stream(frames, 48000, 1, 16, 3 * 192, 192)
    at = fc.spans(good, frames)[1][0]
    refused(good[:at] + b"\x00\x01\x02garbage" + good[at:])
    # a damaged frame, a missing frame
    bad = bytearray(good)
    bad[at + 20] ^= 0x10
    refused(bytes(bad))
    refused(fw.stream(frames[:2], 48000, 1, 16, 3 * 192, 192))
    assert flac_gpu.index(good) is not None


def test_oversized_frames_stay_on_the_host_route():
    """block x channels above flac_gpu.MAX_FRAME_SAMPLES would inflate every
    frame's workspace slice of a batch: such a file is not taken by the device path."""
    rng = np.random.default_rng(6)
    ok, _, _ = fc.make_stream(rng, 12, [fc.KINDS[2]], channels=8, block=4096, n_frames=1)
    big, _, _ = fc.make_stream(rng, 12, [fc.KINDS[2]], channels=8, block=4608, n_frames=1)
    assert flac_gpu.MAX_FRAME_SAMPLES == 4096 * 8
    assert flac_gpu.fits_batch(flac_gpu.index(ok)[1]) and not flac_gpu.fits_batch(flac_gpu.index(big)[1])
    assert flac_gpu.fits_batch(flac_gpu.index(fw.stream([], 48000, 1, 16, 0, 16))[1])


def test_is_flac_on_a_buffer():
    from aa_amd.audio import _is_flac
    rng = np.random.default_rng(7)
    id3 = b"ID3\x04\x00\x00\x00\x00\x00\x05" + b"\x00" * 5
    for data in (fc.make_stream(rng, 16, [fc.KINDS[3]], block=16)[0],
                 fc.make_stream(rng, 16, [fc.KINDS[3]], block=16, id3=id3)[0]):
        slot = np.zeros(len(data) + 100, np.uint8)
        slot[:len(data)] = np.frombuffer(data, np.uint8)
        assert _is_flac(data) and _is_flac(slot, len(data)) and not _is_flac(slot, 3)
    assert not _is_flac(b"RIFF1234WAVE") and not _is_flac(np.frombuffer(id3 + b"fLaC", np.uint8), 16)
