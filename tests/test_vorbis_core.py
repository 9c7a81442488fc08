"""The device Vorbis decoder's core (csrc/aa_vorbis_core.h) as host loops --
aa_vorbis_decode_packets_host: the same unpack, inverse MDCT restatement and
overlap-add the kernels run, over the same flattened setup -- held to the host
decoder aa_vorbis_decode BIT FOR BIT (floats compared as uint32, NaNs
included), over the stream table and the 200 seeded damaged streams of
tests/vorbis_cases.py.  No stream is skipped or excused."""
import numpy as np
import pytest

import vorbis_cases as vc
from aa_amd import _lib, vorbis_gpu as vg
from oracle import vorbis_oracle as vo


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _check(name, data, ix=None):
    ix = ix or vg.index(data)
    ref, ch, sr, _ = vc.oracle(data)
    f32, s16, status = vg.decode_packets_host(ix.payload, ix.packets, ix.stream, ix.setup)
    assert (status == _lib.AA_VORBIS_OK).all(), name
    assert _bits_equal(f32, ref), name
    assert np.array_equal(s16, vc.to_s16(ref)), name
    return f32


@pytest.mark.parametrize("name", list(vc.accepted()))
def test_host_twin_is_the_host_decoder_bit_for_bit(name):
    _check(name, vc.table()[name])


def test_real_file_matches_the_oracle():
    data = vc.table()["real_libvorbis"]
    f32 = _check("real", data)
    ref, sr = vo.decode(data)
    assert sr == 44100 and ref.shape == (22050, 2)
    np.testing.assert_allclose(f32.reshape(-1, 2), ref, rtol=0, atol=2e-6)  # (tests/test_vorbis.py's bound)
    assert np.abs(f32).max() > 0.01


def test_fuzz_set_is_bit_equal():
    fz = vc.fuzz()
    assert len(fz) == 200
    decoded = 0
    for name, data in fz:
        rc, ix = vg.index_rc(data)
        if rc != _lib.AA_OK:  # (test_vorbis_index.py: the same code as aa_vorbis_info)
            continue
        _check(name, data, ix)
        decoded += 1
    assert decoded >= 190


def test_batch_of_mixed_setups():
    """Three streams, two distinct setups (bs 256/2048 twice, bs 64/8192):
    each file decodes to what it decodes to alone; the byte-identical setups
    are kept once."""
    tab = vc.table()
    names = ["stereo_coupled_res2", "bs64_8192", "mono_res1"]
    items = [vg.index(tab[n]) for n in names]
    assert items[0].setup.tobytes() != items[1].setup.tobytes()
    # the first stream again under another paging: the same setup packet
    items2 = [items[0], items[1], vg.index(tab["paged"])]
    for its, n_setups in ((items2, 2), (items, 3)):  # (mono_res1's setup holds another channel count)
        # staggered: a gap in front of every payload and every output
        byte_bases, out_bases, at, o = [], [], 5, 3
        for ix in its:
            byte_bases.append(at)
            out_bases.append(o)
            at += ix.payload.size + 11
            o += int(ix.stream["frames"][0]) * int(ix.stream["channels"][0]) + 7
        b = vg.concat(its, byte_bases, out_bases)
        assert b.n_setups == n_setups
        assert b.setups.size == sum(ix.setup.size for ix in its[:n_setups])
        if its is items2:
            assert int(b.streams["setup_at"][2]) == int(b.streams["setup_at"][0]) == 0
            assert int(b.streams["setup_at"][1]) == items[0].setup.size
        payload = np.full(at, 0xA5, np.uint8)
        for ix, base in zip(its, byte_bases):
            payload[base:base + ix.payload.size] = ix.payload
        f32, s16, status = vg.decode_packets_host(payload, b.packets, b.streams, b.setups, n_out=o)
        assert (status == 0).all() and len(status) == sum(len(ix.packets) for ix in its)
        covered = np.zeros(o, bool)
        for ix, ob in zip(its, out_bases):
            n = int(ix.stream["frames"][0]) * int(ix.stream["channels"][0])
            one = vg.decode_packets_host(ix.payload, ix.packets, ix.stream, ix.setup)
            assert _bits_equal(f32[ob:ob + n], one[0]) and np.array_equal(s16[ob:ob + n], one[1])
            covered[ob:ob + n] = True
        assert (f32[~covered] == 0).all() and (s16[~covered] == 0).all()  # the gaps are untouched


def test_small_slice_and_bad_table_entries_fall_back():
    """A workspace slice too small, a table entry at odds with the packet's own
    bits, a stream or setup out of range: AA_VORBIS_FALLBACK, nothing written
    outside the outputs."""
    import ctypes as C
    ix = vg.index(vc.table()["stereo_coupled_res2"])
    payload, streams = ix.payload, ix.stream
    setups = vg._aligned(ix.setup)
    L = _lib.lib()

    def run(packets, streams=streams, shrink=False, setups=setups):
        pl, nb = vg.plan(ix.packets, ix.stream)
        if shrink:
            pl.stride = int(ix.stream["ws_need"][0][0])  # a short block's need: long blocks do not fit
        n = int(streams["frames"][0] * streams["channels"][0])
        f32 = np.zeros(n, np.float32)
        status = np.full(len(packets), -1, np.int32)
        ws = np.zeros(nb // 8 + 1, np.int64)
        _lib.check(L.aa_vorbis_decode_packets_host(
            payload.ctypes.data, payload.size, packets.ctypes.data, len(packets), streams.ctypes.data, 1,
            setups.ctypes.data, setups.size, C.byref(pl), None, f32.ctypes.data, n, status.ctypes.data,
            ws.ctypes.data, ws.nbytes, None), "host")
        return status

    assert (run(ix.packets) == 0).all()
    st = run(ix.packets, shrink=True)
    assert ((st == _lib.AA_VORBIS_FALLBACK) == (ix.packets["blockflag"] == 1)).all()
    for field, value in (("n", 256), ("prev", 0), ("stream", 1), ("stream", -1), ("offset", payload.size),
                         ("nbytes", 0)):
        t = ix.packets.copy()
        k = int(np.flatnonzero(t["blockflag"] == 1)[1])
        if field == "prev":
            value = 1 - int(t["prev"][k])
        t[field][k] = value
        st = run(t)
        assert st[k] == _lib.AA_VORBIS_FALLBACK and (np.delete(st, k) == 0).all(), field
    s = streams.copy()
    s["setup_at"] = 8
    assert (run(ix.packets, streams=s) == _lib.AA_VORBIS_FALLBACK).all()
    cut = setups[:setups.size // 2 // 8 * 8]
    assert (run(ix.packets, setups=cut) == _lib.AA_VORBIS_FALLBACK).all()
