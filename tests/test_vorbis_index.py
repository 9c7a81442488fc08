"""aa_vorbis_index (csrc/aa_vorbis.cpp, host code): the index of the device
Vorbis decoder against aa_vorbis_info / aa_vorbis_decode over the stream table
and the seeded damaged streams of tests/vorbis_cases.py, the decline-to-host
answer for floor 0, the table's geometry, and batch.vorbis_mode."""
import ctypes as C

import numpy as np
import pytest

import vorbis_cases as vc
from aa_amd import _lib, vorbis_gpu as vg


def _info(data):
    buf = np.frombuffer(data, np.uint8)
    info = _lib.VorbisInfo()
    return _lib.lib().aa_vorbis_info(buf.ctypes.data, buf.size, C.byref(info)), info


@pytest.mark.parametrize("name", list(vc.STREAMS) + list(vc.MORE) + ["real_libvorbis"])
def test_index_agrees_with_info_and_decode(name):
    data = vc.table()[name]
    rc, ix = vg.index_rc(data)
    rci, info = _info(data)
    assert rci == _lib.AA_OK
    if name == vc.FLOOR0:  # declined with the documented value, the reason in aa_last_error
        assert rc == _lib.AA_ERR_UNSUPPORTED and ix is None
        assert b"floor type 0" in _lib.lib().aa_last_error()
        assert vg.index(data) is None
        return
    assert rc == _lib.AA_OK
    s = ix.stream[0]
    assert (s["sample_rate"], s["channels"], s["blocksize_0"], s["blocksize_1"]) == (
        info.sample_rate, info.channels, info.blocksize_0, info.blocksize_1)
    ref, ch, _, _ = vc.oracle(data)
    assert int(s["frames"]) == ref.size // ch
    assert vg.fits_batch(ix)


def test_real_file_is_what_the_issue_measured():
    ix = vg.index(vc.table()["real_libvorbis"])
    s = ix.stream[0]
    assert (int(s["frames"]), int(s["channels"]), int(s["sample_rate"])) == (22050, 2, 44100)


@pytest.mark.parametrize("name", ["all_short", "bs64_8192", "trim", "paged", "two_streams", "real_libvorbis"])
def test_table_geometry(name):
    data = vc.table()[name]
    ix = vg.index(data)
    t, s = ix.packets, ix.stream[0]
    bs0, bs1, ch = int(s["blocksize_0"]), int(s["blocksize_1"]), int(s["channels"])
    assert len(t) == int(s["n_packets"]) and set(np.unique(t["n"])) <= {bs0, bs1}
    assert (t["n"] == np.where(t["blockflag"] == 1, bs1, bs0)).all()
    # payloads back to back, blocks back to back
    assert (t["offset"] == np.concatenate([[0], np.cumsum(t["nbytes"])[:-1]])).all()
    assert int(t["offset"][-1] + t["nbytes"][-1]) == ix.payload.size
    assert (t["blk_at"] == np.concatenate([[0], np.cumsum(t["n"].astype(np.int64) * ch)[:-1]])).all()
    # the timeline: p_0 = bs1, p_k+1 = p_k + 3 n_k / 4 - n_k+1 / 4
    n = t["n"].astype(np.int64)
    assert int(t["pos"][0]) == bs1 and (np.diff(t["pos"]) == 3 * n[:-1] // 4 - n[1:] // 4).all()
    # nonzero spans
    long_ = t["blockflag"] == 1
    assert (t["lstart"] == np.where(long_ & (t["prev"] == 0), n // 4 - bs0 // 4, 0)).all()
    assert (t["rend"] == np.where(long_ & (t["next"] == 0), 3 * n // 4 + bs0 // 4, n)).all()
    assert (t["prev"][~long_] == 1).all() and (t["next"][~long_] == 1).all()
    # the first output frame is at or after the first block's centre, the last before the last one's
    assert int(s["s0"]) >= int(t["pos"][0]) + int(n[0]) // 2
    assert int(s["s0"]) + int(s["frames"]) <= int(t["pos"][-1]) + int(n[-1]) // 2
    if name == "all_short":
        assert len(t) == 76
    if name == "trim":
        assert int(s["s0"]) == int(t["pos"][0]) + int(n[0]) // 2 + 300
    if name in ("paged", "two_streams"):  # the same packets as the plainly paged stream
        base = vg.index(vc.table()["stereo_coupled_res2"])
        for k in ("pos", "n", "nbytes", "prev", "next"):
            assert (base.packets[k] == t[k]).all()
        assert base.payload.tobytes() == ix.payload.tobytes()
        assert base.setup.tobytes() == ix.setup.tobytes()


def test_skipped_packets_get_no_record_and_leave_the_timeline_alone():
    """A packet whose first bit is set is no audio packet (Decoder::audio skips
    it): one byte of a stream, CRC made good again."""
    import struct
    from oracle import vorbis_oracle as vo
    data = vc.table()["all_short"]
    base = vg.index(data)
    pg = vc.pages(data)
    at, size = pg[2 + 10]  # two header pages, then one packet on a page: audio packet 10
    d = bytearray(data)
    d[at + 27 + d[at + 26]] |= 1
    d[at + 22:at + 26] = b"\0\0\0\0"
    d[at + 22:at + 26] = struct.pack("<I", vo.ogg_crc(bytes(d[at:at + size])))
    ix = vg.index(bytes(d))
    assert len(ix.packets) == len(base.packets) - 1
    assert (ix.packets["pos"] == base.packets["pos"][:-1]).all()
    ref, ch, _, _ = vc.oracle(bytes(d))
    assert int(ix.stream["frames"][0]) == ref.size // ch


def test_size_query_and_short_buffers():
    data = vc.table()["mono_res1"]
    buf = np.frombuffer(data, np.uint8)
    ix = vg.index(data)
    st = np.zeros(1, vg.STREAM)
    pb, sb = C.c_int64(), C.c_int64()
    L = _lib.lib()
    rc = L.aa_vorbis_index(buf.ctypes.data, buf.size, st.ctypes.data_as(C.POINTER(_lib.VorbisStream)), None, 0,
                           C.byref(pb), None, 0, None, 0, C.byref(sb))
    assert rc == _lib.AA_ERR_WORKSPACE
    assert (pb.value, sb.value, int(st["n_packets"][0])) == (ix.payload.size, ix.setup.size, len(ix.packets))
    assert sb.value % 8 == 0
    pay = np.full(pb.value + 16, 0xEE, np.uint8)
    tab = np.zeros(len(ix.packets) - 1, vg.PACKET)
    setup = np.zeros(sb.value // 8, np.int64)
    rc = L.aa_vorbis_index(buf.ctypes.data, buf.size, st.ctypes.data_as(C.POINTER(_lib.VorbisStream)),
                           pay.ctypes.data, pb.value, C.byref(pb), tab.ctypes.data, len(tab), setup.ctypes.data,
                           setup.nbytes, C.byref(sb))
    assert rc == _lib.AA_ERR_WORKSPACE and (pay == 0xEE).all()  # one packet short: nothing written


def test_payload_may_overwrite_the_stream_it_came_from():
    data = vc.table()["paged"]
    ix = vg.index(data)
    buf = np.frombuffer(data, np.uint8).copy()
    same = vg.index(buf, payload=buf)
    assert same.payload.tobytes() == ix.payload.tobytes() and same.payload.ctypes.data == buf.ctypes.data
    assert (same.packets == ix.packets).all()


def test_fuzz_set_return_codes_agree_with_info():
    fz = vc.fuzz()
    assert len(fz) == 200
    changed = 0
    for name, data in fz:
        rc, ix = vg.index_rc(data)
        assert rc == _info(data)[0], name
        if rc == _lib.AA_OK:
            ref, ch, _, _ = vc.oracle(data)
            assert int(ix.stream["frames"][0]) == ref.size // ch, name
            base = name.rsplit("_", 1)[0]
            changed += ix.payload.tobytes() != vg.index(vc.table()[base]).payload.tobytes()
    assert changed >= 190  # the damage reaches the packets


def test_vorbis_mode(monkeypatch):
    from aa_amd import batch
    monkeypatch.delenv("AA_VORBIS", raising=False)
    assert batch.vorbis_mode() == "host"  # the default
    assert batch.vorbis_mode("gpu") == "gpu" and batch.vorbis_mode("host") == "host"
    monkeypatch.setenv("AA_VORBIS", "gpu")
    assert batch.vorbis_mode() == "gpu" and batch.vorbis_mode("host") == "host"
    for bad in ("cpu", "GPU", "1"):
        with pytest.raises(ValueError):
            batch.vorbis_mode(bad)
    monkeypatch.setenv("AA_VORBIS", "device")
    with pytest.raises(ValueError):
        batch.vorbis_mode()
