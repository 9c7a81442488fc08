"""The device FLAC decoder's core (csrc/aa_flac_core.h) as a host loop
(aa_flac_decode_frames_host) against the host decoder (aa_flac_decode), which
is separate code: equal sample for sample over every bitstream feature, never
falling back on a conforming stream that its int32 arithmetic holds, and on
damaged streams either the host decoder's samples or a non-OK status."""
import numpy as np
import pytest

import flac_cases as fc
from aa_amd import _lib, flac_gpu

OK, CRC, MALFORMED, FALLBACK = (_lib.AA_FLAC_OK, _lib.AA_FLAC_CRC, _lib.AA_FLAC_MALFORMED, _lib.AA_FLAC_FALLBACK)


def test_status_codes_match_the_core():
    import re
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    core = (root / "audio-analysis_amd" / "csrc" / "aa_flac_core.h").read_text()
    head = (root / "include" / "aa.h").read_text()
    for name, v in (("OK", OK), ("CRC", CRC), ("MALFORMED", MALFORMED), ("FALLBACK", FALLBACK)):
        assert re.search(rf"\bST_{name} = {v}\b", core) and re.search(rf"\bAA_FLAC_{name} = {v}\b", head)
    assert int(re.search(r"#define AA_FLAC_WG (\d+)", head).group(1)) == flac_gpu.WG


def test_equal_to_the_oracle_over_the_table():
    """Every stream of the table: all frames OK and i32 / s16 equal to the
    host decoder's -- except 32-bit streams with a side channel (33-bit
    samples), which fall back, every one of them and nothing else."""
    fell_back = 0
    for name, data, side32 in fc.table():
        q, ch, bits = fc.oracle(data)
        info, tab = flac_gpu.index(data)
        assert (info.channels, info.bits_per_sample, info.total_frames * ch) == (ch, bits, len(q)), name
        i32, s16, st = flac_gpu.decode_frames_host(data, tab)
        if side32:
            assert set(st.tolist()) <= {OK, FALLBACK}, (name, st)
            fell_back += int((st == FALLBACK).any())
            for f, s in zip(tab, st):
                if s == OK:
                    a, b = int(f["out_at"]), int(f["out_at"]) + int(f["keep"]) * ch
                    np.testing.assert_array_equal(i32[a:b], q[a:b], err_msg=name)
            continue
        assert st.tolist() == [OK] * len(tab), (name, st)
        np.testing.assert_array_equal(i32, q, err_msg=name)
        np.testing.assert_array_equal(s16, fc.to_s16(q, bits), err_msg=name)
    assert fell_back == sum(side32 for _, _, side32 in fc.table()) == 3


def test_one_output_at_a_time_and_cut_last_block():
    rng = np.random.default_rng(8)
    data, _, _ = fc.make_stream(rng, 20, [fc.KINDS[8]], "left_side", channels=2, block=192, cut=77)
    q, ch, bits = fc.oracle(data)
    _, tab = flac_gpu.index(data)
    i32, none, st = flac_gpu.decode_frames_host(data, tab, want_s16=False)
    assert none is None and not st.any()
    np.testing.assert_array_equal(i32, q)
    none, s16, st = flac_gpu.decode_frames_host(data, tab, want_i32=False)
    assert none is None and not st.any()
    np.testing.assert_array_equal(s16, fc.to_s16(q, bits))
    assert len(q) == (3 * 192 - 77) * 2


def test_bad_table_entries_are_malformed_not_followed():
    rng = np.random.default_rng(6)
    data, _, _ = fc.make_stream(rng, 16, [fc.KINDS[4]], block=192)
    _, tab = flac_gpu.index(data)
    n_out = 3 * 192
    for field, value in (("offset", len(data) - 3), ("offset", -5), ("nbytes", 1 << 30), ("nbytes", 3), ("block", 191),
                         ("block", 1 << 20), ("keep", 193), ("keep", -1), ("channels", 2), ("channels", 9),
                         ("bits", 24), ("bits", 40), ("out_at", -1)):
        t = tab.copy()
        t[field][1] = value
        i32, _, st = flac_gpu.decode_frames_host(data, t, n_out=n_out)
        assert st[1] != OK and st[0] == OK and st[2] == OK, (field, value, st)
    # a workspace smaller than the table's frames need: FALLBACK, nothing written past it
    import ctypes as C
    buf = np.frombuffer(data, np.uint8)
    ws = np.full(flac_gpu.WG * 100 + 8, 0x5A5A5A5A, np.int32)
    out = np.zeros(n_out, np.int32)
    st = np.full(3, -1, np.int32)
    _lib.check(_lib.lib().aa_flac_decode_frames_host(buf.ctypes.data, buf.size, tab.ctypes.data, 3, out.ctypes.data,
                                                     None, st.ctypes.data, ws.ctypes.data, flac_gpu.WG * 100 * 4, None))
    assert st.tolist() == [FALLBACK] * 3 and (ws[-8:] == 0x5A5A5A5A).all()


def _frame_ranges(tab, ch):
    return [(int(f["out_at"]), int(f["out_at"]) + int(f["keep"]) * ch) for f in tab]


def test_fuzz_left_broken_crc_and_truncation():
    """Bytes flipped inside one frame (its CRC-16 left as it was), or the stream
    cut: through the undamaged stream's table the damaged frame is CRC or
    MALFORMED and every other frame OK with exact samples; the indexer refuses
    the damaged stream."""
    n = 0
    for name, mode, bad, good, k in fc.fuzz():
        if mode == "restamp":
            continue
        q, ch, bits = fc.oracle(good)
        _, tab = flac_gpu.index(good)
        i32, s16, st = flac_gpu.decode_frames_host(bad, tab, n_out=len(q))
        for j, (a, b) in enumerate(_frame_ranges(tab, ch)):
            if j == k or (mode == "trunc" and j > k):
                assert st[j] in (CRC, MALFORMED), (name, j, st)
            else:
                assert st[j] == OK, (name, j, st)
                np.testing.assert_array_equal(i32[a:b], q[a:b], err_msg=name)
                np.testing.assert_array_equal(s16[a:b], fc.to_s16(q[a:b], bits), err_msg=name)
        assert flac_gpu.index(bad) is None, name
        n += 1
    assert n == 200


def test_fuzz_restamped_frames_keep_the_exactness_rule():
    """Damage with the frame's CRC-16 made good again reaches the predictors.
    Frame by frame against aa_flac_decode of the same bytes: status OK means
    the host decoder's samples.  Where the host decoder rejects the stream (at
    the damaged frame k: the others are intact), frame k must not be OK and the
    others are held to the undamaged stream's samples."""
    n = host_ok = differ = 0
    for name, mode, bad, good, k in fc.fuzz():
        if mode != "restamp":
            continue
        ref = fc.oracle(bad)
        q_good, ch, bits = fc.oracle(good)
        ix = flac_gpu.index(bad)
        tab = ix[1] if ix is not None else flac_gpu.index(good)[1]
        i32, s16, st = flac_gpu.decode_frames_host(bad, tab, n_out=len(q_good))
        assert set(st.tolist()) <= {OK, CRC, MALFORMED, FALLBACK}
        for j, (a, b) in enumerate(_frame_ranges(tab, ch)):
            if ref is None and j == k:
                assert st[j] != OK, (name, st)
                continue
            q = ref[0] if ref is not None else q_good
            if j != k:
                assert st[j] == OK, (name, j, st)
            if st[j] == OK:
                np.testing.assert_array_equal(i32[a:b], q[a:b], err_msg=name)
                np.testing.assert_array_equal(s16[a:b], fc.to_s16(q[a:b], bits), err_msg=name)
        if ref is not None:
            host_ok += 1
            differ += int(not np.array_equal(ref[0], q_good))
        n += 1
    assert n == 100
    # the set does what it is for: damage that the host decoder decodes to other samples
    assert host_ok >= 10 and differ >= 10, (host_ok, differ)


def test_mode_switch(monkeypatch):
    from aa_amd.batch import flac_mode
    monkeypatch.delenv("AA_FLAC", raising=False)
    assert flac_mode() == "gpu" and flac_mode("host") == "host"
    monkeypatch.setenv("AA_FLAC", "host")
    assert flac_mode() == "host" and flac_mode("gpu") == "gpu"
    with pytest.raises(ValueError):
        flac_mode("fpga")
