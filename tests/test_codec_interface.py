"""The interface the device codecs give the batched corpus path (aa_amd._codec:
sniff / index_slot / decode_batch / host_samples on flac_gpu, vorbis_gpu and
mp3_gpu), as far as the host alone can hold it: the workspace grouping, what
index_slot says of a file in a slot against the host decoder of the same
bytes, the staging layout of a mixed batch against each codec's host twin, and
the mode switches."""
from pathlib import Path

import numpy as np
import pytest

import flac_cases as fc
import flac_writer as fw
import mp3_cases as mc
import vorbis_cases as vc
from aa_amd import _codec, audio, batch, flac_gpu, mp3_gpu, vorbis_gpu

REAL_MP3 = Path(__file__).resolve().parent / "golden" / "mp3" / "invalid_keypress.mp3"


# ---- the grouping helper ---------------------------------------------------
@pytest.mark.parametrize("needs,cap", [([], 10), ([3], 10), ([11], 10), ([11, 1, 1], 10), ([4, 4, 4, 4], 8),
                                       ([5, 5, 1], 10), ([1, 12, 1], 10), ([10, 10, 10], 10), ([0, 0, 0], 0),
                                       ([3, 9, 2, 2, 2, 7, 30, 1], 9)])
def test_groups_under(needs, cap):
    groups = _codec.groups_under(needs, cap)
    assert [k for g in groups for k in g] == list(range(len(needs)))  # back to range(n): consecutive, in order
    for g in groups:
        assert g and g == list(range(g[0], g[-1] + 1))
        assert len(g) == 1 or sum(needs[k] for k in g) <= cap
    # greedy: a group ends only where the next file would not have fitted
    for a, b in zip(groups, groups[1:]):
        assert sum(needs[k] for k in a) + needs[b[0]] > cap
    if needs == [11, 1, 1]:
        assert groups == [[0], [1, 2]]  # the first alone exceeds the cap and goes alone
    if not needs:
        assert groups == []


# ---- index_slot against the host decoder -----------------------------------
def _slot(data, slack):
    buf = np.full(len(data) + slack, 0xEE, np.uint8)
    buf[:len(data)] = np.frombuffer(data, np.uint8)
    return buf


def _host(decode, data):
    """(frames, channels, rate) of the host decoder, or None where it refuses the stream"""
    try:
        x, ch, sr = decode(data)
    except Exception:
        return None
    return len(x) // ch, ch, sr


def _check_slot(mod, decode, data, name, slack=4096):
    buf = _slot(data, slack)
    s = mod.index_slot(buf, len(data))
    want = _host(decode, data)
    if want is None or want[0] == 0:
        assert s is None, name
    elif s is not None:
        assert (s.n_in, s.channels, s.sr_in) == want, name
    return s, buf


def test_index_slot_flac():
    for name, data, _ in fc.table():
        assert flac_gpu.sniff(_slot(data, 64), len(data)) and not vorbis_gpu.sniff(_slot(data, 64), len(data))
        s, buf = _check_slot(flac_gpu, audio.decode_flac, data, name)
        assert s is not None and s.payload_bytes == len(data), name  # the file stays in its slot as it is
        assert buf[:len(data)].tobytes() == data and s.index.tobytes() == flac_gpu.index(data)[1].tobytes()
    rng = np.random.default_rng(6)
    none = [fw.stream([], 48000, 1, 16, 0, 16),                                          # no frames
            fc.make_stream(rng, 12, [fc.KINDS[2]], channels=8, block=4608, n_frames=1)[0]]  # fits_batch says no
    none += [bad for _, mode, bad, _, _ in fc.fuzz()[::10] if mode != "restamp"]          # the index refuses
    for k, data in enumerate(none):
        assert _check_slot(flac_gpu, audio.decode_flac, data, k)[0] is None, k


def test_index_slot_vorbis():
    for name, data in vc.table().items():
        assert vorbis_gpu.sniff(_slot(data, 64), len(data)) and not flac_gpu.sniff(_slot(data, 64), len(data))
        s, buf = _check_slot(vorbis_gpu, audio.decode_vorbis, data, name)
        if name == vc.FLOOR0:  # (the host decodes it; the device path declines it)
            assert s is None
            continue
        ix = vorbis_gpu.index(data)
        assert s is not None and s.payload_bytes == ix.payload.size, name
        # the payload went over the head of the slot, and nothing behind the file was touched
        assert buf[:s.payload_bytes].tobytes() == ix.payload.tobytes() and (buf[len(data):] == 0xEE).all(), name
        assert s.index.payload.ctypes.data == buf.ctypes.data and (s.index.packets == ix.packets).all(), name
    for name, data in vc.fuzz()[::7]:
        _check_slot(vorbis_gpu, audio.decode_vorbis, data, name)
    assert not vorbis_gpu.sniff(_slot(b"Ogg", 64), 3)


def test_index_slot_mp3():
    cases = [(n, mc.case(n)["data"]) for n in mc.NAMES] + [("real", REAL_MP3.read_bytes())]
    for name, data in cases:
        assert mp3_gpu.sniff(_slot(data, 64), len(data)) and not vorbis_gpu.sniff(_slot(data, 64), len(data))
        s, buf = _check_slot(mp3_gpu, audio.decode_mp3, data, name)
        ix = mp3_gpu.index(data)
        assert s is not None and s.payload_bytes == ix.payload.size, name
        assert buf[:s.payload_bytes].tobytes() == ix.payload.tobytes() and (buf[len(data):] == 0xEE).all(), name
        assert s.index.payload.ctypes.data == buf.ctypes.data and (s.index.frames == ix.frames).all(), name
    for name, data in mc.fuzz()[::7]:
        _check_slot(mp3_gpu, audio.decode_mp3, data, name)
    mpeg2 = (bytes([0xFF, 0xE0 | (2 << 3) | (1 << 1) | 1, 9 << 4, 0]) + bytes(413)) * 4
    assert mp3_gpu.sniff(_slot(mpeg2, 64), len(mpeg2)) and _check_slot(mp3_gpu, audio.decode_mp3, mpeg2, "mpeg2")[0] is None


# ---- the staging layout against the host twins -----------------------------
def _twin(mod, comp, items, byte_bases, out_bases, n_out):
    """(s16, status) of the codec's host twin over a batch laid out like decode_batch's"""
    b = mod.concat(items, byte_bases, out_bases)
    if mod is flac_gpu:
        _, s16, st = mod.decode_frames_host(comp, b, want_i32=False, n_out=n_out)
    elif mod is vorbis_gpu:
        _, s16, st = mod.decode_packets_host(comp, b.packets, b.streams, b.setups, want_f32=False, n_out=n_out)
    else:
        _, s16, st = mod.decode_frames_host(comp, b.frames, b.streams, want_f32=False, n_out=n_out)
    return s16, st


def test_layout_places_every_file_where_its_twin_decodes_it():
    tab = {n: d for n, d, _ in fc.table()}
    streams = [(flac_gpu, tab[n]) for n in ("b16_mid_side", "block576", "b24_indep", "ch3")]
    streams += [(vorbis_gpu, vc.table()[n]) for n in ("mono_res1", "stereo_coupled_res2", "trim", "real_libvorbis")]
    streams += [(mp3_gpu, mc.case(n)["data"]) for n in ("mono_long", "stereo_ms_blocks", "mixed_48k")]
    streams.append((mp3_gpu, REAL_MP3.read_bytes()))
    order = np.random.default_rng(12).permutation(len(streams) + 2).tolist()  # formats and sizes shuffled
    decs, slots = [], []
    for k in order:
        if k >= len(streams):  # a PCM16 file and a host-decoded one between them hold their places too
            n = 300 + k
            decs.append(batch.Decoded(n=n, sr=48000, s16=np.arange(2 * n, dtype=np.int16), channels=2) if k & 1 else
                        batch.Decoded(n=n, sr=48000, f32=np.zeros(n, np.float32)))
            slots.append(None)
            continue
        mod, data = streams[k]
        buf = _slot(data, 512)
        s = mod.index_slot(buf, len(data))
        decs.append(batch.Decoded(n=s.n_in, sr=48000, channels=s.channels, sr_in=s.sr_in, codec=mod, index=s.index,
                                  nbytes=s.payload_bytes, n_in=s.n_in))
        slots.append(buf)
    places, total, n16, nc = batch.staging_layout(decs)
    assert total == sum(d.n for d in decs) and [p[0] for p in places] == np.cumsum([0] + [d.n for d in decs])[:-1].tolist()
    # the int16 and byte regions: back to back in batch order, so none overlaps another
    at16 = atc = 0
    comp = np.zeros(nc, np.uint8)
    for d, buf, (_, o16, oc) in zip(decs, slots, places):
        if d.codec is None and d.s16 is None:
            assert o16 is None and oc is None
            continue
        assert o16 == at16 and oc == (atc if d.codec is not None else None)
        at16 += d.n_in * d.channels if d.codec is not None else d.s16.size
        if d.codec is not None:
            comp[oc:oc + d.nbytes] = buf[:d.nbytes]
            atc += d.nbytes
    assert (at16, atc) == (n16, nc)
    shared = np.zeros(n16, np.int16)
    for mod in (flac_gpu, vorbis_gpu, mp3_gpu):
        mine = [(d, p) for d, p in zip(decs, places) if d.codec is mod]
        assert len(mine) == 4
        s16, st = _twin(mod, comp, [d.index for d, _ in mine], [p[2] for _, p in mine], [p[1] for _, p in mine], n16)
        assert not st.any()
        inside = np.zeros(n16, bool)
        for d, (_, o16, _) in mine:
            inside[o16:o16 + d.n_in * d.channels] = True
        assert not s16[~inside].any()  # the twin wrote into its own files' places only
        shared[inside] = s16[inside]
    for k, d, (_, o16, _) in zip(order, decs, places):
        if d.codec is None:
            continue
        mod, data = streams[k]
        alone = mod.index_slot(_slot(data, 512), len(data)).index
        one, st = _twin(mod, _slot(data, 512) if mod is flac_gpu else alone.payload, [alone], [0], [0], None)
        assert not st.any() and len(one) == d.n_in * d.channels
        np.testing.assert_array_equal(shared[o16:o16 + len(one)], one, err_msg=str(k))


# ---- the mode switches -----------------------------------------------------
def test_mp3_mode(monkeypatch):
    monkeypatch.delenv("AA_MP3", raising=False)
    assert batch.mp3_mode() == "host"  # the default
    assert batch.mp3_mode("gpu") == "gpu" and batch.mp3_mode("host") == "host"
    monkeypatch.setenv("AA_MP3", "gpu")
    assert batch.mp3_mode() == "gpu" and batch.mp3_mode("host") == "host"
    for bad in ("cpu", "GPU", "1", "fpga"):
        with pytest.raises(ValueError):
            batch.mp3_mode(bad)
    monkeypatch.setenv("AA_MP3", "device")
    with pytest.raises(ValueError):
        batch.mp3_mode()


def test_codecs_table(monkeypatch):
    assert [(n, m, e, d) for n, m, e, d in batch.CODECS] == [("flac", flac_gpu, "AA_FLAC", "gpu"),
                                                            ("vorbis", vorbis_gpu, "AA_VORBIS", "host"),
                                                            ("mp3", mp3_gpu, "AA_MP3", "host")]
    for name, mod, env, default in batch.CODECS:
        monkeypatch.delenv(env, raising=False)
        assert batch.codec_mode(name) == default and batch.codec_mode(name, "gpu") == "gpu"
        assert all(callable(getattr(mod, f)) for f in ("sniff", "index_slot", "decode_batch", "host_samples"))
    with pytest.raises(ValueError, match="flac='fpga': \"host\" or \"gpu\""):
        batch.codec_mode("flac", "fpga")
