"""Streams for the device Vorbis decoder's tests (tests/test_vorbis_index.py,
test_vorbis_core.py, test_vorbis_sanitized.py, test_gpu_vorbis.py): a table
written by the test encoder (tests/vorbis_writer.py) at 48 kHz from a short
multi-tone signal, the real libVorbis file tests/golden/vorbis/, and a seeded
set of damaged streams (bytes of audio-page bodies changed, the pages' CRCs
made good again so the damage reaches the packet decoder).  Built once per
process (lru_cache) and never modified."""
from __future__ import annotations

import ctypes as C
import struct
from functools import lru_cache
from pathlib import Path

import numpy as np

import vorbis_writer as vw
from oracle import vorbis_oracle as vo

SR = 48000
REAL = Path(__file__).resolve().parent / "golden" / "vorbis" / "invalid_keypress.ogg"
FLOOR0 = "mono_res0_floor0_short"  # the one stream of the table the device path declines

# tests/test_vorbis.py's STREAMS (copied: test modules are not imported)
STREAMS = {
    "mono_res1": dict(channels=1, kw=dict(schedule=[1, 1, 0, 0, 0, 1], residue_type=1)),
    "mono_res0_floor0_short": dict(channels=1, kw=dict(schedule=[1, 0, 0, 1, 1, 0], residue_type=0,
                                                      floor0_short=True)),
    "stereo_coupled_res2": dict(channels=2, kw=dict(schedule=[1, 0, 1, 1, 0, 0], residue_type=2)),
    "stereo_submaps_res1_res0": dict(channels=2, kw=dict(schedule=[0, 1, 1], residue_type=1, submaps=True,
                                                         coupling=False)),
    "stereo_coupled_submaps": dict(channels=2, kw=dict(schedule=[1, 1, 0], residue_type=1, submaps=True)),
}
# name: (frames, channels, encoder settings)
MORE = {
    "all_short": (9600, 1, dict(schedule=[0])),  # 76 packets: across the 64-packet workgroup edge
    "bs64_8192": (20000, 2, dict(bs=(64, 8192), schedule=[1, 0, 0, 1], residue_type=2)),  # Q = 16 and 2048
    "bs_equal": (4800, 1, dict(bs=(512, 512))),
    "one_block": (100, 1, dict()),  # 2 packets, output shorter than a block
    "trim": (9600, 2, dict(start_trim=300, residue_type=0, coupling=False)),
    "silent": (9600, 2, dict(silent=(2, 3, 5))),  # unused floors
    "paged": (9600, 2, dict(schedule=[1, 0, 1, 1, 0, 0], residue_type=2, max_segs=3, per_page=4)),
    "two_streams": (9600, 2, dict(schedule=[1, 0, 1, 1, 0, 0], residue_type=2, extra_stream=True)),
}


def signal(frames, channels=1, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(frames) / SR
    out = []
    for _ in range(channels):
        f = rng.uniform(200, 6000, 3)
        x = sum(a * np.sin(2 * np.pi * fi * t + rng.uniform(0, 6)) for a, fi in zip((0.3, 0.15, 0.05), f))
        x *= np.minimum(1.0, t / 0.02)  # onset
        out.append(x + rng.normal(0, 0.002, len(t)))
    return np.stack(out, 1)


@lru_cache(maxsize=None)
def table():
    """{name: Ogg bytes}: the streams of the issue's table, the real file last"""
    out = {}
    for name, s in STREAMS.items():
        out[name] = vw.encode(signal(int(0.2 * SR), s["channels"], seed=len(name)), sr=SR, **s["kw"])
    for k, (name, (frames, ch, kw)) in enumerate(MORE.items()):
        # the paging variants carry stereo_coupled_res2's signal: the same packets, paged differently
        x = signal(frames, ch, seed=len("stereo_coupled_res2") if name in ("paged", "two_streams") else 100 + k)
        out[name] = vw.encode(x, sr=SR, **kw)
    out["real_libvorbis"] = REAL.read_bytes()
    return out


def accepted():
    """the table without the stream the device path declines"""
    return {k: v for k, v in table().items() if k != FLOOR0}


def oracle(data):
    """aa_vorbis_decode: (interleaved float32 samples, channels, sample rate, info), or the
    first failing return code"""
    from aa_amd._lib import VorbisInfo, lib
    buf = np.frombuffer(data, np.uint8)
    info, n = VorbisInfo(), C.c_int64()
    rc = lib().aa_vorbis_info(buf.ctypes.data, buf.size, C.byref(info))
    if rc:
        return rc
    rc = lib().aa_vorbis_decode(buf.ctypes.data, buf.size, None, 0, C.byref(n))
    if rc:
        return rc
    out = np.empty(max(n.value, 1) * info.channels, np.float32)
    rc = lib().aa_vorbis_decode(buf.ctypes.data, buf.size, out.ctypes.data, n.value, C.byref(n))
    if rc:
        return rc
    return out[: n.value * info.channels], info.channels, info.sample_rate, info


def to_s16(f):
    from aa_amd.audio import _float_to_s16
    return _float_to_s16(f).astype(np.int16)


def pages(data):
    """[(offset, size)] of the Ogg pages of data (every one of a writer's or libVorbis's stream is intact)"""
    out, pos = [], 0
    while pos + 27 <= len(data):
        assert data[pos:pos + 4] == b"OggS", pos
        nseg = data[pos + 26]
        size = 27 + nseg + sum(data[pos + 27:pos + 27 + nseg])
        out.append((pos, size))
        pos += size
    return out


def repeat(data, times):
    """A longer stream without a longer encode: the writer's stream (two header
    pages, then one audio packet per page) with its audio packets `times` times
    over.  Audio packets decode on their own, so the timeline simply goes on;
    the pages carry no granule (-1), so nothing is trimmed."""
    pg = [data[a:a + n] for a, n in pages(data)]
    serial = struct.unpack("<I", data[14:18])[0]
    out, seq = list(pg[:2]), 2
    audio = [(p[27:27 + p[26]], p[27 + p[26]:]) for p in pg[2:]]
    for r in range(times):
        for k, (segs, body) in enumerate(audio):
            assert segs[-1] < 255  # whole packets
            last = r == times - 1 and k == len(audio) - 1
            out.append(vw.ogg_page(serial, seq, -1, 4 if last else 0, segs, body))
            seq += 1
    return b"".join(out)


# the fuzz set's bases: one per residue type / block geometry, and the real file
FUZZ_BASES = ["mono_res1", "stereo_coupled_res2", "stereo_submaps_res1_res0", "trim", "all_short", "silent",
              "bs64_8192", "real_libvorbis"]


@lru_cache(maxsize=None)
def fuzz(per=25):
    """Seeded damage: [(name, damaged bytes)], 200 streams.  Only the bodies of
    audio pages change (the three header packets sit on the first pages; a page
    is an audio page when no header packet ends or continues on it), and each
    damaged page's CRC is rewritten."""
    out = []
    tab = table()
    for b, base in enumerate(FUZZ_BASES):
        data = tab[base]
        pg = pages(data)
        serial = data[14:18]
        # pages of the Vorbis stream, and how many packets have ended before each
        audio, ended = [], 0
        for at, size in pg:
            if data[at + 14:at + 18] != serial:
                continue
            nseg = data[at + 26]
            if ended >= 3 and not (ended == 3 and data[at + 5] & 1):
                audio.append((at, size))
            ended += sum(1 for v in data[at + 27:at + 27 + nseg] if v < 255)
        assert audio, base
        for s in range(per):
            rng = np.random.default_rng([b, s])
            d = bytearray(data)
            for _ in range(int(rng.integers(1, 4))):
                at, size = audio[int(rng.integers(len(audio)))]
                body0 = at + 27 + d[at + 26]
                for _ in range(int(rng.integers(1, 5))):
                    i = int(rng.integers(body0, at + size))
                    d[i] = (d[i] ^ (1 << int(rng.integers(8)))) if rng.integers(2) else int(rng.integers(256))
                d[at + 22:at + 26] = b"\0\0\0\0"
                d[at + 22:at + 26] = struct.pack("<I", vo.ogg_crc(bytes(d[at:at + size])))
            out.append((f"{base}_{s}", bytes(d)))
    return out
