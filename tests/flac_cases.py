"""Streams for the device FLAC decoder's tests (tests/test_flac_index.py,
test_flac_core.py, test_flac_sanitized.py, test_gpu_flac.py), written by the
test encoder (tests/flac_writer.py): a table over depths, subframe kinds,
stereo modes and block sizes, and a seeded set of damaged streams.  Built once
per process (lru_cache) and never modified."""
from __future__ import annotations

import ctypes as C
from functools import lru_cache

import numpy as np

import flac_writer as fw

BITS = [8, 12, 16, 20, 24, 32]
BLOCKS = [16, 192, 576, 1000, 4096, 4608]
STEREO = ["indep", "left_side", "side_right", "mid_side"]
KINDS = [
    ("constant", {"kind": "constant"}),
    ("verbatim", {"kind": "verbatim"}),
    ("fixed0", {"kind": "fixed", "order": 0}),
    ("fixed1", {"kind": "fixed", "order": 1, "porder": 2}),
    ("fixed2", {"kind": "fixed", "order": 2, "method": 1, "porder": 3}),
    ("fixed3", {"kind": "fixed", "order": 3, "porder": 1, "escape_parts": (1,)}),
    ("fixed4", {"kind": "fixed", "order": 4}),
    ("lpc1", {"kind": "lpc", "order": 1, "prec": 5}),
    ("lpc8", {"kind": "lpc", "order": 8, "porder": 4, "escape_parts": (0, 5)}),
    ("lpc32", {"kind": "lpc", "order": 32, "prec": 14, "porder": 1, "method": 1}),
    ("wasted_fixed", {"kind": "fixed", "order": 2, "wasted": 3}),
    ("wasted_lpc", {"kind": "lpc", "order": 6, "wasted": 2, "method": 1}),
]


def signal(rng, n, bps, kind="smooth"):
    lim = (1 << (bps - 1)) - 1
    if kind == "noise":
        x = rng.integers(-lim - 1, lim + 1, n)
    else:
        t = np.arange(n)
        x = 0.6 * lim * np.sin(2 * np.pi * t * rng.uniform(0.001, 0.05)) + rng.normal(0, lim * 0.01, n)
        x = np.clip(np.round(x), -lim - 1, lim)
    return x.astype(np.int64)


def _kw(kw, bps):
    kw = dict(kw)
    if bps == 32 and kw["kind"] in ("fixed", "lpc"):
        kw["method"] = 1  # 32-bit residuals need 5-bit Rice parameters
    return kw


def _chan(rng, n, bps, name, kw):
    if name == "constant":
        return np.full(n, int(rng.integers(-(1 << (bps - 1)), 1 << (bps - 1))), np.int64)
    # noise only where every residual stays well inside int32 (RFC 9639 asks that of a stream)
    x = signal(rng, n, bps, "noise" if bps <= 24 and name in ("verbatim", "fixed0", "fixed4") else "smooth")
    w = kw.get("wasted", 0)
    return (x >> w) << w


def make_stream(rng, bps, kinds, stereo="indep", block=192, n_frames=3, channels=1, sr=48000, cut=0, total=None,
                variable=False, id3=b"", tag=False, bs_mode="table"):
    """(bytes, [frame byte strings], [channel arrays per frame]); kinds: one (name, kw) per channel"""
    frames, ref, pos = [], [], 0
    for i in range(n_frames):
        chans = [_chan(rng, block, bps, *kinds[c % len(kinds)]) for c in range(channels)]
        if stereo != "indep":  # correlated pair
            chans[1] = np.clip(chans[0] // 2 + chans[1] // 4, -(1 << (bps - 1)), (1 << (bps - 1)) - 1)
        kws = [_kw(kinds[c % len(kinds)][1], bps) for c in range(channels)]
        if stereo != "indep":  # constants do not survive decorrelation
            kws = [kw if kw["kind"] != "constant" else _kw({"kind": "fixed", "order": 1}, bps) for kw in kws]
        frames.append(fw.frame(chans, bps, sr, pos if variable else i, stereo, kws, variable=variable,
                               bs_mode=bs_mode))
        ref.append(np.stack(chans, 1))
        pos += block
    if total is None:
        total = pos - cut
    data = fw.stream(frames, sr, channels, bps, total, block, id3=id3)
    if tag:
        data += b"TAG" + b"\x00" * 125
    return data, frames, ref


@lru_cache(maxsize=None)
def table():
    """[(name, bytes, is a 32-bit stream with a side channel)]"""
    rng = np.random.default_rng(2024)
    out = []
    for bps in BITS:
        for name, kw in KINDS:
            out.append((f"b{bps}_{name}", make_stream(rng, bps, [(name, kw)])[0], False))
    for bps in (16, 24, 32):
        for st in STEREO:
            data = make_stream(rng, bps, [KINDS[4], KINDS[8]], st, channels=2, block=256)[0]
            out.append((f"b{bps}_{st}", data, bps == 32 and st != "indep"))
    for block in BLOCKS:
        kind = ("lpc8", {"kind": "lpc", "order": 8, "porder": 3}) if block >= 192 else KINDS[3]
        out.append((f"block{block}", make_stream(rng, 16, [kind], block=block)[0], False))
    for ch in range(1, 9):
        out.append((f"ch{ch}", make_stream(rng, 12, [KINDS[1], KINDS[4], KINDS[7]], channels=ch, block=64)[0], False))
    return out


def oracle(data):
    """aa_flac_decode: (interleaved int32 samples, channels, bits) or None where it errors"""
    from aa_amd._lib import FlacInfo, lib
    buf = np.frombuffer(data, np.uint8)
    info, n = FlacInfo(), C.c_int64()
    if lib().aa_flac_info(buf.ctypes.data, buf.size, C.byref(info)):
        return None
    if lib().aa_flac_decode(buf.ctypes.data, buf.size, None, 0, C.byref(n)):
        return None
    out = np.empty(max(n.value, 1) * info.channels, np.int32)
    if lib().aa_flac_decode(buf.ctypes.data, buf.size, out.ctypes.data, n.value, C.byref(n)):
        return None
    return out[: n.value * info.channels], info.channels, info.bits_per_sample


def to_s16(q, bits):
    """audio.decode_flac's conversion, as int16"""
    q = q.astype(np.int32)
    return (q << (16 - bits) if bits <= 16 else q >> (bits - 16)).astype(np.int16)


def spans(data, frames):
    """[(offset, size)] of the frames inside data (they follow the metadata back to back)"""
    at = data.index(frames[0])
    out = []
    for f in frames:
        out.append((at, len(f)))
        at += len(f)
    return out


def _bases():
    rng = np.random.default_rng(77)
    K = dict(KINDS)
    return [
        make_stream(rng, 16, [("lpc8", {"kind": "lpc", "order": 8, "porder": 2})], block=256, n_frames=4),
        make_stream(rng, 24, [("verbatim", K["verbatim"]), ("fixed3", K["fixed3"])], "mid_side", block=128,
                    n_frames=4, channels=2),
        make_stream(rng, 8, [("fixed2", {"kind": "fixed", "order": 2, "porder": 2, "escape_parts": (0, 1, 2, 3)})],
                    block=256, n_frames=4),
        make_stream(rng, 12, [("verbatim", K["verbatim"]), ("lpc1", K["lpc1"]), ("fixed4", K["fixed4"])],
                    block=64, n_frames=4, channels=3),
    ]


@lru_cache(maxsize=None)
def fuzz(per=25):
    """Seeded damage: [(name, mode, damaged bytes, undamaged bytes, damaged frame)],
    mode flip (CRC left broken), trunc, restamp (CRC-16 of the damaged frame made
    good again, so the damage reaches the predictors)."""
    out = []
    for b, (data, frames, _) in enumerate(_bases()):
        sp = spans(data, frames)
        for mode in ("flip", "trunc", "restamp"):
            for s in range(per):
                rng = np.random.default_rng([b, s, len(mode)])
                d = bytearray(data)
                k = int(rng.integers(len(frames)))
                at, size = sp[k]
                if mode == "trunc":
                    cut = int(rng.integers(sp[0][0] + 1, len(data)))
                    d = d[:cut]
                    k = next(i for i, (a, n) in enumerate(sp) if a + n > cut)
                else:
                    hdr = 6  # sync, codes, one-byte number, CRC-8: the body starts here
                    last = size - (2 if mode == "restamp" else 0)
                    for _ in range(int(rng.integers(1, 4))):
                        i = at + int(rng.integers(hdr, last))
                        d[i] ^= (1 << int(rng.integers(8))) if rng.integers(2) else int(rng.integers(1, 256))
                    if mode == "restamp":
                        d[at + size - 2:at + size] = fw.crc16(bytes(d[at:at + size - 2])).to_bytes(2, "big")
                out.append((f"base{b}_{mode}{s}", mode, bytes(d), data, k))
    return out
