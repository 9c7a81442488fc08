"""The MP3 stream table of the tests: short streams (3-6 frames) written by
tests/mp3_writer.py from seeded random side info, scalefactors and is[576],
covering mono and stereo, every block type, mixed blocks, scfsi, linbits
values up to 8206, the count1 region with both tables, MS stereo, every
Huffman table (10 included, which the real fixture never uses), the three
rates, the bit reservoir, padding, the CRC flag, VBR, an ID3v2 front, an Info
frame with delay and padding, an ID3v1 tail, a first frame with
main_data_begin > 0 and one malformed granule -- and 200 seeded damaged
streams.  global_gain keeps every line near 0.004 (peaks of 0.01-0.03, s16 values to about 900):
|x| < 1 with room, and low on purpose -- see tests/test_mp3_core.py on the s16 check.

case(name) -> dict(data, frames, sr_index, channels, silent, skip, n_out)
"""
import functools

import numpy as np

import mp3_writer as mw

PAIR_TABLES = [t for t in range(1, 32) if t not in (4, 14)]


def _maxv(t):
    lb = int(mw.tables()["linbits"][t])
    return 15 + (1 << lb) - 1 if lb else mw.dim(t) - 1


def granule(rng, sr_index, block_type=0, mixed=0, tabs=(1, 7, 13), big_values=40, quads=6, count1b=0, preflag=0,
            scalefac_scale=0, sbg=(0, 0, 0), compress=9, big=False):
    T = mw.tables()
    g = dict(block_type=block_type, mixed=mixed, table_select=list(tabs), big_values=big_values,
             count1table_select=count1b, preflag=preflag, scalefac_scale=scalefac_scale, subblock_gain=list(sbg),
             scalefac_compress=compress, region0_count=3, region1_count=2)
    if block_type != 0:
        g["region0_count"], g["region1_count"] = (8, 12) if block_type == 2 and not mixed else (7, 13)
    r1, r2 = mw.regions(g, sr_index)
    q = np.zeros(576, np.int64)
    for i in range(2 * big_values):
        t = tabs[0 if i < r1 else 1 if i < r2 else 2]
        if t == 0:
            continue
        m = _maxv(t)
        v = m if (big or rng.random() < 0.08) and rng.random() < 0.5 else int(rng.integers(0, min(m, 3) + 1))
        q[i] = v * (-1 if rng.random() < 0.5 else 1)
    for i in range(2 * big_values, min(2 * big_values + 4 * quads, 576)):
        q[i] = int(rng.integers(-1, 2))
    if quads and 2 * big_values + 4 * quads <= 576:
        q[2 * big_values + 4 * quads - 1] = 1
    g["is"] = q.tolist()
    s1, s2 = int(T["slen"][0][compress]), int(T["slen"][1][compress])
    g["sfl"] = [int(rng.integers(0, 1 << (s1 if s < 11 else s2))) for s in range(21)]
    g["sfs"] = [[int(rng.integers(0, 1 << (s1 if s < 6 else s2))) for _ in range(3)] for s in range(12)]
    peak = float(np.abs(q).max()) or 1.0
    g["global_gain"] = int(210 + np.floor(4 * np.log2(0.004 / peak ** (4.0 / 3.0))))
    assert 0 <= g["global_gain"] <= 255
    return g


def frame(grs, channels, scfsi=None, ms=0, bitrate_index=14, **kw):
    f = dict(gr=grs, scfsi=list(scfsi or [0] * channels), ms=ms, bitrate_index=bitrate_index)
    f.update(kw)
    # under scfsi granule 1 carries granule 0's long scalefactors
    for c in range(channels):
        for s in range(21):
            grp = 8 if s < 6 else 4 if s < 11 else 2 if s < 16 else 1
            if f["scfsi"][c] & grp and grs[1][c]["block_type"] != 2:
                grs[1][c]["sfl"][s] = grs[0][c]["sfl"][s] if grs[0][c]["block_type"] != 2 else 0
    return f


def _build(name):
    rng = np.random.default_rng(abs(hash_name(name)))
    sr_index, channels, kw, silent, skip_end = 0, 2, {}, set(), None
    if name == "mono_long":
        channels = 1
        frames = [frame([[granule(rng, 0, preflag=gr, scalefac_scale=k & 1, tabs=((1, 2, 3, 5)[k], 7, 13))] for gr in range(2)],
                        1, scfsi=[(0, 10, 15, 5)[k]]) for k in range(4)]
    elif name == "stereo_ms_blocks":
        types = [(0, 1), (2, 3), (0, 1), (2, 3)]
        frames = [frame([[granule(rng, 0, block_type=bt, tabs=(5, 9, 0), big_values=30, count1b=c, sbg=(1, 0, 3))
                          for c in range(2)] for bt in types[k]], 2, ms=1) for k in range(4)]
    elif name == "mixed_48k":
        sr_index = 1
        frames = [frame([[granule(rng, 1, block_type=2 if (k + gr) & 1 else 0, mixed=(k + gr) & 1, tabs=(6, 11, 12),
                                  big_values=50, scalefac_scale=c) for c in range(2)] for gr in range(2)], 2)
                  for k in range(3)]
    elif name == "linbits_8206":
        channels = 1
        pairs = [(16, 23), (24, 31), (19, 27)]
        frames = [frame([[granule(rng, 0, tabs=(pairs[k][gr], 15, 13), big_values=24, big=True, quads=3)]
                         for gr in range(2)], 1) for k in range(3)]
    elif name == "every_table":
        channels = 1
        tabs = PAIR_TABLES + [1, 2, 3, 5]  # 33 = 11 granules of three
        grs = [granule(rng, 0, tabs=tuple(tabs[3 * k:3 * k + 3]), big_values=36, quads=4, count1b=k & 1)
               for k in range(11)] + [granule(rng, 0, tabs=(10, 10, 10), big_values=60)]
        frames = [frame([[grs[2 * k]], [grs[2 * k + 1]]], 1) for k in range(6)]
    elif name == "reservoir_vbr_32k":
        sr_index = 2
        rates = [5, 9, 3, 12, 5]
        frames = [frame([[granule(rng, 2, tabs=(2, 3, 8), big_values=(44, 12, 50, 10, 40)[k], quads=5,
                                  block_type=(0, 1, 2, 3, 0)[k] if gr == 0 else 0) for _ in range(2)]
                         for gr in range(2)], 2, scfsi=[0, 15 if k == 3 else 0], bitrate_index=rates[k],
                        padding=k & 1, crc=k in (1, 2), max_back=511) for k in range(5)]
        kw = dict(id3v2=37, info=(576, 1000), id3v1=True, junk=b"\xff\x00junk" * 3)
    elif name == "nodata_first":
        channels = 1
        frames = [frame([[granule(rng, 0)] for _ in range(2)], 1, force_mdb=40 if k == 0 else None) for k in range(3)]
        for f in frames:
            if f["force_mdb"] is None:
                del f["force_mdb"]
        silent = {(0, 0, 0), (0, 1, 0)}
    elif name == "malformed_granule":
        frames = [frame([[granule(rng, 0, tabs=(7, 8, 9)) for _ in range(2)] for _ in range(2)], 2, ms=k & 1)
                  for k in range(3)]
        frames[1]["gr"][0][1]["override"] = {"big_values": 300}
        silent = {(1, 0, 1)}
    else:
        raise KeyError(name)
    data = mw.stream(frames, sr_index, channels, **kw)
    total = len(frames) * 1152
    skip, end = 0, total
    if "info" in kw:
        skip, end = kw["info"][0] + 529, min(total, total - kw["info"][1] + 529)
    return dict(data=data, frames=frames, sr_index=sr_index, channels=channels, silent=silent, skip=skip,
                n_out=end - skip)


def hash_name(name):
    return sum((i + 1) * b for i, b in enumerate(name.encode())) * 2654435761 % (1 << 31)


NAMES = ["mono_long", "stereo_ms_blocks", "mixed_48k", "linbits_8206", "every_table", "reservoir_vbr_32k",
         "nodata_first", "malformed_granule"]


@functools.lru_cache(maxsize=None)
def case(name):
    return _build(name)


@functools.lru_cache(maxsize=None)
def fuzz():
    """200 seeded damaged streams: (name, bytes)."""
    out = []
    rng = np.random.default_rng(20260)
    for k in range(200):
        name = NAMES[k % len(NAMES)]
        b = bytearray(case(name)["data"])
        kind = k % 4
        if kind == 0:  # flipped bits anywhere
            for _ in range(int(rng.integers(1, 12))):
                b[int(rng.integers(0, len(b)))] ^= 1 << int(rng.integers(0, 8))
        elif kind == 1:  # cut short
            del b[int(rng.integers(8, len(b))):]
        elif kind == 2:  # a run of random bytes
            at, n = int(rng.integers(0, len(b) - 64)), int(rng.integers(1, 64))
            b[at:at + n] = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        else:  # side info of one frame randomised (behind the first header found)
            at = bytes(b).find(b"\xff\xfb")
            at = max(at, 0) + 4
            b[at:at + 17] = rng.integers(0, 256, 17, dtype=np.uint8).tobytes()
        out.append((f"fuzz{k:03d}_{name}", bytes(b)))
    return out
