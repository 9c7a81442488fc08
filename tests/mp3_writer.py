"""An MPEG-1 Layer III bitstream writer for the tests (not an encoder): it
takes side info, scalefactors and the quantised values is[576] of every granule
and emits frames -- headers, optional CRC word, side info, and the main data
placed through the bit reservoir.  The Huffman code words, linbits, slen and
band edges are read from the library's own single copy (aa_mp3_table).

A granule is a dict:
  block_type 0..3, mixed, global_gain, scalefac_compress, scalefac_scale,
  preflag, subblock_gain [3], table_select [3], region0_count, region1_count,
  count1table_select, big_values (pairs), sfl [21] long scalefactors, sfs
  [12][3] short ones, is [576] ints (bitstream order), and optionally
  `override` {side-info field: value written instead of the true one}.
A frame is a dict: gr [2][channels] granules, scfsi [channels] (4-bit masks,
band group 0 in bit 3), ms, bitrate_index, padding, crc, max_back (bytes of
reservoir the frame may reach back), force_mdb (main_data_begin written
regardless of where the data lies).
"""
import ctypes as C

import numpy as np

from aa_amd import _lib

KBPS = (0, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320)
RATES = (44100, 48000, 32000)


def table(kind, index=0):
    out = np.zeros(512, np.int32)
    n = C.c_int64()
    _lib.check(_lib.lib().aa_mp3_table(kind, index, out.ctypes.data, out.size, C.byref(n)), "aa_mp3_table")
    return out[:n.value].copy()


_CACHE = {}


def tables():
    if not _CACHE:
        _CACHE["linbits"] = table(2)
        _CACHE["slen"] = (table(3, 0), table(3, 1))
        _CACHE["pretab"] = table(4)
        _CACHE["sfb_long"] = [table(5, i) for i in range(3)]
        _CACHE["sfb_short"] = [table(6, i) for i in range(3)]
        _CACHE["huff"] = {t: (table(0, t), table(1, t)) for t in list(range(1, 34)) if t not in (4, 14)}
    return _CACHE


def dim(t):
    return int(round(len(tables()["huff"][t][0]) ** 0.5))


class Bits:
    def __init__(self):
        self.b = []

    def put(self, v, n):
        v = int(v)
        assert 0 <= v < (1 << n) or n == 0, (v, n)
        self.b.extend((v >> (n - 1 - i)) & 1 for i in range(n))

    def bytes(self):
        b = self.b + [0] * (-len(self.b) % 8)
        return bytes(np.packbits(np.array(b, np.uint8)).tolist()) if b else b""


def regions(g, sr_index):
    """(region1 start, region2 start) in lines"""
    if g["block_type"] != 0:
        return 36, 576
    sl = tables()["sfb_long"][sr_index]
    return int(sl[min(g["region0_count"] + 1, 22)]), int(sl[min(g["region0_count"] + g["region1_count"] + 2, 22)])


def granule_bits(g, sr_index, gr, scfsi):
    """The granule's part2 + part3 bits."""
    T = tables()
    w = Bits()
    s1, s2 = int(T["slen"][0][g["scalefac_compress"]]), int(T["slen"][1][g["scalefac_compress"]])
    if g["block_type"] == 2:
        if g["mixed"]:
            for s in range(8):
                w.put(g["sfl"][s], s1)
        for s in range(3 if g["mixed"] else 0, 12):
            for k in range(3):
                w.put(g["sfs"][s][k], s1 if s < 6 else s2)
    else:
        for s in range(21):
            grp = 8 if s < 6 else 4 if s < 11 else 2 if s < 16 else 1
            if gr == 1 and scfsi & grp:
                continue
            w.put(g["sfl"][s], s1 if s < 11 else s2)
    r1, r2 = regions(g, sr_index)
    q = [int(v) for v in g["is"]]
    bv = 2 * g["big_values"]
    for i in range(0, bv, 2):
        t = g["table_select"][0 if i < r1 else 1 if i < r2 else 2]
        x, y = q[i], q[i + 1]
        if t == 0:
            assert x == 0 and y == 0
            continue
        code, ln = T["huff"][t]
        lb, d = int(T["linbits"][t]), dim(t)
        ax, ay = min(abs(x), 15) if lb else abs(x), min(abs(y), 15) if lb else abs(y)
        assert ax < d and ay < d, (t, x, y)
        w.put(code[ax * d + ay], int(ln[ax * d + ay]))
        if lb and ax == 15:
            w.put(abs(x) - 15, lb)
        if x:
            w.put(x < 0, 1)
        if lb and ay == 15:
            w.put(abs(y) - 15, lb)
        if y:
            w.put(y < 0, 1)
    last = max([i for i in range(576) if q[i]] + [-1]) + 1
    code, ln = T["huff"][33 if g["count1table_select"] else 32]
    i = bv
    while i < last:
        assert i + 4 <= 576 and all(abs(v) <= 1 for v in q[i:i + 4]), i
        k = sum((1 if q[i + j] else 0) << (3 - j) for j in range(4))
        w.put(code[k], int(ln[k]))
        for j in range(4):
            if q[i + j]:
                w.put(q[i + j] < 0, 1)
        i += 4
    w.b.extend([0] * g.get("stuffing", 0))
    return w.b


def side_info(frame, channels, mdb, lengths):
    w = Bits()
    w.put(mdb, 9)
    w.put(0, 5 if channels == 1 else 3)
    for c in range(channels):
        w.put(frame["scfsi"][c], 4)
    for gr in range(2):
        for c in range(channels):
            g = dict(frame["gr"][gr][c])
            g["part2_3_length"] = lengths[gr][c]
            g.update(g.get("override", {}))
            w.put(g["part2_3_length"], 12)
            w.put(g["big_values"], 9)
            w.put(g["global_gain"], 8)
            w.put(g["scalefac_compress"], 4)
            ws = g["block_type"] != 0
            w.put(ws, 1)
            if ws:
                w.put(g["block_type"], 2)
                w.put(g["mixed"], 1)
                for r in range(2):
                    w.put(g["table_select"][r], 5)
                for k in range(3):
                    w.put(g["subblock_gain"][k], 3)
            else:
                for r in range(3):
                    w.put(g["table_select"][r], 5)
                w.put(g["region0_count"], 4)
                w.put(g["region1_count"], 3)
            w.put(g["preflag"], 1)
            w.put(g["scalefac_scale"], 1)
            w.put(g["count1table_select"], 1)
    out = w.bytes()
    assert len(out) == (17 if channels == 1 else 32)
    return out


def header(sr_index, channels, frame, mode=None):
    if mode is None:
        mode = 3 if channels == 1 else (1 if frame.get("ms") else 0)
    ext = 2 if (mode == 1 and frame.get("ms")) else 0
    b1 = 0xE0 | (3 << 3) | (1 << 1) | (0 if frame.get("crc") else 1)
    b2 = (frame["bitrate_index"] << 4) | (sr_index << 2) | (frame.get("padding", 0) << 1)
    b3 = (mode << 6) | (ext << 4)
    return bytes([0xFF, b1, b2, b3])


def frame_len(sr_index, frame):
    return 144000 * KBPS[frame["bitrate_index"]] // RATES[sr_index] + frame.get("padding", 0)


def info_frame(sr_index, channels, n_frames, delay, padding, bitrate_index=9):
    """A Xing-style "Info" frame with a LAME-style tag carrying delay and padding."""
    f = {"bitrate_index": bitrate_index, "padding": 0}
    n = frame_len(sr_index, f)
    body = bytearray(n)
    body[:4] = header(sr_index, channels, f)
    x = 4 + (17 if channels == 1 else 32)
    body[x:x + 4] = b"Info"
    body[x + 4:x + 8] = (1).to_bytes(4, "big")  # flags: the frame count follows
    body[x + 8:x + 12] = int(n_frames).to_bytes(4, "big")
    v = x + 12
    body[v:v + 9] = b"LAME3.100"
    body[v + 21:v + 24] = ((delay << 12) | padding).to_bytes(3, "big")
    return bytes(body)


def stream(frames, sr_index=0, channels=2, mode=None, id3v2=0, info=None, id3v1=False, junk=b""):
    """The stream's bytes.  id3v2: bytes of ID3v2 tag body in front (0: none);
    info: (delay, padding) for an Info frame; id3v1: a 128-byte TAG behind."""
    side = 17 if channels == 1 else 32
    datas, lengths = [], []
    for f in frames:
        w, ln = [], [[0] * channels for _ in range(2)]
        for gr in range(2):
            for c in range(channels):
                b = granule_bits(f["gr"][gr][c], sr_index, gr, f["scfsi"][c])
                ln[gr][c] = len(b)
                w += b
        bb = Bits()
        bb.b = w
        datas.append(bb.bytes())
        lengths.append(ln)
    caps = [frame_len(sr_index, f) - 4 - (2 if f.get("crc") else 0) - side for f in frames]
    flat = bytearray(sum(caps))
    write_pos, slot, out = 0, 0, bytearray()
    if id3v2:
        out += b"ID3\x04\x00\x00" + bytes([(id3v2 >> 21) & 127, (id3v2 >> 14) & 127, (id3v2 >> 7) & 127, id3v2 & 127])
        out += bytes(id3v2)
    if info is not None:
        out += info_frame(sr_index, channels, len(frames), *info)
    mdbs = []
    for f, d, cap in zip(frames, datas, caps):
        start = max(write_pos, slot - min(f.get("max_back", 0), 511))
        assert start <= slot and start + len(d) <= slot + cap, ("main data does not fit", start, slot, len(d), cap)
        flat[start:start + len(d)] = d
        mdbs.append(slot - start)
        write_pos = start + len(d)
        slot += cap
    slot = 0
    for f, ln, cap, mdb in zip(frames, lengths, caps, mdbs):
        out += header(sr_index, channels, f, mode)
        if f.get("crc"):
            out += b"\x00\x00"
        out += side_info(f, channels, f.get("force_mdb", mdb), ln)
        out += flat[slot:slot + cap]
        slot += cap
    out += junk
    if id3v1:
        out += b"TAG" + bytes(125)
    return bytes(out)
