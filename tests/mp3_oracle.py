"""MPEG-1 Layer III in numpy float64, written straight from the formulas of
ISO/IEC 11172-3 (2.4.3.4): requantisation with numpy's own power function, MS
stereo, reorder, alias reduction, the IMDCT as matrix products, overlap-add,
frequency inversion, and the polyphase synthesis with the V FIFO carried along
the stream as in the standard's flow chart.  It starts from the values a
stream was written from (tests/mp3_writer.py's frames), not from the bits, so
it shares no parsing and no arithmetic with the decoder; only the integer
tables (band edges, pretab) and the window D come from the library's single
copy, and those are held separately (tests/test_mp3_tables.py)."""
import numpy as np

import mp3_writer as mw

ALIAS_C = np.array([-0.6, -0.535, -0.33, -0.185, -0.095, -0.041, -0.0142, -0.0037])


def window(bt):
    i = np.arange(36)
    lng = np.sin(np.pi / 36 * (i + 0.5))
    if bt == 0:
        return lng
    if bt == 1:
        return np.where(i < 18, lng, np.where(i < 24, 1.0, np.where(i < 30, np.sin(np.pi / 12 * (i - 18 + 0.5)), 0.0)))
    if bt == 3:
        return np.where(i < 6, 0.0, np.where(i < 12, np.sin(np.pi / 12 * (i - 6 + 0.5)), np.where(i < 18, 1.0, lng)))
    return np.sin(np.pi / 12 * (np.arange(12) + 0.5))


def requantise(g, sr_index):
    T = mw.tables()
    sl, ss, pretab = T["sfb_long"][sr_index], T["sfb_short"][sr_index], T["pretab"]
    q = np.array(g["is"], np.float64)
    mult = 1.0 if g["scalefac_scale"] else 0.5
    xr = np.zeros(576)
    for i in range(576):
        if q[i] == 0:
            continue
        if g["block_type"] == 2 and not (g["mixed"] and i < 36):
            s = max(k for k in range(13) if 3 * ss[k] <= i)
            width = ss[s + 1] - ss[s]
            w = (i - 3 * ss[s]) // width
            sf = g["sfs"][s][w] if s < 12 else 0
            e = (g["global_gain"] - 210 - 8 * g["subblock_gain"][w]) / 4.0 - mult * sf
        else:
            s = max(k for k in range(22) if sl[k] <= i)
            sf = g["sfl"][s] if s < 21 else 0
            e = (g["global_gain"] - 210) / 4.0 - mult * (sf + (pretab[s] if g["preflag"] else 0))
        xr[i] = np.sign(q[i]) * np.abs(q[i]) ** (4.0 / 3.0) * 2.0 ** e
    return xr


def reorder(xr, g, sr_index):
    if g["block_type"] != 2:
        return xr
    ss = mw.tables()["sfb_short"][sr_index]
    out = xr.copy()
    for s in range(3 if g["mixed"] else 0, 13):
        lo, width = int(ss[s]), int(ss[s + 1] - ss[s])
        for w in range(3):
            for f in range(width):
                out[3 * (lo + f) + w] = xr[3 * lo + w * width + f]
    return out


def alias(xr, g):
    nb = (1 if g["mixed"] else 0) if g["block_type"] == 2 else 31
    cs, ca = 1 / np.sqrt(1 + ALIAS_C ** 2), ALIAS_C / np.sqrt(1 + ALIAS_C ** 2)
    x = xr.copy()
    for sb in range(1, nb + 1):
        for k in range(8):
            bu, bd = x[18 * sb - 1 - k], x[18 * sb + k]
            x[18 * sb - 1 - k] = bu * cs[k] - bd * ca[k]
            x[18 * sb + k] = bd * cs[k] + bu * ca[k]
    return x


def imdct(xr, g):
    """[32][36] windowed IMDCT outputs"""
    out = np.zeros((32, 36))
    i36, k18 = np.arange(36)[:, None], np.arange(18)[None, :]
    c36 = np.cos(np.pi / 72 * (2 * i36 + 1 + 18) * (2 * k18 + 1))
    i12, k6 = np.arange(12)[:, None], np.arange(6)[None, :]
    c12 = np.cos(np.pi / 24 * (2 * i12 + 1 + 6) * (2 * k6 + 1))
    for sb in range(32):
        bt = g["block_type"]
        if bt == 2 and g["mixed"] and sb < 2:
            bt = 0
        x = xr[18 * sb:18 * sb + 18]
        if bt != 2:
            out[sb] = (c36 @ x) * window(bt)
        else:
            for w in range(3):
                out[sb, 6 + 6 * w:18 + 6 * w] += (c12 @ x[w::3]) * window(2)
    return out


def decode(frames, sr_index, channels, silent=()):
    """float64 PCM [n_frames * 1152][channels].  silent: (frame, granule,
    channel) triples whose spectrum is zero (a frame without data, a malformed
    granule)."""
    D = mw.table(7) / 65536.0
    i64, k32 = np.arange(64)[:, None], np.arange(32)[None, :]
    N = np.cos((16 + i64) * (2 * k32 + 1) * np.pi / 64)
    prev = np.zeros((channels, 32, 18))
    V = np.zeros((channels, 1024))
    pcm = np.zeros((len(frames) * 1152, channels))
    for fi, f in enumerate(frames):
        for gr in range(2):
            xr = []
            for c in range(channels):
                g = f["gr"][gr][c]
                xr.append(np.zeros(576) if (fi, gr, c) in silent else requantise(g, sr_index))
            if channels == 2 and f.get("ms"):
                m, s = xr
                xr = [(m + s) / np.sqrt(2.0), (m - s) / np.sqrt(2.0)]
            for c in range(channels):
                g = f["gr"][gr][c]
                y = imdct(alias(reorder(xr[c], g, sr_index), g), g)
                sbs = y[:, :18] + prev[c]
                prev[c] = y[:, 18:]
                sbs[1::2, 1::2] *= -1
                for t in range(18):
                    V[c, 64:] = V[c, :-64].copy()
                    V[c, :64] = N @ sbs[:, t]
                    U = np.zeros(512)
                    for i in range(8):
                        U[i * 64:i * 64 + 32] = V[c, i * 128:i * 128 + 32]
                        U[i * 64 + 32:i * 64 + 64] = V[c, i * 128 + 96:i * 128 + 128]
                    pcm[(fi * 2 + gr) * 576 + t * 32:(fi * 2 + gr) * 576 + t * 32 + 32, c] = (U * D).reshape(16, 32).sum(0)
    return pcm
