"""MPEG-1 Layer III decode on the device (csrc/aa_mp3_gpu.hip).

The host indexes a stream (``index``: headers walked, side info parsed into one
record per frame, the frames' main data copied back to back so the bit
reservoir is one flat byte stream -- nothing of the audio decoded), the main
data cross PCIe, and one ``aa_mp3_decode_device`` call (unpack, hybrid, synth)
decodes every frame of every stream of a batch into ffmpeg's s16 integers --
the corpus path's int16 staging buffer, which ``aa_pcm_s16_to_f32`` widens
exactly as for a PCM16 WAV.  The device runs the host decoder's own core
(csrc/aa_mp3_core.h), so its samples are ``aa_mp3_decode``'s bit for bit for
every stream, damaged ones included: a frame or granule that cannot be decoded
is silence on both sides and a status, and no host redo exists.  What the
decoder declines (MPEG-2 / 2.5, Layers I and II, free format, intensity
stereo) ``index`` refuses.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._codec import groups_under, read_bytes, reread_samples as host_samples, slot_stream, to_device, u8 as _u8

WG = _lib.AA_MP3_WG
# side info fields: [granule * 2 + channel] (table_select / subblock_gain: three values each)
FRAME = np.dtype([("main_at", "<i8"), ("main_lo", "<i8"), ("main_end", "<i8"), ("stream", "<i4"), ("number", "<i4"),
                  ("ms", "<i4"), ("nodata", "<i4"), ("scfsi", "<i4", (2,)), ("part2_3_length", "<i4", (4,)),
                  ("big_values", "<i4", (4,)), ("global_gain", "<i4", (4,)), ("scalefac_compress", "<i4", (4,)),
                  ("window_switching", "<i4", (4,)), ("block_type", "<i4", (4,)), ("mixed", "<i4", (4,)),
                  ("table_select", "<i4", (12,)), ("subblock_gain", "<i4", (12,)), ("region0_count", "<i4", (4,)),
                  ("region1_count", "<i4", (4,)), ("preflag", "<i4", (4,)), ("scalefac_scale", "<i4", (4,)),
                  ("count1table_select", "<i4", (4,))])
STREAM = np.dtype([("out_at", "<i8"), ("frames", "<i8"), ("skip", "<i8"), ("first_frame", "<i8"),
                   ("n_frames", "<i8"), ("channels", "<i4"), ("sample_rate", "<i4"), ("sr_index", "<i4"),
                   ("reserved", "<i4")])
assert FRAME.itemsize == C.sizeof(_lib.Mp3Frame) == 336 and STREAM.itemsize == C.sizeof(_lib.Mp3Stream) == 56

# One indexed stream: ``stream`` a STREAM array of one record, ``frames`` its
# FRAME table, ``payload`` the flat main data (uint8).
Indexed = namedtuple("Indexed", "stream frames payload")
# A batch: the concatenated frame table and the stream records.
Batch = namedtuple("Batch", "frames streams")

_TABLES = {}  # device -> the table blob there


def index_rc(data, payload=None):
    """(return code of aa_mp3_index, Indexed or None).  payload: a uint8 buffer
    to take the main data (it may be the buffer holding ``data``); None: a
    fresh one."""
    buf = _u8(data)
    L = _lib.lib()
    st = np.zeros(1, STREAM)
    pb = C.c_int64()
    pay = np.empty(max(buf.size, 1), np.uint8) if payload is None else payload
    tab = np.zeros(max(16, buf.size // 96 + 1), FRAME)  # (the shortest MPEG-1 Layer III frame is 96 bytes)
    rc = L.aa_mp3_index(buf.ctypes.data, buf.size, st.ctypes.data_as(C.POINTER(_lib.Mp3Stream)), pay.ctypes.data,
                        pay.size, C.byref(pb), tab.ctypes.data, len(tab))
    if rc != _lib.AA_OK:
        return rc, None
    return rc, Indexed(st, tab[:int(st["n_frames"][0])].copy(), pay[:pb.value])


def index(data, payload=None):
    """Indexed of an MP3 stream's bytes, or None when it is not one the decoder
    takes (then ``audio.decode_mp3`` gives its error)."""
    return index_rc(data, payload)[1]


# A batch's workspace is 2.5 KB of unpack slice per frame and channel plus
# 4608 bytes of float64 subband samples per granule and channel (two channels
# held): 23 KB per frame, 54 MB per minute at 44.1 kHz.  A file above this
# many frames (about 50 minutes) takes the host route.
MAX_FRAMES = 1 << 17


def fits_batch(ix) -> bool:
    """Whether the corpus path decodes this file's frames on the device."""
    return int(ix.stream["n_frames"][0]) <= MAX_FRAMES


def concat(items, byte_bases, out_bases) -> Batch:
    """One batch of Indexed streams: stream k's main data at byte_bases[k] of
    the concatenated payloads, its frames written from element out_bases[k]."""
    frames, streams = [], []
    first = 0
    for k, (ix, b, o) in enumerate(zip(items, byte_bases, out_bases)):
        t, s = ix.frames.copy(), ix.stream.copy()
        for f in ("main_at", "main_lo", "main_end"):
            t[f] += b
        t["stream"] = k
        s["out_at"], s["first_frame"] = o, first
        first += len(t)
        frames.append(t)
        streams.append(s)
    return Batch(np.concatenate(frames) if frames else np.zeros(0, FRAME),
                 np.concatenate(streams) if streams else np.zeros(0, STREAM))


def workspace_bytes(n_frames) -> int:
    return int(_lib.lib().aa_mp3_device_workspace_bytes(int(n_frames)))


def tables_host() -> np.ndarray:
    """The decoder's table blob (aa_mp3_tables) as uint8."""
    n = C.c_int64()
    L = _lib.lib()
    rc = L.aa_mp3_tables(None, 0, C.byref(n))
    if rc != _lib.AA_ERR_WORKSPACE:
        _lib.check(rc or 1, "aa_mp3_tables")
    out = np.empty(n.value // 8, np.int64)
    _lib.check(L.aa_mp3_tables(out.ctypes.data, out.nbytes, C.byref(n)), "aa_mp3_tables")
    return out.view(np.uint8)


def tables_device(device):
    """The table blob on ``device`` (uploaded once per device)."""
    device = torch.device(device)
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    t = _TABLES.get(key)
    if t is None:
        t = _TABLES[key] = torch.from_numpy(tables_host().view(np.int64).copy()).to(device)
    return t


def decode_frames_host(payload, frames, streams, want_f32=True, want_s16=True, n_out=None, want_left=False):
    """The core as host loops (aa_mp3_decode_frames_host): (f32, s16, status
    [n_frames, 2, 2]); want_left: also, per [frame, granule, channel], the bits
    of part2_3_length left behind the granule's last value (negative: a count1
    quadruple overshot the granule and was dropped), out of the unpack slices."""
    buf, frames, streams = _u8(payload), np.ascontiguousarray(frames), np.ascontiguousarray(streams)
    if n_out is None:
        n_out = int((streams["out_at"] + streams["frames"] * streams["channels"]).max()) if len(streams) else 0
    f32 = np.zeros(n_out, np.float32) if want_f32 else None
    s16 = np.zeros(n_out, np.int16) if want_s16 else None
    status = np.full((len(frames), 2, 2), -1, np.int32)
    ws = np.zeros(max(workspace_bytes(len(frames)) // 8, 1), np.int64)
    _lib.check(_lib.lib().aa_mp3_decode_frames_host(
        buf.ctypes.data, buf.size, frames.ctypes.data, len(frames), streams.ctypes.data, len(streams),
        s16.ctypes.data if want_s16 else None, f32.ctypes.data if want_f32 else None, n_out, status.ctypes.data,
        ws.ctypes.data, ws.nbytes), "aa_mp3_decode_frames_host")
    if want_left:
        groups = (2 * len(frames) + WG - 1) // WG
        sl = ws.view(np.int16)[:groups * 1280 * WG].reshape(groups, 1280, WG)  # [group][element][lane]
        lane = np.arange(2 * len(frames))
        left = np.stack([sl[lane // WG, g * 640 + 638, lane % WG] for g in range(2)], 0)  # [gr][frame * 2 + ch]
        return f32, s16, status, left.reshape(2, len(frames), 2).transpose(1, 0, 2)
    return f32, s16, status


def decode_device(bytes_dev, frames_dev, n_frames, streams_dev, n_streams, status_dev, ws, out_s16=None,
                  out_f32=None, out_elems=None, stream=None):
    """One aa_mp3_decode_device call over device tensors (no synchronisation).
    status_dev: int32 [n_frames * 4]; out_elems: elements the outputs hold."""
    if out_elems is None:
        out_elems = min(t.numel() for t in (out_s16, out_f32) if t is not None)
    _lib.check(_lib.lib().aa_mp3_decode_device(
        _lib.dptr(tables_device(bytes_dev.device)), _lib.dptr(bytes_dev), bytes_dev.numel(), _lib.dptr(frames_dev),
        int(n_frames), _lib.dptr(streams_dev), int(n_streams), _lib.dptr(out_s16), _lib.dptr(out_f32),
        int(out_elems), _lib.dptr(status_dev), _lib.dptr(ws), ws.numel() * ws.element_size(),
        _lib.stream_ptr(stream)), "aa_mp3_decode_device")


WS_BYTES = 1 << 30  # workspace one aa_mp3_decode_device call of a batch may take (sixteen 60 s clips: about 0.86 GB)


def sniff(buf, size) -> bool:
    from .audio import _is_mp3
    return _is_mp3(buf, size)


def index_slot(buf, size):
    """Slotted of the MP3 file in buf[:size], whose flat main data the index
    writes over the head of buf, or None (_codec.slot_stream)."""
    return slot_stream(index(buf[:size], payload=buf), fits_batch)


def decode_batch(scratch, items, byte_bases, out_bases, comp, s16, device, stream):
    """aa_mp3_decode_device over the Indexed ``items`` (file k's main data at
    comp[byte_bases[k]:], its samples into s16[out_bases[k]:]), in as many calls
    as keep one call's workspace under WS_BYTES (a file alone may exceed it).
    The device runs the host decoder's core, damaged frames included (silence
    on both sides), so no status is read back and no file is in doubt: []."""
    for g in groups_under([workspace_bytes(len(ix.frames)) for ix in items], WS_BYTES):
        b = concat([items[k] for k in g], [byte_bases[k] for k in g], [out_bases[k] for k in g])
        if not len(b.frames):
            continue
        status = scratch("status", 4 * len(b.frames), torch.int32)[:4 * len(b.frames)]
        ws = scratch("mp3_ws", max(workspace_bytes(len(b.frames)) // 8, 1), torch.int64)
        decode_device(comp, to_device(b.frames, device), len(b.frames), to_device(b.streams, device),
                      len(b.streams), status, ws, out_s16=s16, out_elems=s16.numel(), stream=stream)
    return []


def decode_to_device(data_or_path, device=None):
    """An MP3 file (path or bytes) -> (mono float32 PCM on the device at the
    file's own rate, sample rate): the samples ``audio.decode`` gives, decoded
    on the device.  A stream the index declines raises as ``audio.decode_mp3``
    does."""
    device = torch.device(device or "cuda")
    data = read_bytes(data_or_path)
    rc, ix = index_rc(data)
    if ix is None:
        _lib.check(rc, "aa_mp3_index")
    st = ix.stream[0]
    n, ch, sr = int(st["frames"]), int(st["channels"]), int(st["sample_rate"])
    if n == 0:
        return torch.empty(0, dtype=torch.float32, device=device), sr
    comp = torch.from_numpy(ix.payload.copy()).to(device)
    s16 = torch.empty(n * ch, dtype=torch.int16, device=device)
    status = torch.empty(len(ix.frames) * 4, dtype=torch.int32, device=device)
    ws = torch.empty(max(workspace_bytes(len(ix.frames)) // 8, 1), dtype=torch.int64, device=device)
    decode_device(comp, to_device(ix.frames, device), len(ix.frames), to_device(ix.stream, device), 1, status, ws,
                  out_s16=s16)
    pcm = torch.empty(n, dtype=torch.float32, device=device)
    _lib.check(_lib.lib().aa_pcm_s16_to_f32(_lib.dptr(s16), n, ch, _lib.dptr(pcm), _lib.stream_ptr()),
               "aa_pcm_s16_to_f32")
    return pcm, sr
