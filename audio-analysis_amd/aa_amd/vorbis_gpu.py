"""Ogg Vorbis decode on the device (csrc/aa_vorbis_gpu.hip).

The host indexes a stream (``index``: pages walked and CRC-checked, packets
reassembled, the block timeline laid out from each packet's mode bits, the
setup header flattened into one blob -- nothing of the audio decoded), the
packet payloads cross PCIe, and one ``aa_vorbis_decode_device`` call (unpack,
inverse MDCT + window, overlap-add + float -> s16) decodes every packet of
every stream of a batch into ffmpeg's s16 integers -- the corpus path's int16
staging buffer, which ``aa_pcm_s16_to_f32`` widens exactly as for a PCM16 WAV.
The decoder core is held to the host decoder (``aa_vorbis_decode``) bit for
bit; what it declines (a floor of type 0, more than 8 channels) ``index``
refuses, and a packet the device does not vouch for comes back as a status:
the file is then decoded on the host, so its samples -- or its error -- are
the host route's.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._codec import groups_under, read_bytes, reread_samples as host_samples, slot_stream, to_device, u8 as _u8

WG = _lib.AA_VORBIS_WG  # packets one unpack workgroup takes
PACKET = np.dtype([("offset", "<i8"), ("pos", "<i8"), ("blk_at", "<i8"), ("nbytes", "<i4"), ("n", "<i4"),
                   ("blockflag", "<i4"), ("prev", "<i4"), ("next", "<i4"), ("lstart", "<i4"), ("rend", "<i4"),
                   ("stream", "<i4")])
STREAM = np.dtype([("setup_at", "<i8"), ("out_at", "<i8"), ("frames", "<i8"), ("s0", "<i8"), ("first_packet", "<i8"),
                   ("n_packets", "<i8"), ("channels", "<i4"), ("sample_rate", "<i4"), ("blocksize_0", "<i4"),
                   ("blocksize_1", "<i4"), ("ws_need", "<i4", (2,))])
assert PACKET.itemsize == C.sizeof(_lib.VorbisPacket) and STREAM.itemsize == C.sizeof(_lib.VorbisStream)

# One indexed stream: ``stream`` a STREAM array of one record, ``packets`` its
# PACKET table, ``payload`` the packets' bytes (uint8), ``setup`` the flattened
# setup (uint8, a multiple of 8 bytes).
Indexed = namedtuple("Indexed", "stream packets payload setup")
# A batch: the concatenated packet table, the stream records, the distinct
# setups back to back, and how many distinct setups there are.
Batch = namedtuple("Batch", "packets streams setups n_setups")

_GUESS = {"setup": 1 << 20}  # bytes a flattened setup has needed so far (grow-only)


def index_rc(data, payload=None):
    """(return code of aa_vorbis_index, Indexed or None).  payload: a uint8
    buffer to take the packet bytes (it may be the buffer holding ``data``:
    every packet is read before the first is written); None: a fresh one."""
    buf = _u8(data)
    L = _lib.lib()
    st = np.zeros(1, STREAM)
    pb, sb = C.c_int64(), C.c_int64()
    pay = np.empty(max(buf.size, 1), np.uint8) if payload is None else payload
    tab = np.zeros(max(64, buf.size // 32), PACKET)
    setup = np.empty(_GUESS["setup"] // 8, np.int64)
    for _ in range(2):
        rc = L.aa_vorbis_index(buf.ctypes.data, buf.size, st.ctypes.data_as(C.POINTER(_lib.VorbisStream)),
                               pay.ctypes.data, pay.size, C.byref(pb), tab.ctypes.data, len(tab), setup.ctypes.data,
                               setup.nbytes, C.byref(sb))
        if rc != _lib.AA_ERR_WORKSPACE:
            break
        if int(st["n_packets"][0]) > len(tab):
            tab = np.zeros(int(st["n_packets"][0]), PACKET)
        if sb.value > setup.nbytes:
            _GUESS["setup"] = max(_GUESS["setup"], int(sb.value))
            setup = np.empty(sb.value // 8, np.int64)
        if pb.value > pay.size:  # (only a caller's short buffer)
            pay = np.empty(pb.value, np.uint8)
    if rc != _lib.AA_OK:
        return rc, None
    return rc, Indexed(st, tab[:int(st["n_packets"][0])].copy(), pay[:pb.value],
                       setup[:sb.value // 8].copy().view(np.uint8))


def index(data, payload=None):
    """Indexed of an Ogg Vorbis stream's bytes, or None when the stream is not
    indexable or is one the device path declines (then ``audio.decode_vorbis``
    gives its samples or its error)."""
    return index_rc(data, payload)[1]


# As for FLAC (flac_gpu.MAX_FRAME_SAMPLES): a batch's unpack workspace is its
# packet count times the LARGEST need of any of its packets, so one file of
# huge multichannel blocks (or of a setup with an outsize classification
# buffer) would inflate every packet's slice.  Above this many samples per
# block (8192 x 4 channels; the slice is twice that in floats plus the
# classifications) a file takes the host route.
MAX_BLOCK_SAMPLES = 32768


def fits_batch(ix) -> bool:
    """Whether the corpus path decodes this file's packets on the device."""
    s = ix.stream[0]
    return (int(s["blocksize_1"]) * int(s["channels"]) <= MAX_BLOCK_SAMPLES and
            int(s["ws_need"].max()) <= 4 * MAX_BLOCK_SAMPLES)


def concat(items, byte_bases, out_bases) -> Batch:
    """One batch of Indexed streams: stream k's packets at byte_bases[k] of
    the concatenated payloads, its frames written from element out_bases[k].
    Byte-identical setups (files of one encoder) are kept once."""
    packets, streams, setups, seen = [], [], [], {}
    first = blk = at = 0
    for k, (ix, b, o) in enumerate(zip(items, byte_bases, out_bases)):
        t, s = ix.packets.copy(), ix.stream.copy()
        t["offset"] += b
        t["blk_at"] += blk
        t["stream"] = k
        key = ix.setup.tobytes()
        if key not in seen:
            seen[key] = at
            setups.append(ix.setup)
            at += ix.setup.size
        s["setup_at"], s["out_at"], s["first_packet"] = seen[key], o, first
        first += len(t)
        blk += int(t["n"].astype(np.int64).sum()) * int(s["channels"][0])
        packets.append(t)
        streams.append(s)
    return Batch(np.concatenate(packets) if packets else np.zeros(0, PACKET),
                 np.concatenate(streams) if streams else np.zeros(0, STREAM),
                 np.concatenate(setups) if setups else np.zeros(0, np.uint8), len(seen))


def plan(packets, streams):
    """(VorbisPlan, workspace bytes) of one decode call over these tables."""
    packets, streams = np.ascontiguousarray(packets), np.ascontiguousarray(streams)
    pl = _lib.VorbisPlan()
    n = _lib.lib().aa_vorbis_device_workspace_bytes(packets.ctypes.data, len(packets), streams.ctypes.data,
                                                    len(streams), C.byref(pl))
    return pl, int(n)


def workspace_bytes(packets, streams) -> int:
    return plan(packets, streams)[1]


def _aligned(a):
    """a uint8 array's bytes at an 8-byte aligned address"""
    out = np.empty((a.size + 7) // 8, np.int64).view(np.uint8)[:a.size]
    out[:] = a
    return out


def decode_packets_host(payload, packets, streams, setups, want_f32=True, want_s16=True, n_out=None):
    """The core as host loops (aa_vorbis_decode_packets_host): (f32, s16, status)."""
    buf, packets, streams = _u8(payload), np.ascontiguousarray(packets), np.ascontiguousarray(streams)
    setups = _aligned(_u8(setups))
    if n_out is None:
        n_out = int((streams["out_at"] + streams["frames"] * streams["channels"]).max()) if len(streams) else 0
    f32 = np.zeros(n_out, np.float32) if want_f32 else None
    s16 = np.zeros(n_out, np.int16) if want_s16 else None
    status = np.full(len(packets), -1, np.int32)
    pl, nb = plan(packets, streams)
    ws = np.zeros(max(nb // 8, 1), np.int64)
    _lib.check(_lib.lib().aa_vorbis_decode_packets_host(
        buf.ctypes.data, buf.size, packets.ctypes.data, len(packets), streams.ctypes.data, len(streams),
        setups.ctypes.data, setups.size, C.byref(pl), s16.ctypes.data if want_s16 else None,
        f32.ctypes.data if want_f32 else None, n_out, status.ctypes.data, ws.ctypes.data, ws.nbytes, None),
        "aa_vorbis_decode_packets_host")
    return f32, s16, status


def decode_device(bytes_dev, packets_dev, n_packets, streams_dev, n_streams, setups_dev, pl, status_dev, ws,
                  out_s16=None, out_f32=None, out_elems=None, stream=None):
    """One aa_vorbis_decode_device call over device tensors (no synchronisation).
    pl: the host VorbisPlan of ``plan``; out_elems: elements the outputs hold."""
    if out_elems is None:
        out_elems = min(t.numel() for t in (out_s16, out_f32) if t is not None)
    _lib.check(_lib.lib().aa_vorbis_decode_device(
        _lib.dptr(bytes_dev), bytes_dev.numel(), _lib.dptr(packets_dev), int(n_packets), _lib.dptr(streams_dev),
        int(n_streams), _lib.dptr(setups_dev), setups_dev.numel() * setups_dev.element_size(), C.byref(pl),
        _lib.dptr(out_s16), _lib.dptr(out_f32), int(out_elems), _lib.dptr(status_dev), _lib.dptr(ws),
        ws.numel() * ws.element_size(), _lib.stream_ptr(stream)), "aa_vorbis_decode_device")


WS_BYTES = 1 << 30  # workspace one aa_vorbis_decode_device call of a batch may take


def sniff(buf, size) -> bool:
    return size >= 4 and bytes(buf[:4]) == b"OggS"


def index_slot(buf, size):
    """Slotted of the Ogg Vorbis file in buf[:size], whose packet bytes the
    index writes over the head of buf, or None (_codec.slot_stream)."""
    return slot_stream(index(buf[:size], payload=buf), fits_batch)


def decode_batch(scratch, items, byte_bases, out_bases, comp, s16, device, stream):
    """aa_vorbis_decode_device over the Indexed ``items`` (file k's packet bytes
    at comp[byte_bases[k]:], its samples into s16[out_bases[k]:]), in as many
    calls as keep one call's workspace under WS_BYTES (a file alone may exceed
    it); after each the per-packet statuses, read back before any sample is
    used: the positions of the files with a packet not OK."""
    bad = []
    for g in groups_under([workspace_bytes(ix.packets, ix.stream) for ix in items], WS_BYTES):
        b = concat([items[k] for k in g], [byte_bases[k] for k in g], [out_bases[k] for k in g])
        if not len(b.packets):
            continue
        pl, nb = plan(b.packets, b.streams)
        status = scratch("status", len(b.packets), torch.int32)[:len(b.packets)]
        ws = scratch("vorbis_ws", max(nb // 8, 1), torch.int64)
        decode_device(comp, to_device(b.packets, device), len(b.packets), to_device(b.streams, device),
                      len(b.streams), to_device(b.setups, device), pl, status, ws, out_s16=s16,
                      out_elems=s16.numel(), stream=stream)
        st = status.cpu().numpy()  # (orders the decode before the next group reuses the workspace, too)
        bad += [g[k] for k in sorted(set(b.packets["stream"][st != _lib.AA_VORBIS_OK].tolist()))]
    return bad


def _host_route(data, device):
    from .audio import _float_to_s16, _to_mono, decode_vorbis
    f, channels, sr = decode_vorbis(bytes(data))
    return torch.from_numpy(_to_mono(_float_to_s16(f), channels)).to(device), int(sr)


def decode_to_device(data_or_path, device=None):
    """An Ogg Vorbis file (path or bytes) -> (mono float32 PCM on the device at
    the file's own rate, sample rate): the samples ``audio.decode`` gives,
    decoded on the device.  A stream the index declines, or any packet the
    device does not vouch for, sends the whole file through
    ``audio.decode_vorbis`` (its samples, or its exception)."""
    device = torch.device(device or "cuda")
    data = read_bytes(data_or_path)
    ix = index(data)
    if ix is None:
        return _host_route(data, device)
    st = ix.stream[0]
    n, ch, sr = int(st["frames"]), int(st["channels"]), int(st["sample_rate"])
    if n == 0:
        return torch.empty(0, dtype=torch.float32, device=device), sr
    pl, nb = plan(ix.packets, ix.stream)
    comp = torch.from_numpy(ix.payload.copy()).to(device)
    s16 = torch.empty(n * ch, dtype=torch.int16, device=device)
    status = torch.empty(len(ix.packets), dtype=torch.int32, device=device)
    ws = torch.empty(max(nb // 8, 1), dtype=torch.int64, device=device)
    decode_device(comp, to_device(ix.packets, device), len(ix.packets), to_device(ix.stream, device), 1,
                  to_device(ix.setup, device), pl, status, ws, out_s16=s16)
    if int(status.count_nonzero()):  # (the readback orders the decode before any use of s16)
        return _host_route(data, device)
    pcm = torch.empty(n, dtype=torch.float32, device=device)
    _lib.check(_lib.lib().aa_pcm_s16_to_f32(_lib.dptr(s16), n, ch, _lib.dptr(pcm), _lib.stream_ptr()),
               "aa_pcm_s16_to_f32")
    return pcm, sr
