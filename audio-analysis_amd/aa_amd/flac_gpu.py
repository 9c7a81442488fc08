"""FLAC decode on the device (csrc/aa_flac_gpu.hip).

The host finds a stream's frames (``index``: one pass over the bytes, header
CRC-8 and frame CRC-16 checked, nothing decoded), the compressed bytes cross
PCIe, and one ``aa_flac_decode_device`` launch decodes every frame of every
stream of a batch into ffmpeg's s16 integers -- the corpus path's int16
staging buffer, which ``aa_pcm_s16_to_f32`` widens exactly as for a PCM16
WAV.  The decoder core is held to the host decoder (``aa_flac_decode``)
sample for sample; whatever it does not hold (a damaged frame, arithmetic
beyond int32) comes back as a per-frame status, and the file is then decoded
on the host, so its samples -- or its error -- are the host route's.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._codec import Slotted, read_bytes, to_device as table_to_device, u8 as _u8

WG = _lib.AA_FLAC_WG  # frames one workgroup takes
FRAME = np.dtype([("offset", "<i8"), ("out_at", "<i8"), ("nbytes", "<i4"), ("block", "<i4"), ("keep", "<i4"),
                  ("channels", "<i4"), ("bits", "<i4"), ("stream", "<i4")])
assert FRAME.itemsize == C.sizeof(_lib.FlacFrame)
Info = namedtuple("Info", "sample_rate channels bits_per_sample total_frames")


def index(data):
    """(Info, frame table as a FRAME array) of a FLAC stream's bytes, or None
    when the stream is not indexable (then ``audio.decode_flac`` gives its
    samples or its error).  Info.total_frames is the table's: the samples per
    channel the frames write."""
    buf = _u8(data)
    L = _lib.lib()
    info, n = _lib.FlacInfo(), C.c_int64()
    tab = np.zeros(max(16, buf.size // 512), FRAME)
    rc = L.aa_flac_index(buf.ctypes.data, buf.size, C.byref(info), tab.ctypes.data, len(tab), C.byref(n))
    if rc == _lib.AA_ERR_WORKSPACE:
        tab = np.zeros(n.value, FRAME)
        rc = L.aa_flac_index(buf.ctypes.data, buf.size, C.byref(info), tab.ctypes.data, len(tab), C.byref(n))
    if rc != _lib.AA_OK:
        return None
    tab = tab[:n.value]
    return Info(info.sample_rate, info.channels, info.bits_per_sample, int(tab["keep"].sum())), tab


# A batch's workspace is its frame count times the LARGEST block * channels of
# any of its frames (aa_flac_device_workspace_bytes), so one file of huge
# multichannel blocks would inflate every frame's slice: above this many
# samples per frame (4096 x 8 channels, 16384 x 2; 128 KiB of workspace a
# frame) a file takes the host route.
MAX_FRAME_SAMPLES = 32768


def fits_batch(table) -> bool:
    """Whether the corpus path decodes this file's frames on the device (see
    MAX_FRAME_SAMPLES)."""
    return not len(table) or int((table["block"].astype(np.int64) * table["channels"]).max()) <= MAX_FRAME_SAMPLES


def concat(tables, byte_bases, out_bases):
    """One table for a batch: stream k's frames at byte_bases[k] of the
    concatenated bytes, writing from element out_bases[k]."""
    parts = []
    for k, (t, b, o) in enumerate(zip(tables, byte_bases, out_bases)):
        t = t.copy()
        t["offset"] += b
        t["out_at"] += o
        t["stream"] = k
        parts.append(t)
    return np.concatenate(parts) if parts else np.zeros(0, FRAME)


def workspace_bytes(table) -> int:
    table = np.ascontiguousarray(table)
    return int(_lib.lib().aa_flac_device_workspace_bytes(table.ctypes.data, len(table)))


def decode_frames_host(data, table, want_i32=True, want_s16=True, n_out=None):
    """The core as a host loop (aa_flac_decode_frames_host): (i32, s16, status)."""
    buf, table = _u8(data), np.ascontiguousarray(table)
    if n_out is None:
        n_out = int((table["out_at"] + table["keep"].astype(np.int64) * table["channels"]).max()) if len(table) else 0
    i32 = np.zeros(n_out, np.int32) if want_i32 else None
    s16 = np.zeros(n_out, np.int16) if want_s16 else None
    status = np.full(len(table), -1, np.int32)
    ws = np.zeros(max(workspace_bytes(table) // 4, 1), np.int32)
    _lib.check(_lib.lib().aa_flac_decode_frames_host(
        buf.ctypes.data, buf.size, table.ctypes.data, len(table), i32.ctypes.data if want_i32 else None,
        s16.ctypes.data if want_s16 else None, status.ctypes.data, ws.ctypes.data, ws.nbytes, None),
        "aa_flac_decode_frames_host")
    return i32, s16, status


def decode_device(bytes_dev, table_dev, n_frames, status_dev, ws, out_i32=None, out_s16=None, stream=None):
    """One aa_flac_decode_device launch over device tensors (no synchronisation)."""
    _lib.check(_lib.lib().aa_flac_decode_device(
        _lib.dptr(bytes_dev), bytes_dev.numel(), _lib.dptr(table_dev), int(n_frames), _lib.dptr(out_i32),
        _lib.dptr(out_s16), _lib.dptr(status_dev), _lib.dptr(ws), ws.numel() * ws.element_size(),
        _lib.stream_ptr(stream)), "aa_flac_decode_device")


def sniff(buf, size) -> bool:
    from .audio import _is_flac
    return _is_flac(buf, size)


def index_slot(buf, size):
    """Slotted of the FLAC file in buf[:size] (it stays there as it is), or None:
    not indexable, no frames, or frames too large for a batch (fits_batch)."""
    ix = index(buf[:size])
    if ix is None or ix[0].total_frames <= 0 or not fits_batch(ix[1]):
        return None
    info, tab = ix
    return Slotted(tab, int(size), info.total_frames, info.channels, info.sample_rate)


def decode_batch(scratch, items, byte_bases, out_bases, comp, s16, device, stream):
    """One aa_flac_decode_device over the frame tables ``items`` (file k's bytes
    at comp[byte_bases[k]:], its samples into s16[out_bases[k]:]), then the
    per-frame statuses, read back before any sample is used: the positions of
    the files with a frame not OK.  scratch(name, n, dtype): device buffers."""
    tab = concat(items, byte_bases, out_bases)
    status = scratch("status", len(tab), torch.int32)[:len(tab)]
    ws = scratch("ws", max(workspace_bytes(tab) // 4, 1), torch.int32)
    decode_device(comp, table_to_device(tab, device), len(tab), status, ws, out_s16=s16, stream=stream)
    st = status.cpu().numpy()
    return sorted(set(tab["stream"][st != _lib.AA_FLAC_OK].tolist()))


def host_samples(decoded):
    """The host decode of a Decoded's slot (the file's bytes), mono float32."""
    from .audio import _to_mono, decode_flac
    q, ch, _ = decode_flac(decoded.comp_t.numpy().tobytes())
    return _to_mono(q, ch)


def _host_route(data, device):
    from .audio import _to_mono, decode_flac
    q, channels, sr = decode_flac(bytes(data))
    return torch.from_numpy(_to_mono(q, channels)).to(device), int(sr)


def decode_to_device(data_or_path, device=None):
    """A FLAC file (path or bytes) -> (mono float32 PCM on the device at the
    file's own rate, sample rate): the samples ``audio.decode`` gives, decoded
    on the device.  Any frame the device does not vouch for sends the whole
    file through ``audio.decode_flac`` (its samples, or its exception)."""
    device = torch.device(device or "cuda")
    data = read_bytes(data_or_path)
    ix = index(data)
    if ix is None:
        return _host_route(data, device)
    info, tab = ix
    n, ch = info.total_frames, info.channels
    if n == 0:
        return torch.empty(0, dtype=torch.float32, device=device), info.sample_rate
    comp = torch.from_numpy(_u8(data).copy()).to(device)
    s16 = torch.empty(n * ch, dtype=torch.int16, device=device)
    status = torch.empty(len(tab), dtype=torch.int32, device=device)
    ws = torch.empty(max(workspace_bytes(tab) // 4, 1), dtype=torch.int32, device=device)
    decode_device(comp, table_to_device(tab, device), len(tab), status, ws, out_s16=s16)
    if int(status.count_nonzero()):  # (the readback orders the decode before any use of s16)
        return _host_route(data, device)
    pcm = torch.empty(n, dtype=torch.float32, device=device)
    _lib.check(_lib.lib().aa_pcm_s16_to_f32(_lib.dptr(s16), n, ch, _lib.dptr(pcm), _lib.stream_ptr()),
               "aa_pcm_s16_to_f32")
    return pcm, info.sample_rate
