"""Batched corpus analysis: K recordings per GPU pass (BASELINE configs[3]).

The reference analyses one recording per process (``analyse.py FILE``,
src/analyse.py:434-470 -> classify(), src/identify_tracks.py:416-573).  Per
file that is decode, get_end, signal_noise, the track builder, the front end
and the models over the tracks' windows, and the post-processing to JSON.
On the GPU every one of those device steps is small for a single 60 s file
(tens of microseconds), so running them file by file leaves the device idle
behind launch latencies and blocking readbacks.  Here a rank takes its files
K at a time:

  * decode: worker threads read each PCM16 48 kHz WAV straight into a pinned
    host slot (other formats and rates go through ``load_recording``); the
    batch crosses PCIe as int16 and ``aa_pcm_s16_to_f32`` widens it on the
    device exactly as the host decode would.  With ``flac="gpu"`` a FLAC
    file stays compressed in its slot too: the worker only indexes its frames
    (``flac_gpu.index``), the compressed bytes cross PCIe, and one
    ``aa_flac_decode_device`` per batch decodes them into the same int16
    staging buffer; a file with a frame the device does not vouch for is
    redone through ``load_recording``, so its samples or its failure are the
    host route's.  With ``vorbis="gpu"`` an Ogg Vorbis file goes the same way:
    the worker indexes it (``vorbis_gpu.index``: packets, block timeline,
    flattened setup), the packet bytes cross PCIe, and one
    ``aa_vorbis_decode_device`` per batch decodes them into the staging buffer.
    With ``mp3="gpu"`` an MP3 file likewise: the worker indexes it
    (``mp3_gpu.index``: headers, side info, the bit reservoir laid out flat),
    the main data cross PCIe, and one ``aa_mp3_decode_device`` per batch
    decodes them -- with the host decoder's own core, so no file is redone;
  * get_end: one ``aa_span_nonzero`` launch over every file's chunk spans,
    one readback;
  * signal_noise: ``aa_sn_run_batch`` -- per file the STFT / medians / mask
    launches back to back, then one morphology + components pass for the
    whole batch -- into per-file result slots, one readback of the counts and
    component rows;
  * tracks: host, per file (as the reference);
  * classify: ``Classifier.classify_batch`` -- one front-end launch set over
    every file's windows, one forward per model, one track mean, one copy;
  * post-processing (``analyse.species_result``) on a host thread while the
    next batch runs on the device.

Each file's result is the document ``analyse.examine`` writes for it alone,
byte for byte (tests/test_gpu_batch.py): numpy's global RandomState is
reseeded per file right before its window schedule, exactly as the per-file
corpus path seeds it before ``examine``.
"""
from __future__ import annotations

import logging
import os
import struct
import time
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib

SR = 48000


@dataclass
class Decoded:
    """A decoded recording: ``s16`` (interleaved int16 samples as a view of a
    pinned slot, ``channels`` of them per frame) or ``f32`` (mono samples at
    ``sr_in``, resampled to 48 kHz on the device as they are uploaded; parity
    unpinned for those: aa_amd.resample is held to libsoxr HQ's specification,
    not to its samples, see its header)."""
    n: int                   # frames at 48 kHz
    sr: int                  # 48000
    s16: object = None       # numpy int16 [n * channels] (view into a pinned slot)
    s16_t: object = None     # the same bytes as a pinned torch int16 tensor
    channels: int = 1
    f32: object = None       # numpy float32 [n_in] at sr_in
    sr_in: int = SR
    slot: int = -1
    dev: object = None       # the recording's samples in the batch's device PCM
    flac: object = None      # flac="gpu": the frame table (flac_gpu.FRAME) of the compressed bytes ...
    comp_t: object = None    # ... which are this pinned torch uint8 view of the slot
    vorbis: object = None    # vorbis="gpu": the index (vorbis_gpu.Indexed); comp_t: its packet bytes in the slot
    mp3: object = None       # mp3="gpu": the index (mp3_gpu.Indexed); comp_t: its flat main data in the slot
    n_in: int = 0            # frames at sr_in the table decodes to
    path: str = ""

    def frames(self):
        """Host float32 samples at 48 kHz (only band-pass filtered tracks need them)."""
        if self.f32 is None and self.flac is not None:  # decoded on the device: the host decode, lazily
            from .audio import _to_mono, decode_flac
            q, ch, _ = decode_flac(self.comp_t.numpy().tobytes())
            self.f32 = _to_mono(q, ch)
        if self.f32 is None and (self.vorbis is not None or self.mp3 is not None):
            # (the slot holds packets / main data, not the file: read it again)
            from .audio import decode
            self.f32 = decode(self.path)[0]
        if self.f32 is None:
            from .audio import _to_mono
            self.f32 = _to_mono(np.asarray(self.s16), self.channels)
        if self.sr_in != SR:
            return self.dev.cpu().numpy()
        return self.f32


def _wav_pcm16(buf: np.ndarray, size: int):
    """(data offset, data bytes, channels, sr) if buf[:size] is a PCM16 RIFF/WAVE
    file, else None (decode() handles everything else)."""
    b = buf[:min(size, 1 << 16)].tobytes()
    if len(b) < 12 or b[:4] != b"RIFF" or b[8:12] != b"WAVE":
        return None
    pos, fmt = 12, None
    while pos + 8 <= size:
        if pos + 8 > len(b):
            b = buf[:min(size, pos + (1 << 16))].tobytes()
        cid, csz = b[pos:pos + 4], struct.unpack("<I", b[pos + 4:pos + 8])[0]
        if cid == b"fmt ":
            if pos + 8 + 16 > len(b):
                return None
            fmt = struct.unpack("<HHIIHH", b[pos + 8:pos + 24])
            if fmt[0] == 0xFFFE and csz >= 26 and pos + 34 <= len(b):
                fmt = (struct.unpack("<H", b[pos + 32:pos + 34])[0],) + fmt[1:]
        elif cid == b"data":
            if fmt is None:
                return None
            tag, ch, sr, _, _, bits = fmt
            if tag != 1 or bits != 16 or not 1 <= ch <= 8 or (pos + 8) % 2:
                return None
            n = min(csz, size - pos - 8)
            return pos + 8, n // (2 * ch) * 2 * ch, ch, sr
        pos += 8 + csz + (csz & 1)
    return None


class SlotPool:
    """Pinned host slots, each holding one file's bytes (one per recording in
    flight: the prefetch depth plus the batches on the device)."""

    def __init__(self, n_slots: int, slot_bytes: int):
        import threading
        self.bytes = int(slot_bytes)
        self.t, self.np, self.free = [], [], []
        self._cv = threading.Condition()
        self.grow(n_slots)

    def grow(self, n_slots: int):
        with self._cv:
            while len(self.t) < n_slots:
                self.t.append(torch.empty(self.bytes, dtype=torch.uint8, pin_memory=True))
                self.np.append(self.t[-1].numpy())
                self.free.append(len(self.t) - 1)
                self._cv.notify()

    def get(self) -> int:
        with self._cv:
            while not self.free:
                self._cv.wait()
            return self.free.pop()

    def put(self, i: int):
        with self._cv:
            self.free.append(i)
            self._cv.notify()


def flac_mode(flac=None) -> str:
    """"host" (aa_flac_decode on a decoder thread) or "gpu" (aa_flac_decode_device
    per batch); None: AA_FLAC, else "gpu" -- the default by the corpus A/B of
    DESIGN section 4 (`flac_decode_frames`)."""
    mode = flac or os.environ.get("AA_FLAC") or "gpu"
    if mode not in ("host", "gpu"):
        raise ValueError(f"flac={mode!r}: \"host\" or \"gpu\"")
    return mode


def vorbis_mode(vorbis=None) -> str:
    """"host" (aa_vorbis_decode on a decoder thread) or "gpu"
    (aa_vorbis_decode_device per batch); None: AA_VORBIS, else "host" -- opt-in
    until the corpus A/B of DESIGN section 4 (`vorbis_unpack`) says otherwise."""
    mode = vorbis or os.environ.get("AA_VORBIS") or "host"
    if mode not in ("host", "gpu"):
        raise ValueError(f"vorbis={mode!r}: \"host\" or \"gpu\"")
    return mode


def mp3_mode(mp3=None) -> str:
    """"host" (aa_mp3_decode on a decoder thread) or "gpu" (aa_mp3_decode_device
    per batch); None: AA_MP3, else "host" -- opt-in until a corpus A/B on the
    device says otherwise (`mp3_unpack`)."""
    mode = mp3 or os.environ.get("AA_MP3") or "host"
    if mode not in ("host", "gpu"):
        raise ValueError(f"mp3={mode!r}: \"host\" or \"gpu\"")
    return mode


def decode_into(path, pool: SlotPool, flac="host", vorbis="host", mp3="host",  # (BatchAnalyser passes its modes)
                sr_out=SR, wav_any_rate=False, host_decode=None):
    """Decode one file; PCM16 48 kHz WAV lands in a pinned slot untouched, and
    with flac="gpu" an indexable FLAC file stays there compressed; with
    vorbis="gpu" an indexable Ogg Vorbis file stays there as its audio packets
    (the index writes them over the file's bytes), and with mp3="gpu" an MP3
    file as its flat main data (likewise).
    The file comes in with one aa_read_file call (stat, open, read, close
    without the interpreter lock: the decoder threads otherwise queued for it
    behind the lanes' Python at every step).
    The batched old-index path (aa_amd.ci_batch) analyses at ``sr_out`` = 16 kHz
    and resamples every rate on the device, so it keeps a PCM16 WAV of any rate
    in its slot (``wav_any_rate``) and decodes the rest with ``host_decode``
    (path -> (mono f32, rate); default load_recording at the file's rate)."""
    import ctypes as C
    from . import identify_tracks as it
    from .audio import _is_flac
    i = pool.get()
    got = C.c_int64(0)
    rc = _lib.lib().aa_read_file(os.fsencode(path), pool.t[i].data_ptr(), pool.bytes, C.byref(got))
    if rc == _lib.AA_ERR_INVALID:
        pool.put(i)
        raise OSError(_lib.lib().aa_last_error().decode(errors="replace"))
    if rc == _lib.AA_OK:
        try:
            buf = pool.np[i]
            w = _wav_pcm16(buf, got.value)
            if w is not None and (wav_any_rate or w[3] == SR):
                off, nb, ch, sr = w
                t = pool.t[i][off:off + nb].view(torch.int16)
                n_in = nb // (2 * ch)
                n = n_in
                if sr != sr_out:
                    from .resample import out_length
                    n = out_length(n_in, sr, sr_out)
                return Decoded(n=n, sr=sr_out, s16=buf[off:off + nb].view(np.int16), s16_t=t,
                               channels=ch, sr_in=sr, slot=i, n_in=n_in, path=str(path))
            if flac == "gpu" and _is_flac(buf, got.value):
                from . import flac_gpu
                from .resample import out_length
                ix = flac_gpu.index(buf[:got.value])
                if ix is not None and ix[0].total_frames > 0 and flac_gpu.fits_batch(ix[1]):
                    info, tab = ix
                    return Decoded(n=out_length(info.total_frames, info.sample_rate, sr_out), sr=sr_out,
                                   channels=info.channels, sr_in=info.sample_rate, slot=i, flac=tab,
                                   comp_t=pool.t[i][:got.value], n_in=info.total_frames, path=str(path))
            if vorbis == "gpu" and got.value >= 4 and bytes(buf[:4]) == b"OggS":
                from . import vorbis_gpu
                from .resample import out_length
                ix = vorbis_gpu.index(buf[:got.value], payload=buf)
                if ix is not None and int(ix.stream["frames"][0]) > 0 and vorbis_gpu.fits_batch(ix):
                    st = ix.stream[0]
                    n_in, sr_in = int(st["frames"]), int(st["sample_rate"])
                    return Decoded(n=out_length(n_in, sr_in, sr_out), sr=sr_out, channels=int(st["channels"]), sr_in=sr_in,
                                   slot=i, vorbis=ix, comp_t=pool.t[i][:ix.payload.size], n_in=n_in, path=str(path))
            if mp3 == "gpu":
                from .audio import _is_mp3
                if _is_mp3(buf, got.value):
                    from . import mp3_gpu
                    from .resample import out_length
                    ix = mp3_gpu.index(buf[:got.value], payload=buf)
                    if ix is not None and int(ix.stream["frames"][0]) > 0 and mp3_gpu.fits_batch(ix):
                        st = ix.stream[0]
                        n_in, sr_in = int(st["frames"]), int(st["sample_rate"])
                        return Decoded(n=out_length(n_in, sr_in, sr_out), sr=sr_out, channels=int(st["channels"]),
                                       sr_in=sr_in, slot=i, mp3=ix, comp_t=pool.t[i][:ix.payload.size], n_in=n_in,
                                       path=str(path))
        except Exception:
            pool.put(i)
            raise
    pool.put(i)  # (larger than a slot, or not a 48 kHz PCM16 WAV)
    # FLAC, other WAV encodings; other rates are resampled on the device at upload
    frames, sr = host_decode(str(path)) if host_decode else it.load_recording(str(path), resample=None)
    from .resample import out_length
    return Decoded(n=out_length(len(frames), sr, sr_out), sr=sr_out,
                   f32=np.ascontiguousarray(frames, dtype=np.float32), sr_in=sr, n_in=len(frames), path=str(path))


class _Laps:
    """Wall time per host phase of the batch loop (AA_BATCH_PROFILE=1 prints it;
    AA_BATCH_TRACE=path also keeps every (thread, phase, start, end) interval,
    CLOCK_MONOTONIC ns like rocprofv3's kernel trace, written there as JSON)."""

    def __init__(self):
        self.t = {}
        self.cpu = {}  # the calling thread's CPU time per phase (time.thread_time)
        self._c0 = {}
        self.events = [] if os.environ.get("AA_BATCH_TRACE") else None

    def lap(self, name, t0):
        import threading
        t1 = time.perf_counter()
        self.t[name] = self.t.get(name, 0.0) + (t1 - t0)
        tid = threading.get_ident()
        c1 = time.thread_time()
        if tid in self._c0:
            self.cpu[name] = self.cpu.get(name, 0.0) + (c1 - self._c0[tid])
        self._c0[tid] = c1
        if self.events is not None:
            import threading
            now = time.clock_gettime_ns(time.CLOCK_MONOTONIC)
            self.events.append((threading.get_ident(), name, now - int((t1 - t0) * 1e9), now))
        return t1

    def report(self):
        return " ".join(f"{k}={1e3 * v:.1f}ms (cpu {1e3 * self.cpu.get(k, 0.0):.1f})" for k, v in self.t.items())


@dataclass
class _Rec:
    idx: int
    path: str
    dec: Decoded
    meta: object
    off: int = 0
    length: float = 0.0
    signals: list = field(default_factory=list)
    tracks: list = field(default_factory=list)
    res: object = None
    err: object = None


class _Lane:
    """One batch in flight: its own HIP stream and every device buffer a batch
    touches (PCM, int16 staging, signal_noise workspace and result slots, the
    front-end / model workspaces), so two host threads can each drive a batch:
    while one waits on its readbacks the other runs its host steps, and the
    device overlaps the two batches' kernels."""

    def __init__(self, dev):
        self.dev = dev
        self.stream = torch.cuda.Stream(device=dev)
        self.copy = torch.cuda.Stream(device=dev)
        self.pcm = torch.empty(0, dtype=torch.float32, device=dev)
        self.s16 = torch.empty(0, dtype=torch.int16, device=dev)
        self.sn_ws = None
        self.sn_buf = None
        self.ws = {}  # classify_batch workspaces
        # flac="gpu" / vorbis="gpu": compressed bytes, decode workspace, per-frame status, f32 before a resample
        self.flac = {}

    def flac_buffer(self, name, n, dtype):
        t = self.flac.get(name)
        if t is None or t.numel() < n:
            t = self.flac[name] = torch.empty(int(n * 1.25) + 1, dtype=dtype, device=self.dev)
        return t

    def buffers(self, n_f32, n_s16):
        if self.pcm.numel() < n_f32:
            self.pcm = torch.empty(int(n_f32 * 1.25) + 1, dtype=torch.float32, device=self.dev)
        if self.s16.numel() < n_s16:
            self.s16 = torch.empty(int(n_s16 * 1.25) + 1, dtype=torch.int16, device=self.dev)
        return self.pcm, self.s16


SN_CAP = 4096   # components per recording kept in the batch slots
VORBIS_WS_BYTES = 1 << 30  # workspace one aa_vorbis_decode_device call of a batch may take
MP3_WS_BYTES = 1 << 30     # the same for aa_mp3_decode_device (sixteen 60 s clips need about 0.86 GB)
PREFETCH = 2    # batches decoded ahead of the newest batch a lane has taken
_SN_LOCK = __import__("threading").Lock()
SN_HEAD = 64    # component rows read back with the counts (more: a second copy)

_POOLS = {}


def slot_pool(n_slots, slot_bytes):
    """Pinned slots persist across runs (allocating pinned memory is slow):
    one grow-only pool per slot size class."""
    size = -(-int(slot_bytes) // (1 << 20)) << 20
    pool = _POOLS.get(size)
    if pool is None:
        pool = _POOLS[size] = SlotPool(0, size)
    pool.grow(n_slots)
    return pool


class BatchAnalyser:
    """examine() for many files of one rank, K per device pass, ``lanes``
    batches in flight."""

    def __init__(self, bird_models, analyse_tracks=False, device=None, precision=None, batch=16, workers=8,
                 lanes=2, flac=None, vorbis=None, mp3=None):
        """flac: "host" decodes FLAC files on the decoder threads (aa_flac_decode),
        "gpu" on the device per batch (aa_flac_decode_device); None: AA_FLAC, else "gpu".
        vorbis: the same for Ogg Vorbis files (aa_vorbis_decode / aa_vorbis_decode_device);
        None: AA_VORBIS, else "host".
        mp3: the same for MP3 files (aa_mp3_decode / aa_mp3_decode_device); None: AA_MP3, else "host"."""
        self.flac = flac_mode(flac)
        self.vorbis = vorbis_mode(vorbis)
        self.mp3 = mp3_mode(mp3)
        from .identify_tracks import _group_models
        from .pipeline import Classifier
        self.bird_models = bird_models
        self.analyse_tracks = bool(analyse_tracks)
        self.dev = torch.device(device or "cuda")
        self.K = int(batch)
        self.workers = int(workers)
        self.n_lanes = max(1, int(lanes))
        self.groups = _group_models(bird_models) if bird_models is not None else None
        self.clf = Classifier.shared(precision=precision, device=self.dev)
        self.timing = _Laps()

    # ---- one batch --------------------------------------------------------
    def _upload(self, lane, recs):
        """PCM of the batch into one device f32 buffer (recording r at r.off)."""
        total = sum(r.dec.n for r in recs)
        n16 = sum(r.dec.n * r.dec.channels for r in recs if r.dec.s16 is not None)
        fl = [r for r in recs if r.dec.flac is not None]
        vb = [r for r in recs if r.dec.vorbis is not None]
        m3 = [r for r in recs if r.dec.mp3 is not None]
        n16 += sum(r.dec.n_in * r.dec.channels for r in fl + vb + m3)
        pcm, s16 = lane.buffers(total, n16)
        comp = (lane.flac_buffer("bytes", sum(r.dec.comp_t.numel() for r in fl + vb + m3), torch.uint8)
                if fl or vb or m3 else None)
        cur = torch.cuda.current_stream(self.dev)
        lane.copy.wait_stream(cur)  # the lane's previous batch is done with both buffers
        off = o16 = oc = 0
        with torch.cuda.stream(lane.copy):
            for r in recs:
                r.off = off
                d = r.dec
                if d.flac is not None or d.vorbis is not None or d.mp3 is not None:  # compressed; decoded into s16[o16:] below
                    comp[oc:oc + d.comp_t.numel()].copy_(d.comp_t, non_blocking=True)
                    d.oc, d.o16 = oc, o16
                    oc += d.comp_t.numel()
                    o16 += d.n_in * d.channels
                elif d.s16 is not None:
                    s16[o16:o16 + d.s16_t.numel()].copy_(d.s16_t, non_blocking=True)
                    d.o16 = o16
                    o16 += d.s16_t.numel()
                elif d.sr_in == SR:
                    pcm[off:off + d.n].copy_(torch.from_numpy(d.f32), non_blocking=False)
                off += d.n
        cur.wait_stream(lane.copy)
        L = _lib.lib()
        from .resample import resample_device
        if fl:
            pcm, total = self._flac_decode(lane, fl, comp, s16, pcm, total, cur)
        if vb:
            pcm, total = self._vorbis_decode(lane, vb, comp, s16, pcm, total, cur)
        if m3:
            self._mp3_decode(lane, m3, comp, s16, cur)
        # every recording mono PCM16 (or FLAC decoded to it) at 48 kHz: the int16
        # and f32 offsets coincide, so one widening launch covers the batch.  (A
        # file that failed its host redo counts too: it still holds its place in
        # both buffers, and only as mono 48 kHz are the two places the same.)
        mono16 = all((r.dec.s16 is not None or
                      ((r.dec.flac is not None or r.dec.vorbis is not None or r.dec.mp3 is not None) and
                       r.dec.sr_in == SR)) and
                     r.dec.channels == 1 for r in recs)
        if mono16 and total:
            _lib.check(L.aa_pcm_s16_to_f32(_lib.dptr(s16), total, 1, _lib.dptr(pcm), _lib.stream_ptr(cur)),
                       "aa_pcm_s16_to_f32")
        for r in recs:
            d = r.dec
            d.dev = pcm[r.off:r.off + d.n]
            if mono16 or r.err is not None:
                continue
            if d.flac is not None or d.vorbis is not None or d.mp3 is not None:
                if d.sr_in == SR:
                    _lib.check(L.aa_pcm_s16_to_f32(_lib.dptr(s16) + 2 * d.o16, d.n, d.channels,
                                                   _lib.dptr(pcm) + 4 * r.off, _lib.stream_ptr(cur)),
                               "aa_pcm_s16_to_f32")
                else:  # widen at the file's rate, then librosa.resample to 48 kHz as the host route does
                    tmp = lane.flac_buffer("f32", d.n_in, torch.float32)[:d.n_in]
                    _lib.check(L.aa_pcm_s16_to_f32(_lib.dptr(s16) + 2 * d.o16, d.n_in, d.channels, _lib.dptr(tmp),
                                                   _lib.stream_ptr(cur)), "aa_pcm_s16_to_f32")
                    resample_device(tmp, d.sr_in, SR, out=d.dev)
            elif d.s16 is not None and d.n:
                _lib.check(L.aa_pcm_s16_to_f32(_lib.dptr(s16) + 2 * d.o16, d.n, d.channels,
                                               _lib.dptr(pcm) + 4 * r.off, _lib.stream_ptr(cur)),
                           "aa_pcm_s16_to_f32")
            elif d.s16 is None and d.sr_in != SR:  # librosa.resample to 48 kHz (aa_amd.resample)
                resample_device(torch.from_numpy(d.f32).to(self.dev), d.sr_in, SR, out=d.dev)
        return pcm[:total]

    def _flac_decode(self, lane, fl, comp, s16, pcm, total, cur):
        """One aa_flac_decode_device over the batch's FLAC files (compressed
        bytes in comp, samples into s16), then the per-frame statuses: a file
        with any frame not OK is redone through load_recording, the host route,
        whose samples -- or whose "Could not load" -- then stand for it.
        Returns (pcm, total): the host route may decode another number of
        samples than the index counted (a crafted stream); fewer use the head
        of the file's place in pcm, more move the file behind the batch."""
        from . import flac_gpu
        tab = flac_gpu.concat([r.dec.flac for r in fl], [r.dec.oc for r in fl], [r.dec.o16 for r in fl])
        status = lane.flac_buffer("status", len(tab), torch.int32)[:len(tab)]
        ws = lane.flac_buffer("ws", max(flac_gpu.workspace_bytes(tab) // 4, 1), torch.int32)
        flac_gpu.decode_device(comp, flac_gpu.table_to_device(tab, self.dev), len(tab), status, ws, out_s16=s16,
                               stream=cur)
        st = status.cpu().numpy()  # before any of these files' samples is used
        bad = sorted(set(tab["stream"][st != _lib.AA_FLAC_OK].tolist()))
        return self._redo_on_host(lane, [fl[k] for k in bad], pcm, total)

    def _vorbis_decode(self, lane, vb, comp, s16, pcm, total, cur):
        """aa_vorbis_decode_device over the batch's Ogg Vorbis files (packet
        bytes in comp, samples into s16), then the per-packet statuses, read
        before any sample is used: a file with any packet not OK is redone
        through load_recording like a FLAC file (_flac_decode).  The files are
        taken in as many calls as keep one call's workspace under
        VORBIS_WS_BYTES (a file alone may exceed it)."""
        from . import vorbis_gpu as vg
        groups, size = [[]], 0
        for r in vb:
            need = vg.workspace_bytes(r.dec.vorbis.packets, r.dec.vorbis.stream)
            if groups[-1] and size + need > VORBIS_WS_BYTES:
                groups.append([])
                size = 0
            groups[-1].append(r)
            size += need
        bad = []
        for g in groups:
            b = vg.concat([r.dec.vorbis for r in g], [r.dec.oc for r in g], [r.dec.o16 for r in g])
            if not len(b.packets):
                continue
            pl, nb = vg.plan(b.packets, b.streams)
            status = lane.flac_buffer("status", len(b.packets), torch.int32)[:len(b.packets)]
            ws = lane.flac_buffer("vorbis_ws", max(nb // 8, 1), torch.int64)
            vg.decode_device(comp, vg.to_device(b.packets, self.dev), len(b.packets), vg.to_device(b.streams, self.dev),
                             len(b.streams), vg.to_device(b.setups, self.dev), pl, status, ws, out_s16=s16,
                             out_elems=s16.numel(), stream=cur)
            st = status.cpu().numpy()  # (orders the decode before the next group reuses the workspace, too)
            bad += [g[k] for k in sorted(set(b.packets["stream"][st != _lib.AA_VORBIS_OK].tolist()))]
        return self._redo_on_host(lane, bad, pcm, total)

    def _mp3_decode(self, lane, m3, comp, s16, cur):
        """aa_mp3_decode_device over the batch's MP3 files (flat main data in
        comp, samples into s16), in as many calls as keep one call's workspace
        under MP3_WS_BYTES (a file alone may exceed it).  The device runs the
        host decoder's core, damaged frames included (silence on both sides),
        so no status is read back and no file is redone."""
        from . import mp3_gpu as mg
        groups, size = [[]], 0
        for r in m3:
            need = mg.workspace_bytes(len(r.dec.mp3.frames))
            if groups[-1] and size + need > MP3_WS_BYTES:
                groups.append([])
                size = 0
            groups[-1].append(r)
            size += need
        for g in groups:
            b = mg.concat([r.dec.mp3 for r in g], [r.dec.oc for r in g], [r.dec.o16 for r in g])
            if not len(b.frames):
                continue
            status = lane.flac_buffer("status", 4 * len(b.frames), torch.int32)[:4 * len(b.frames)]
            ws = lane.flac_buffer("mp3_ws", max(mg.workspace_bytes(len(b.frames)) // 8, 1), torch.int64)
            mg.decode_device(comp, mg.to_device(b.frames, self.dev), len(b.frames), mg.to_device(b.streams, self.dev),
                             len(b.streams), status, ws, out_s16=s16, out_elems=s16.numel(), stream=cur)

    def _redo_on_host(self, lane, bad, pcm, total):
        """The files of `bad` (device-decoded, not vouched for) through
        load_recording; returns (pcm, total) as _flac_decode describes."""
        from . import identify_tracks as it
        from .resample import out_length
        redone = []
        for r in bad:
            d = r.dec
            try:
                frames, sr = it.load_recording(d.path, resample=None)
            except Exception as e:
                logging.error("Could not load %s", d.path, exc_info=True)
                r.err = e if isinstance(e, ValueError) else Exception(f"Could not load {d.path}")
                continue
            d.flac = d.vorbis = None
            d.f32, d.sr_in = np.ascontiguousarray(frames, dtype=np.float32), int(sr)
            n = out_length(len(d.f32), d.sr_in, SR)
            if n > d.n:  # no room in its place: behind the batch
                r.off = total
                total += n
            d.n = n
            redone.append(r)
        if total > pcm.numel():
            grown = torch.empty(int(total * 1.25) + 1, dtype=torch.float32, device=self.dev)
            grown[:pcm.numel()].copy_(pcm)
            pcm = lane.pcm = grown
        for r in redone:
            d = r.dec
            if d.sr_in == SR:  # (other rates: the loop in _upload resamples d.f32)
                pcm[r.off:r.off + d.n].copy_(torch.from_numpy(d.f32), non_blocking=False)
        return pcm, total

    def _get_end(self, pcm, recs):
        """get_end (src/identify_tracks.py:387-413) of every recording, one launch."""
        from .gpu_ops import get_end_spans
        spans, owner, starts = [], [], []
        for k, r in enumerate(recs):
            sp, st, hop = get_end_spans(r.dec.n, r.dec.sr)
            r.length = r.dec.n / r.dec.sr
            if len(st):
                spans.append(sp + r.off)
                owner += [k] * len(st)
                starts += st
        if not spans:
            return
        sp = torch.from_numpy(np.concatenate(spans)).to(self.dev)
        flags = torch.empty(len(owner), dtype=torch.int32, device=self.dev)
        _lib.check(_lib.lib().aa_span_nonzero(_lib.dptr(pcm), int(pcm.numel()), _lib.dptr(sp), len(owner),
                                              _lib.dptr(flags), _lib.stream_ptr()), "aa_span_nonzero")
        f = flags.cpu().numpy()
        seen = set()
        for j in np.flatnonzero(f == 0):
            k = owner[j]
            if k not in seen:  # the first constant chunk of recording k
                seen.add(k)
                recs[k].length = starts[j] * 281 // recs[k].dec.sr

    def _signal_noise(self, lane, pcm, recs):
        """signal_noise (src/identify_tracks.py:650-706) of every recording:
        aa_sn_run_batch over up to 64 recordings at a time (per recording the
        STFT / medians / mask launches, then one morphology + components pass
        for all of them) into per-recording slots [1 + SN_CAP][6] int32 (row 0:
        count, status), one readback of every slot's head."""
        import ctypes as C
        from .identify_tracks import Signal
        from .signals import detector
        by_sr = {}
        for k, r in enumerate(recs):
            by_sr.setdefault(r.dec.sr, []).append(k)
        L = _lib.lib()
        for sr, ks in by_sr.items():
            det = detector(sr, 281, self.dev)
            nsig = [int(sr * recs[k].length) for k in ks]
            K = min(len(ks), 64)
            need = L.aa_sn_batch_workspace_bytes(det._h, max(nsig), K)
            if lane.sn_ws is None or lane.sn_ws.numel() < need:
                lane.sn_ws = torch.empty(need, dtype=torch.uint8, device=self.dev)
            if lane.sn_buf is None or lane.sn_buf.shape[0] < len(ks):
                lane.sn_buf = torch.empty((len(ks), 1 + SN_CAP, 6), dtype=torch.int32, device=self.dev)
            buf, ws = lane.sn_buf, lane.sn_ws
            for c0 in range(0, len(ks), 64):
                part = ks[c0:c0 + 64]
                offs = (C.c_int64 * len(part))(*[recs[k].off if nsig[c0 + j] else 0 for j, k in enumerate(part)])
                lens = (C.c_int64 * len(part))(*nsig[c0:c0 + len(part)])
                _lib.check(L.aa_sn_run_batch(det._h, _lib.dptr(pcm), offs, lens, len(part), _lib.dptr(ws), ws.numel(),
                                             _lib.dptr(buf[c0, 1:]), SN_CAP, 1 + SN_CAP, _lib.dptr(buf[c0, 0]),
                                             (1 + SN_CAP) * 6, _lib.stream_ptr()), "aa_sn_run_batch")
            head = buf[:len(ks), :1 + SN_HEAD].cpu().numpy()
            for j, k in enumerate(ks):
                c, status = int(head[j, 0, 0]), int(head[j, 0, 1])
                if status & _lib.AA_SN_NONFINITE:
                    recs[k].err = ValueError("Audio buffer is not finite everywhere")  # librosa valid_audio
                    continue
                if status & _lib.AA_SN_RUN_OVERFLOW or c > SN_CAP:
                    # more components than a slot holds: this recording alone,
                    # through the detector's own (shared) buffers
                    try:
                        with _SN_LOCK:
                            stats = det.components(pcm[recs[k].off:recs[k].off + nsig[j]])
                    except Exception as e:
                        recs[k].err = e
                        continue
                else:
                    rows = head[j, 1:1 + c] if c <= SN_HEAD else buf[j, 1:1 + c].cpu().numpy()
                    rows = rows.astype(np.int64)
                    stats = rows[np.lexsort((rows[:, 5], rows[:, 0]))][:, :5]
                recs[k].signals = [Signal(*tu) for tu in det.to_tuples(stats)]

    def _classify(self, lane, pcm, recs):
        from .identify_tracks import MAX_FRQUENCY, Signal, tracks_from_signals
        from .pipeline import BatchRec
        todo = []
        for r in recs:
            if r.err is not None:
                continue
            raw_length = r.dec.n / r.dec.sr
            if self.analyse_tracks:
                if r.meta is None:
                    r.res = None
                    continue
                tracks = []
                for t in r.meta["Tracks"]:
                    s = Signal(t["start"], t["end"], t.get("minFreq", 0), t.get("maxFreq", MAX_FRQUENCY))
                    s.track_id = t["id"]
                    tracks.append(s)
            else:
                tracks = tracks_from_signals(r.signals, r.length)
            if len(tracks) == 0:
                r.res = ([], r.length, [], raw_length, [])
                continue
            r.tracks = tracks
            todo.append(r)
        if not todo:
            return
        brs = [BatchRec(n=r.dec.n, off=r.off, tracks=r.tracks, frames=r.dec.frames, seed=r.idx) for r in todo]
        out = self.clf.classify_batch(pcm, SR, brs, self.groups, ws=lane.ws)
        for r, o in zip(todo, out):
            if isinstance(o, BaseException):
                r.err = o
            else:
                r.res = (r.tracks, r.length, r.signals, r.dec.n / r.dec.sr, list(o))

    def _finish(self, recs, t0):
        from .analyse import species_result
        from .corpus import FAILED
        out = {}
        dt = round((time.time() - t0) / max(len(recs), 1), 1)
        for r in recs:
            if r.err is not None:
                logging.error("%s: %s", r.path, r.err)
                out[r.idx] = {FAILED: f"{type(r.err).__name__}: {r.err}"}
                continue
            doc = species_result(r.res, r.meta, self.analyse_tracks, self.bird_models is not None)
            doc["processing_time_seconds"] = dt
            out[r.idx] = doc
        return out

    def process(self, items, lane, pool=None):
        """items: [(file_idx, path, Decoded | Exception, sidecar meta)] -> {file_idx: document}."""
        t0 = time.time()
        recs, failed, held = [], [], []
        for idx, path, dec, meta in items:
            if isinstance(dec, BaseException):
                failed.append(_Rec(idx, str(path), None, meta, err=dec))
            else:
                recs.append(_Rec(idx, str(path), dec, meta))
        if recs:
            held = recs
            try:
                with torch.cuda.stream(lane.stream):
                    tm = self.timing
                    t = time.perf_counter()
                    pcm = self._upload(lane, recs)
                    t = tm.lap("upload", t)
                    held = recs  # (their slots are returned below)
                    failed += [r for r in recs if r.err is not None]  # a FLAC file the host route could not load
                    recs = [r for r in recs if r.err is None]
                    self._get_end(pcm, recs)
                    t = tm.lap("get_end", t)
                    self._signal_noise(lane, pcm, recs)
                    t = tm.lap("signal_noise", t)
                    self._classify(lane, pcm, recs)
                    tm.lap("classify", t)
            finally:
                # (the slots stay held until here: band-pass filtered tracks
                # read a recording's host samples during classify)
                if pool is not None:
                    for r in held:
                        if r.dec.slot >= 0:
                            pool.put(r.dec.slot)
                            r.dec.slot = -1
        t = time.perf_counter()
        docs = self._finish(recs + failed, t0)
        self.timing.lap("post", t)
        return docs

    def _load(self, path, pool):
        """(Decoded | the exception that stands for the file, sidecar meta) of one file, on a decoder thread."""
        from .analyse import read_sidecar
        meta = None
        try:
            meta = read_sidecar(path)
            return decode_into(path, pool, self.flac, self.vorbis, self.mp3), meta
        except Exception as e:
            logging.error("Could not load %s", path, exc_info=True)
            return Exception(f"Could not load {path}") if not isinstance(e, ValueError) else e, meta

    def run(self, jobs):
        """jobs: [(file_idx, path)] -> {file_idx: document} (the files of this rank)."""
        import threading
        from .analyse import read_sidecar
        if not jobs:
            return {}
        if self.bird_models is None:  # examine() without models reads no audio
            from .analyse import species_result
            return {i: dict(species_result(None, read_sidecar(p), self.analyse_tracks, False),
                            processing_time_seconds=0.0) for i, p in sorted(jobs)}
        K = self.K
        lanes = [_Lane(self.dev) for _ in range(min(self.n_lanes, -(-len(jobs) // K)))]
        slot_bytes = max(os.path.getsize(p) for _, p in jobs) + 4096
        # slots: every lane's batch plus PREFETCH batches decoded ahead of the
        # newest batch a lane has taken -- exactly the batches that can hold
        # slots at once, so a decode never waits for a slot (a waiting decode
        # of a later batch could otherwise hold the slots the oldest batch needs)
        pool = slot_pool(min(len(jobs), (len(lanes) + PREFETCH) * K), slot_bytes)

        def load(job):
            idx, path = job
            return (idx, path) + self._load(path, pool)

        results, errors = {}, []
        lock = threading.Lock()
        batches = [jobs[b:b + K] for b in range(0, len(jobs), K)]
        with ThreadPoolExecutor(max_workers=self.workers) as io:
            futs = {}  # batch index -> its decode futures, submitted PREFETCH batches ahead
            state = {"next": 0, "submitted": 0}

            def submit_upto(b):
                while state["submitted"] < min(b, len(batches)):
                    futs[state["submitted"]] = [io.submit(load, j) for j in batches[state["submitted"]]]
                    state["submitted"] += 1

            def worker(lane):
                torch.cuda.set_device(self.dev)
                prof = None
                if os.environ.get("AA_BATCH_CPROFILE"):  # host-side profile of this lane (tools)
                    import cProfile
                    # AA_BATCH_CPROFILE_CPU=1: the lane thread's CPU time (what
                    # holds the GIL) instead of wall time (GPU waits included)
                    cpu = os.environ.get("AA_BATCH_CPROFILE_CPU") == "1"
                    prof = cProfile.Profile(time.thread_time) if cpu else cProfile.Profile()
                    prof.enable()
                try:
                    while True:
                        with lock:
                            b = state["next"]
                            if b >= len(batches):
                                return
                            state["next"] += 1
                            submit_upto(b + 1 + PREFETCH)
                            fb = futs.pop(b)
                        t = time.perf_counter()
                        items = [f.result() for f in fb]
                        self.timing.lap("wait_decode", t)
                        docs = self.process(items, lane, pool)
                        with lock:
                            results.update(docs)
                except BaseException as e:  # surfaces in the caller
                    errors.append(e)
                finally:
                    if prof is not None:
                        prof.disable()
                        prof.dump_stats(f"{os.environ['AA_BATCH_CPROFILE']}.{time.monotonic_ns()}")

            with lock:
                submit_upto(len(lanes) + PREFETCH)
            threads = [threading.Thread(target=worker, args=(ln,), daemon=True) for ln in lanes]
            for th in threads:
                th.start()
            for th in threads:
                th.join()
        for ln in lanes:
            ln.stream.synchronize()
        if errors:
            raise errors[0]
        if os.environ.get("AA_BATCH_PROFILE"):
            logging.warning("batch phases over %d files (%d lanes): %s", len(jobs), len(lanes), self.timing.report())
        if self.timing.events is not None:
            import json
            with open(os.environ["AA_BATCH_TRACE"], "w") as f:
                json.dump(self.timing.events, f)
        return dict(sorted(results.items()))
