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
    device exactly as the host decode would.  A FLAC, Ogg Vorbis or MP3 file
    whose mode is "gpu" (``CODECS``: ``flac=``, ``vorbis=``, ``mp3=``) stays
    compressed in its slot too: the worker only indexes it (the codec module's
    ``index_slot``: FLAC frames; Vorbis packets, block timeline and flattened
    setup; MP3 headers, side info and the bit reservoir laid out flat), the
    compressed bytes cross PCIe, and the module's ``decode_batch`` decodes
    every such file of the batch into the same int16 staging buffer.  A file
    the device does not vouch for is redone through ``load_recording``, so
    its samples or its failure are the host route's (MP3 runs the host
    decoder's own core on the device, so none of its files is redone);
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
from functools import partial

import numpy as np
import torch

from . import _lib, flac_gpu, mp3_gpu, vorbis_gpu
from .resample import out_length

SR = 48000
# The device codecs (see _codec), in the order decode_into tries them and a batch
# launches them: name (the keyword argument), module, environment variable, default
# mode.  FLAC is "gpu" by the corpus A/B of DESIGN section 4 (`flac_decode_frames`);
# Vorbis and MP3 are opt-in until theirs say otherwise (`vorbis_unpack`, `mp3_unpack`).
CODECS = (("flac", flac_gpu, "AA_FLAC", "gpu"),
          ("vorbis", vorbis_gpu, "AA_VORBIS", "host"),
          ("mp3", mp3_gpu, "AA_MP3", "host"))


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
    codec: object = None     # decoded on the device: the module of CODECS that does it, ...
    index: object = None     # ... its index of the file (Slotted.index: flac_gpu.FRAME table, vorbis_gpu / mp3_gpu Indexed) ...
    comp_t: object = None    # ... and the compressed bytes: this pinned torch uint8 view of the slot, ...
    nbytes: int = 0          # ... this many
    n_in: int = 0            # frames at sr_in the index decodes to
    path: str = ""

    def frames(self):
        """Host float32 samples at 48 kHz (only band-pass filtered tracks need them)."""
        if self.f32 is None and self.codec is not None:  # decoded on the device: the host decode, lazily
            self.f32 = self.codec.host_samples(self)
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


def codec_mode(name, value=None) -> str:
    """How the corpus path decodes the files of codec ``name`` of CODECS: "host"
    (on a decoder thread) or "gpu" (on the device, per batch); None: the
    codec's environment variable, else its default."""
    env, default = next(c[2:] for c in CODECS if c[0] == name)
    mode = value or os.environ.get(env) or default
    if mode not in ("host", "gpu"):
        raise ValueError(f"{name}={mode!r}: \"host\" or \"gpu\"")
    return mode


flac_mode = partial(codec_mode, "flac")
vorbis_mode = partial(codec_mode, "vorbis")
mp3_mode = partial(codec_mode, "mp3")


def decode_into(path, pool: SlotPool, codecs=(), sr_out=SR, wav_any_rate=False, host_decode=None):
    """Decode one file; PCM16 48 kHz WAV lands in a pinned slot untouched, and
    a file that one of ``codecs`` (modules of CODECS) takes stays there compressed: a
    FLAC file as it is, an Ogg Vorbis file as its audio packets and an MP3 file
    as its flat main data (the index writes them over the file's bytes).
    The file comes in with one aa_read_file call (stat, open, read, close
    without the interpreter lock: the decoder threads otherwise queued for it
    behind the lanes' Python at every step).
    The batched old-index path (aa_amd.ci_batch) analyses at ``sr_out`` = 16 kHz
    and resamples every rate on the device, so it keeps a PCM16 WAV of any rate
    in its slot (``wav_any_rate``) and decodes the rest with ``host_decode``
    (path -> (mono f32, rate); default load_recording at the file's rate)."""
    import ctypes as C
    from . import identify_tracks as it
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
                n = n_in if sr == sr_out else out_length(n_in, sr, sr_out)
                return Decoded(n=n, sr=sr_out, s16=buf[off:off + nb].view(np.int16), s16_t=t,
                               channels=ch, sr_in=sr, slot=i, n_in=n_in, path=str(path))
            for codec in codecs:
                s = codec.index_slot(buf, got.value) if codec.sniff(buf, got.value) else None
                if s is not None:
                    return Decoded(n=out_length(s.n_in, s.sr_in, sr_out), sr=sr_out, channels=s.channels,
                                   sr_in=s.sr_in, slot=i, codec=codec, index=s.index, nbytes=s.payload_bytes,
                                   comp_t=pool.t[i][:s.payload_bytes], n_in=s.n_in, path=str(path))
        except Exception:
            pool.put(i)
            raise
    pool.put(i)  # (larger than a slot, or not a 48 kHz PCM16 WAV)
    # FLAC, other WAV encodings; other rates are resampled on the device at upload
    frames, sr = host_decode(str(path)) if host_decode else it.load_recording(str(path), resample=None)
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


def split_items(items):
    """items of process(): (_Rec of every decoded file, _Rec with ``err`` of every file whose decode raised)."""
    recs, failed = [], []
    for idx, path, dec, meta in items:
        if isinstance(dec, BaseException):
            failed.append(_Rec(idx, str(path), None, meta, err=dec))
        else:
            recs.append(_Rec(idx, str(path), dec, meta))
    return recs, failed


def return_slots(pool, recs):
    if pool is not None:
        for r in recs:
            if r.dec.slot >= 0:
                pool.put(r.dec.slot)
                r.dec.slot = -1


def staging_layout(decs):
    """Where a batch's recordings go, from the Decodeds alone: per recording
    (off, o16, oc) -- its first sample in the batch's f32 PCM (``n`` each, back
    to back), its first element in the int16 staging buffer (PCM16 as it is; a
    compressed file the n_in * channels samples it decodes to; None: host f32)
    and its first byte in the compressed buffer (None: not compressed) -- and
    the three buffers' sizes."""
    places, off, o16, oc = [], 0, 0, 0
    for d in decs:
        if d.codec is not None:
            places.append((off, o16, oc))
            oc += d.nbytes
            o16 += d.n_in * d.channels
        elif d.s16 is not None:
            places.append((off, o16, None))
            o16 += d.s16.size
        else:
            places.append((off, None, None))
        off += d.n
    return places, off, o16, oc


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
        # grow-only buffers by purpose: compressed bytes, the codecs' workspaces and
        # (shared) status, f32 before a resample, the old index's segments and workspace
        self._scratch = {}

    def scratch(self, name, n, dtype):
        t = self._scratch.get(name)
        if t is None or t.numel() < n:
            t = self._scratch[name] = torch.empty(int(n * 1.25) + 1, dtype=dtype, device=self.dev)
        return t

    def buffers(self, n_f32, n_s16):
        if self.pcm.numel() < n_f32:
            self.pcm = torch.empty(int(n_f32 * 1.25) + 1, dtype=torch.float32, device=self.dev)
        if self.s16.numel() < n_s16:
            self.s16 = torch.empty(int(n_s16 * 1.25) + 1, dtype=torch.int16, device=self.dev)
        return self.pcm, self.s16


SN_CAP = 4096   # components per recording kept in the batch slots
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
        """flac, vorbis, mp3: "host" decodes such files on the decoder threads, "gpu"
        on the device per batch; None: AA_FLAC / AA_VORBIS / AA_MP3, else the default (codec_mode)."""
        from .identify_tracks import _group_models
        from .pipeline import Classifier
        self._setup(device, batch, workers, lanes, flac, vorbis, mp3)
        self.bird_models = bird_models
        self.analyse_tracks = bool(analyse_tracks)
        self.groups = _group_models(bird_models) if bird_models is not None else None
        self.clf = Classifier.shared(precision=precision, device=self.dev)

    def _setup(self, device, batch, workers, lanes, flac, vorbis, mp3):
        """What the run loop and the staging of a batch need (CiBatchAnalyser's too)."""
        given = {"flac": flac, "vorbis": vorbis, "mp3": mp3}
        self.codecs = [mod for name, mod, _, _ in CODECS if codec_mode(name, given[name]) == "gpu"]  # for decode_into
        self.dev = torch.device(device or "cuda")
        self.K = int(batch)
        self.workers = int(workers)
        self.n_lanes = max(1, int(lanes))
        self.timing = _Laps()

    # ---- one batch --------------------------------------------------------
    def _stage(self, lane, recs, f32=True):
        """The batch's slots into the lane's buffers on lane.copy, each recording
        where staging_layout puts it (r.off, r.dec.o16, r.dec.oc): compressed
        bytes into comp, PCM16 into s16 and, with ``f32``, host-decoded samples
        already at 48 kHz into pcm.  Returns (pcm, s16, comp, total, cur)."""
        places, total, n16, nc = staging_layout([r.dec for r in recs])
        pcm, s16 = lane.buffers(total if f32 else 0, n16)
        comp = lane.scratch("bytes", nc, torch.uint8) if any(r.dec.codec is not None for r in recs) else None
        cur = torch.cuda.current_stream(self.dev)
        lane.copy.wait_stream(cur)  # the lane's previous batch is done with the buffers
        with torch.cuda.stream(lane.copy):
            for r, (off, o16, oc) in zip(recs, places):
                d = r.dec
                r.off, d.o16, d.oc = off, o16, oc
                if d.codec is not None:  # compressed; decoded into s16[o16:] by _decode_compressed
                    comp[oc:oc + d.nbytes].copy_(d.comp_t, non_blocking=True)
                elif d.s16 is not None:
                    s16[o16:o16 + d.s16.size].copy_(d.s16_t, non_blocking=True)
                elif f32 and d.sr_in == SR:
                    pcm[off:off + d.n].copy_(torch.from_numpy(d.f32), non_blocking=False)
        cur.wait_stream(lane.copy)
        return pcm, s16, comp, total, cur

    def _decode_compressed(self, lane, recs, comp, s16, cur, pcm=None, total=0):
        """Each codec's decode_batch, in CODECS order, over its files of the
        batch (compressed bytes in comp, samples into s16); the files a codec
        does not vouch for are redone on the host (_redo_on_host) before the
        next codec runs.  Returns (pcm, total) as _redo_on_host leaves them."""
        for _, codec, _, _ in CODECS:
            rs = [r for r in recs if r.dec.codec is codec]
            if not rs:
                continue
            bad = codec.decode_batch(lane.scratch, [r.dec.index for r in rs], [r.dec.oc for r in rs],
                                     [r.dec.o16 for r in rs], comp, s16, self.dev, cur)
            if bad:
                pcm, total = self._redo_on_host(lane, [rs[k] for k in bad], pcm, total)
        return pcm, total

    def _upload(self, lane, recs):
        """PCM of the batch into one device f32 buffer (recording r at r.off)."""
        pcm, s16, comp, total, cur = self._stage(lane, recs)
        L = _lib.lib()
        from .resample import resample_device
        pcm, total = self._decode_compressed(lane, recs, comp, s16, cur, pcm, total)
        # every recording mono PCM16 (or a compressed file decoded to it) at 48 kHz:
        # the int16 and f32 offsets coincide, so one widening launch covers the
        # batch.  (A file that failed its host redo counts too: it still holds its
        # place in both buffers, and only as mono 48 kHz are the two places the same.)
        mono16 = all((r.dec.s16 is not None or (r.dec.codec is not None and r.dec.sr_in == SR)) and
                     r.dec.channels == 1 for r in recs)

        def widen(o16, n, channels, dst):  # n frames from s16[o16:] as mono f32 to the device address dst
            _lib.check(L.aa_pcm_s16_to_f32(_lib.dptr(s16) + 2 * o16, n, channels, dst, _lib.stream_ptr(cur)),
                       "aa_pcm_s16_to_f32")

        if mono16 and total:
            widen(0, total, 1, _lib.dptr(pcm))
        for r in recs:
            d = r.dec
            d.dev = pcm[r.off:r.off + d.n]
            if mono16 or r.err is not None:
                continue
            if d.codec is not None and d.sr_in != SR:
                # widen at the file's rate, then librosa.resample to 48 kHz as the host route does
                tmp = lane.scratch("f32", d.n_in, torch.float32)[:d.n_in]
                widen(d.o16, d.n_in, d.channels, _lib.dptr(tmp))
                resample_device(tmp, d.sr_in, SR, out=d.dev)
            elif d.codec is not None or (d.s16 is not None and d.n):
                widen(d.o16, d.n, d.channels, _lib.dptr(pcm) + 4 * r.off)
            elif d.s16 is None and d.sr_in != SR:  # librosa.resample to 48 kHz (aa_amd.resample)
                resample_device(torch.from_numpy(d.f32).to(self.dev), d.sr_in, SR, out=d.dev)
        return pcm[:total]

    def _redo_on_host(self, lane, bad, pcm, total):
        """The files of `bad` (device-decoded, not vouched for) through
        load_recording, the host route, whose samples -- or whose "Could not
        load" -- then stand for them.  Returns (pcm, total): the host route may
        decode another number of samples than the index counted (a crafted
        stream); fewer use the head of the file's place in pcm, more move the
        file behind the batch."""
        from . import identify_tracks as it
        redone = []
        for r in bad:
            d = r.dec
            try:
                frames, sr = it.load_recording(d.path, resample=None)
            except Exception as e:
                logging.error("Could not load %s", d.path, exc_info=True)
                r.err = e if isinstance(e, ValueError) else Exception(f"Could not load {d.path}")
                continue
            d.codec = d.index = None
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
        recs, failed = split_items(items)
        ok = []
        if recs:
            try:
                with torch.cuda.stream(lane.stream):
                    tm = self.timing
                    t = time.perf_counter()
                    pcm = self._upload(lane, recs)
                    t = tm.lap("upload", t)
                    failed += [r for r in recs if r.err is not None]  # a file the host redo could not load
                    ok = [r for r in recs if r.err is None]
                    self._get_end(pcm, ok)
                    t = tm.lap("get_end", t)
                    self._signal_noise(lane, pcm, ok)
                    t = tm.lap("signal_noise", t)
                    self._classify(lane, pcm, ok)
                    tm.lap("classify", t)
            finally:
                # (the slots stay held until here: band-pass filtered tracks
                # read a recording's host samples during classify)
                return_slots(pool, recs)
        t = time.perf_counter()
        docs = self._finish(ok + failed, t0)
        self.timing.lap("post", t)
        return docs

    def _load(self, path, pool):
        """(Decoded | the exception that stands for the file, sidecar meta) of one file, on a decoder thread."""
        from .analyse import read_sidecar
        meta = None
        try:
            meta = read_sidecar(path)
            return decode_into(path, pool, self.codecs), meta
        except Exception as e:
            logging.error("Could not load %s", path, exc_info=True)
            return Exception(f"Could not load {path}") if not isinstance(e, ValueError) else e, meta

    def run(self, jobs):
        """jobs: [(file_idx, path)] -> {file_idx: document} (the files of this rank)."""
        if jobs and self.bird_models is None:  # examine() without models reads no audio
            from .analyse import read_sidecar, species_result
            return {i: dict(species_result(None, read_sidecar(p), self.analyse_tracks, False),
                            processing_time_seconds=0.0) for i, p in sorted(jobs)}
        return self._run(jobs)

    def _run(self, jobs):
        """The run loop (CiBatchAnalyser's too): the files K at a time, decoded
        ahead on the worker threads, each batch through process() on a lane."""
        import threading
        if not jobs:
            return {}
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
