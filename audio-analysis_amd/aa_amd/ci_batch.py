"""Batched old cacophony index: K recordings per GPU pass.

``analyse.py --old-cacophony-index FILE`` (reference src/cacophony_index.py)
is, per file, a host decode, one blocking upload, one ``aa_resample_poly`` and
one ``aa_ci_run`` over a single recording.  ``CiBatchAnalyser`` runs a rank's
files K at a time on the lanes, slot pool and decoders of ``aa_amd.batch``:

  * decode: a PCM16 WAV of any rate stays in its pinned slot as int16; FLAC,
    Ogg Vorbis and MP3 follow the ``flac`` / ``vorbis`` / ``mp3`` modes of
    ``BatchAnalyser`` (on the device into the int16 staging buffer, a file the
    device does not vouch for redone on the host); everything else goes
    through ``audio.decode`` to f32 at the file's rate;
  * to 16 kHz: one ``aa_resample_batch`` per distinct input rate of the batch
    (64 recordings per launch) reads the staging buffers and writes one 16 kHz
    buffer; recordings already at 16 kHz are widened (``aa_pcm_s16_to_f32``) or
    copied into it unfiltered;
  * index: one ``aa_ci_run`` per 64 recordings over that buffer, one readback
    of the points, ``cacophony_index.score_table`` per file on the host.

Each file's document is what ``cacophony_index.calculate(path)`` returns for
it alone (tests/test_gpu_ci_corpus.py) plus ``processing_time_seconds``; a
file that fails carries the exception ``calculate`` raises for it, and the
rest of its batch is unaffected.  No model is loaded.  Parity with the
reference's libswresample resampler and downmix stays unpinned, as in
``cacophony_index``.
"""
from __future__ import annotations

import ctypes as C
import logging
import time
from dataclasses import dataclass, field
from typing import List, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import AA_CI_MAX_REC as MAX_REC, AA_RS_F32, AA_RS_S16
from .batch import BatchAnalyser, decode_into, return_slots, split_items
from .cacophony_index import SAMPLE_RATE
from .resample import out_length


# ---- host-side planning (no device) ---------------------------------------
@dataclass
class Source:
    """Where one decoded recording sits: ``kind`` AA_RS_S16 (element ``off``
    of the int16 staging buffer, ``channels`` per frame) or AA_RS_F32 (element
    ``off`` of the f32 staging buffer), ``n_in`` frames at ``sr``."""
    kind: int
    off: int
    n_in: int
    channels: int
    sr: int


@dataclass
class Plan:
    """The 16 kHz buffer of a batch: recording k at ``offsets[k]``, ``lengths[k]``
    samples (``total`` in all); ``resample``: per input rate the launches of
    aa_resample_batch as lists of (recording, _lib.RsSegment), at most 64 each;
    ``direct``: the recordings already at 16 kHz; ``groups``: the recordings of
    each aa_ci_run, at most 64 each; ``points[k]``: the points recording k
    yields (max(aa_ci_n_frames - 1, 0)), in the order a run returns them."""
    offsets: List[int]
    lengths: List[int]
    total: int
    points: List[int] = field(default_factory=list)
    resample: List[Tuple[int, List[Tuple[int, object]]]] = field(default_factory=list)
    direct: List[int] = field(default_factory=list)
    groups: List[List[int]] = field(default_factory=list)


def plan_segments(sources: Sequence[Source], sr_out: int = SAMPLE_RATE, max_rec: int = MAX_REC) -> Plan:
    """Lay the recordings out back to back at ``sr_out`` (librosa's length,
    resample.out_length) and group them by what brings them there."""
    offsets, lengths, pos = [], [], 0
    by_rate, direct = {}, []
    for k, s in enumerate(sources):
        if s.kind not in (AA_RS_S16, AA_RS_F32) or s.n_in < 0 or s.off < 0 or s.sr <= 0:
            raise ValueError(f"recording {k}: bad source {s}")
        if s.kind == AA_RS_S16 and not 1 <= s.channels <= 8:
            raise ValueError(f"recording {k}: {s.channels} channels")
        n = s.n_in if s.sr == sr_out else out_length(s.n_in, s.sr, sr_out)
        offsets.append(pos)
        lengths.append(n)
        if s.sr == sr_out:
            direct.append(k)
        else:
            seg = _lib.RsSegment(src_off=s.off, n_in=s.n_in, dst_off=pos, n_out=n, kind=s.kind,
                                 channels=s.channels if s.kind == AA_RS_S16 else 1)
            by_rate.setdefault(int(s.sr), []).append((k, seg))
        pos += n
    from .cacophony_index import n_frames
    plan = Plan(offsets, lengths, pos, points=[max(n_frames(n) - 1, 0) for n in lengths], direct=direct)
    for sr, segs in by_rate.items():
        for i in range(0, len(segs), max_rec):
            plan.resample.append((sr, segs[i:i + max_rec]))
    idx = list(range(len(sources)))
    plan.groups = [idx[i:i + max_rec] for i in range(0, len(idx), max_rec)]
    return plan


def resample_batch(s16, f32, segments, sr_in: int, y, sr_out: int = SAMPLE_RATE, stream=None, segs_dev=None) -> None:
    """One aa_resample_batch: ``segments`` (_lib.RsSegment, at most 64) of the
    device int16 buffer ``s16`` / f32 buffer ``f32`` (either may be None) at
    ``sr_in`` into the device f32 buffer ``y`` at ``sr_out``."""
    import torch
    from .resample import _bank
    segments = list(segments)
    if not segments:
        return
    L, M, half, taps, bank = _bank(sr_in, sr_out, y.device)
    arr = (_lib.RsSegment * len(segments))(*segments)
    host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
    if segs_dev is None:
        segs_dev = torch.empty(host.numel(), dtype=torch.uint8, device=y.device)
    segs_dev[:host.numel()].copy_(host)
    _lib.check(_lib.lib().aa_resample_batch(
        _lib.dptr(s16) if s16 is not None and s16.numel() else 0, int(s16.numel()) if s16 is not None else 0,
        _lib.dptr(f32) if f32 is not None and f32.numel() else 0, int(f32.numel()) if f32 is not None else 0,
        _lib.dptr(segs_dev), len(segments), max(int(s.n_out) for s in segments), _lib.dptr(bank), L, M, taps, half,
        _lib.dptr(y), int(y.numel()), _lib.stream_ptr(stream)), "aa_resample_batch")


def _calculate_decode(path):
    """What cacophony_index.load_16k_device reads of a file, its failures included."""
    from . import audio
    if str(path).endswith(".opus"):
        raise ValueError(f"{path}: Opus needs a codec this build does not have")
    return audio.decode(path)


class CiBatchAnalyser(BatchAnalyser):
    """cacophony_index.calculate() for many files of one rank, K per device
    pass, ``lanes`` batches in flight (BatchAnalyser's run loop, decoders and
    slot pool; no classifier, no models)."""

    def __init__(self, device=None, batch=16, workers=8, lanes=2, flac=None, vorbis=None, mp3=None):
        import torch
        self._setup(device, batch, workers, lanes, flac, vorbis, mp3)
        if self.dev.index is None:  # (one spelling per device: it keys the index plan and the filter banks)
            self.dev = torch.device("cuda", torch.cuda.current_device())

    def run(self, jobs):
        from . import cacophony_index as ci
        if jobs:
            import torch
            with torch.cuda.device(self.dev):
                ci._plan(self.dev)  # made once, before the lane threads ask for it
        return self._run(jobs)

    def _load(self, path, pool):
        try:
            if str(path).endswith(".opus"):
                return _calculate_decode(path), None  # (raises)
            return decode_into(path, pool, self.codecs, sr_out=SAMPLE_RATE, wav_any_rate=True,
                               host_decode=_calculate_decode), None
        except Exception as e:
            try:  # the failure calculate() reports for this file, not the batched decoder's
                _calculate_decode(path)
            except Exception as e2:
                e = e2
            logging.error("Could not load %s", path, exc_info=True)
            return e, None

    def _redo_on_host(self, lane, bad, pcm, total):
        """The files of `bad` (device-decoded, not vouched for) through
        audio.decode: its samples, as f32 at the file's rate, or its failure
        then stand for the file."""
        for r in bad:
            d = r.dec
            try:
                frames, sr = _calculate_decode(d.path)
            except Exception as e:
                logging.error("Could not load %s", d.path, exc_info=True)
                r.err = e
                continue
            d.codec = d.index = None
            d.f32, d.sr_in, d.n_in = np.ascontiguousarray(frames, dtype=np.float32), int(sr), len(frames)
        return pcm, total

    def _to_16k(self, lane, recs):
        """The batch at 16 kHz mono in one device f32 buffer; returns (pcm, plan,
        the recordings the plan covers)."""
        import torch
        # (no f32 placement: pcm is laid out below, from the resample plan)
        _, s16, comp, _, cur = self._stage(lane, recs, f32=False)
        self._decode_compressed(lane, recs, comp, s16, cur)
        ok = [r for r in recs if r.err is None]
        # host-decoded samples (other WAV encodings, oversized files, redone files): one f32 staging buffer
        hf = [r for r in ok if r.dec.f32 is not None]
        f32 = lane.scratch("f32", sum(len(r.dec.f32) for r in hf), torch.float32) if hf else None
        of = 0
        for r in hf:
            n = len(r.dec.f32)
            if n:
                f32[of:of + n].copy_(torch.from_numpy(r.dec.f32), non_blocking=False)
            r.dec.of = of
            of += n
        plan = plan_segments([Source(AA_RS_F32, r.dec.of, len(r.dec.f32), 1, r.dec.sr_in) if r.dec.f32 is not None
                              else Source(AA_RS_S16, r.dec.o16, r.dec.n_in, r.dec.channels, r.dec.sr_in)
                              for r in ok])
        pcm, _ = lane.buffers(max(plan.total, 1), 0)
        L = _lib.lib()
        segs_dev = lane.scratch("segments", MAX_REC * C.sizeof(_lib.RsSegment), torch.uint8)
        for sr, segs in plan.resample:
            resample_batch(s16, f32, [s for _, s in segs], sr, pcm, stream=cur, segs_dev=segs_dev)
        for k in plan.direct:
            d, n = ok[k].dec, plan.lengths[k]
            if not n:
                continue
            if d.f32 is not None:
                pcm[plan.offsets[k]:plan.offsets[k] + n].copy_(f32[d.of:d.of + n])
            else:
                _lib.check(L.aa_pcm_s16_to_f32(_lib.dptr(s16) + 2 * d.o16, n, d.channels,
                                               _lib.dptr(pcm) + 4 * plan.offsets[k], _lib.stream_ptr(cur)),
                           "aa_pcm_s16_to_f32")
        return pcm, plan, ok

    def _index(self, lane, pcm, plan, recs):
        """aa_ci_run per 64 recordings, the points read back once per run and
        handed to each recording (_finish scores them)."""
        import torch
        from . import cacophony_index as ci
        pending = []
        for g in plan.groups:
            lengths = [plan.lengths[k] for k in g]
            need = int(_lib.lib().aa_ci_workspace_bytes((C.c_int64 * len(g))(*lengths), len(g)))
            ws = lane.scratch("ci_ws", max(need, 1), torch.uint8)
            points, _ = ci.run_device(pcm, [plan.offsets[k] for k in g], lengths, workspace=ws)
            pending.append((g, lengths, points.cpu().numpy()))  # (before the next group reuses the workspace)
        for g, lengths, host in pending:
            pos = 0
            for k, n in zip(g, lengths):
                c = plan.points[k]
                recs[k].res = (host[pos:pos + c], n)  # (scored in _finish, with the documents)
                pos += c

    def _finish(self, recs, t0):
        from .cacophony_index import score_table
        from .corpus import FAILED
        out = {}
        dt = round((time.time() - t0) / max(len(recs), 1), 1)
        for r in recs:
            if r.err is not None:
                logging.error("%s: %s", r.path, r.err)
                out[r.idx] = {FAILED: f"{type(r.err).__name__}: {r.err}"}
                continue
            doc = score_table(*r.res)
            doc["processing_time_seconds"] = dt
            out[r.idx] = doc
        return out

    def process(self, items, lane, pool=None):
        """items: [(file_idx, path, Decoded | Exception, None)] -> {file_idx: document}."""
        import torch
        t0 = time.time()
        recs, failed = split_items(items)
        ok = []
        if recs:
            try:
                with torch.cuda.stream(lane.stream):
                    tm = self.timing
                    t = time.perf_counter()
                    pcm, plan, ok = self._to_16k(lane, recs)
                    t = tm.lap("to_16k", t)
                    failed += [r for r in recs if r.err is not None]
                    self._index(lane, pcm, plan, ok)
                    lane.stream.synchronize()  # every copy out of the slots has landed before they go back
                    tm.lap("index", t)
            finally:
                return_slots(pool, recs)
        t = time.perf_counter()
        docs = self._finish(ok + failed, t0)
        self.timing.lap("post", t)
        return docs
