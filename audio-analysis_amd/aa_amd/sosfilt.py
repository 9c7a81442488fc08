"""Band-pass filtered tracks on the device (aa_sosfilt_*, csrc/aa_sosfilt.hip).

The reference filters a track's whole sample range with scipy's ``sosfilt``
before it cuts the track's windows (src/identify_tracks.py:152-162,
:1036-1056).  ``windows.filtered_sources`` does that on the host and hands
back a buffer to upload; here the same selection becomes filter *jobs*
(struct aa_sos_job): the design of each filter stays on the host
(``windows.butter_bandpass``, a few dozen flops), the recurrence over the
samples runs in one ``aa_sosfilt_run`` that reads each span from the device
PCM buffer and writes the filtered copy behind it.
"""
from __future__ import annotations

import ctypes as C
from bisect import bisect_right
from typing import List, Sequence

import numpy as np

from . import _lib
from ._lib import AA_SOS_BLOCK as BLOCK, AA_SOS_CHUNK as CHUNK, AA_SOS_MAX_N as MAX_N, SosJob  # noqa: F401
from .windows import butter_bandpass


def plan_job(sos, src: int, n: int, dst: int) -> SosJob:
    """One job: ``pcm[src, src + n)`` through ``sos`` (scipy rows) into
    ``pcm[dst, dst + n)``; the state-transition powers are made on the host."""
    sos = np.ascontiguousarray(sos, dtype=np.float64)
    if sos.ndim != 2 or sos.shape[1] != 6:
        raise ValueError(f"sos must have shape (n_sections, 6), not {sos.shape}")
    job = SosJob()
    _lib.check(_lib.lib().aa_sosfilt_plan(sos.ctypes.data, int(sos.shape[0]), int(src), int(n), int(dst),
                                          C.byref(job)), "aa_sosfilt_plan")
    return job


def filtered_sources_device(pcm, n_pcm: int, rec_off: int, sr: int, tracks: Sequence, views, spans,
                            filter_freqs: bool, filter_below, base: int):
    """``windows.filtered_sources`` with the filtering left to the device.

    Same selection of tracks and the same remapped views (relative to the
    recording, filtered copies from ``base`` on); instead of the filtered
    samples it returns the jobs that make them: the recording starts at
    sample ``rec_off`` of the device buffer ``pcm`` (``n_pcm`` valid samples;
    ``pcm`` may be None when only planning), so a track span ``(a, b)`` is the
    job ``rec_off + a -> rec_off + base + ...`` of ``b - a`` samples.
    Returns (jobs, remapped views)."""
    if pcm is not None and int(pcm.numel()) < n_pcm:
        raise ValueError(f"pcm holds {int(pcm.numel())} samples, fewer than n_pcm = {n_pcm}")
    jobs: List[SosJob] = []
    out = []
    off = base
    for t, tv, (a, b) in zip(tracks, views, spans):
        if tv and (filter_freqs or (filter_below and t.freq_end < filter_below)):
            sos = butter_bandpass(t.freq_start, t.freq_end, sr)
            n = b - a
            if a < 0 or rec_off + b > n_pcm:
                raise ValueError(f"track span [{a}, {b}) at offset {rec_off} is outside the {n_pcm} samples of pcm")
            if n > 0:
                jobs.append(plan_job(sos, rec_off + a, n, rec_off + off))
            out.append([(off + (src - a), k, p) if k else (src, k, p) for (src, k, p) in tv])
            off += n
        else:
            out.append(tv)
    return jobs, out


def check_ranges(jobs: Sequence[SosJob], n_pcm: int) -> None:
    """The launch contract the host can see and the device cannot report:
    every range inside the buffer, no destination over a source or another
    destination."""
    dst = sorted((j.dst, j.dst + j.n) for j in jobs if j.n > 0)
    for j in jobs:
        if j.n < 0 or j.src < 0 or j.dst < 0 or j.src + j.n > n_pcm or j.dst + j.n > n_pcm:
            raise ValueError(f"sosfilt job src={j.src} dst={j.dst} n={j.n} is outside the {n_pcm} samples of pcm")
    for (_, e0), (b1, _) in zip(dst, dst[1:]):
        if b1 < e0:
            raise ValueError("sosfilt jobs write overlapping ranges")
    starts = [d[0] for d in dst]
    for j in jobs:
        if j.n > 0:
            k = bisect_right(starts, j.src + j.n - 1) - 1  # the last destination starting inside or before the source
            if k >= 0 and dst[k][1] > j.src:
                raise ValueError(f"sosfilt job src={j.src} n={j.n} is overwritten by a destination range")


def workspace_bytes(jobs: Sequence[SosJob]) -> int:
    if not jobs:
        return 0
    arr = (SosJob * len(jobs))(*jobs)
    return int(_lib.lib().aa_sosfilt_workspace_bytes(arr, len(jobs)))


def run(pcm, jobs: Sequence[SosJob], workspace=None) -> None:
    """All jobs in one launch set on the current stream, in place on the
    device f32 tensor ``pcm``."""
    import torch
    if not jobs:
        return
    if pcm.dtype != torch.float32:
        raise _lib.AAError("sosfilt needs float32 pcm")
    n_pcm = int(pcm.numel())
    check_ranges(jobs, n_pcm)
    arr = (SosJob * len(jobs))(*jobs)
    need = int(_lib.lib().aa_sosfilt_workspace_bytes(arr, len(jobs)))
    if workspace is None:
        workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=pcm.device)
    jobs_dev = torch.frombuffer(memoryview(arr).cast("B"), dtype=torch.uint8).to(pcm.device)
    _lib.check(_lib.lib().aa_sosfilt_run(_lib.dptr(pcm), n_pcm, _lib.dptr(jobs_dev), len(jobs),
                                         max(j.n for j in jobs), _lib.dptr(workspace), int(workspace.numel()),
                                         _lib.stream_ptr()), "aa_sosfilt_run")
    # jobs_dev (and an own workspace) die here: the caching allocator hands
    # their memory only to later work on this same stream
