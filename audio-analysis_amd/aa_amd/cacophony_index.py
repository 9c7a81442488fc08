"""The old cacophony index (reference src/cacophony_index.py), the frame loop
on the device.

``calculate(file)`` is the reference's entry point behind ``analyse.py
--old-cacophony-index``: decode, 16 kHz mono, 2048-sample frames at hop 1024,
Hann window, DCT-II, the energy of ten log-spaced bands, per pair of
neighbouring frames the number of bands that more than halved or doubled
(:53-97), then percentile scores over windows of 312 points (:69-125).  The
samples are uploaded once; resampling (``aa_resample_poly``), the float64
DCT bands and the points (``aa_ci_run``, csrc/aa_cacophony.hip) run on the
device; the points come back (one int per 64 ms) and the score table is
built here, operation by operation as the reference does.

The window and the band edges are numpy's own values, handed to the plan as
data.

Unpinned against the reference: it gets its 16 kHz samples from ``ffmpeg -ar
16000 -ac 1 -f f32le`` (libswresample's resampler and downmix).  A 16 kHz mono
PCM16 file yields exactly ffmpeg's samples here (x / 32768, no resampling);
any other rate goes through this build's soxr-HQ-specified filter
(aa_amd.resample) and stereo through the channel mean, whose parity with
libswresample is not pinned (no ffmpeg in this image).  ``.opus`` (the
reference's ``opusdec`` branch) is rejected with the other lossy codecs.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Sequence

import numpy

from . import _lib
from ._lib import AA_CI_BANDS as BANDS, AA_CI_HOP as HOP, AA_CI_MAX_REC as MAX_REC, AA_CI_N as WINDOW_SIZE

SAMPLE_RATE = 16000
BIN_20_WIDTH = 312  # ~20 seconds
VERSION = "2020-01-20_A"


def window() -> numpy.ndarray:
    """common.get_window_const(2048, "hanning"): numpy.hanning(2048) * 1.0."""
    return numpy.hanning(WINDOW_SIZE) * 1.0


def band_edges() -> numpy.ndarray:
    """get_ci_bins' edges (:58-63), numpy's integer truncation included."""
    bass_cut_off_frequency = 100
    bass_cut_off_band = bass_cut_off_frequency * 2 * WINDOW_SIZE // SAMPLE_RATE
    return numpy.logspace(math.log10(bass_cut_off_band), math.log10(WINDOW_SIZE), num=11, dtype=int)


def n_frames(n_samples: int) -> int:
    return int(_lib.lib().aa_ci_n_frames(int(n_samples)))


class Plan:
    """aa_ci_create (``host_only``: aa_ci_plan, the checks without a device)."""

    def __init__(self, win=None, edges=None, host_only: bool = False):
        w = numpy.ascontiguousarray(window() if win is None else win, dtype=numpy.float64)
        e = numpy.ascontiguousarray(band_edges() if edges is None else edges, dtype=numpy.int32)
        if w.shape != (WINDOW_SIZE,) or e.shape != (BANDS + 1,):
            raise ValueError(f"window {w.shape} / edges {e.shape}: need ({WINDOW_SIZE},) and ({BANDS + 1},)")
        self._h = C.c_void_p()
        fn = _lib.lib().aa_ci_plan if host_only else _lib.lib().aa_ci_create
        _lib.check(fn(w.ctypes.data, e.ctypes.data, C.byref(self._h)), "aa_ci_plan" if host_only else "aa_ci_create")

    def close(self) -> None:
        if self._h:
            _lib.lib().aa_ci_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_plans = {}


def _plan(device) -> Plan:
    key = str(device)
    if key not in _plans:
        _plans[key] = Plan()
    return _plans[key]


def run_device(pcm16k, offsets: Sequence[int], lengths: Sequence[int], want_bins: bool = False, workspace=None):
    """One ``aa_ci_run`` on the current stream over up to 64 recordings of the
    device f32 buffer ``pcm16k``.  Returns (points, bins): device int32
    [sum max(F_k - 1, 0)] and, when ``want_bins``, device float64 [sum F_k][10]
    (None otherwise: the energies stay in the workspace)."""
    import torch
    if pcm16k.dtype != torch.float32:
        raise _lib.AAError("the cacophony index needs float32 pcm")
    n_rec = len(offsets)
    if len(lengths) != n_rec:
        raise ValueError("offsets and lengths differ in length")
    total = int(pcm16k.numel())
    for o, n in zip(offsets, lengths):
        if o < 0 or n < 0 or o + n > total:
            raise ValueError(f"recording [{o}, {o + n}) is outside the {total} samples of pcm")
    frames = [n_frames(n) for n in lengths]
    rows, pts = sum(frames), sum(max(f - 1, 0) for f in frames)
    dev = pcm16k.device
    points_buf = torch.empty(max(pts, 1), dtype=torch.int32, device=dev)  # never a null pointer
    points = points_buf[:pts]
    bins =torch.empty((rows, BANDS), dtype=torch.float64, device=dev) if want_bins else None
    if n_rec == 0 or rows == 0:
        return points, bins
    off = (C.c_int64 * n_rec)(*map(int, offsets))
    ln = (C.c_int64 * n_rec)(*map(int, lengths))
    ws_ptr, ws_bytes = 0, 0
    if not want_bins:
        need = int(_lib.lib().aa_ci_workspace_bytes(ln, n_rec))
        if workspace is None:
            workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        ws_ptr, ws_bytes = _lib.dptr(workspace), int(workspace.numel())
    _lib.check(_lib.lib().aa_ci_run(_plan(dev)._h, _lib.dptr(pcm16k), off, ln, n_rec, ws_ptr, ws_bytes,
                                    _lib.dptr(bins) if want_bins else 0, _lib.dptr(points_buf),
                                    _lib.stream_ptr()), "aa_ci_run")
    return points, bins


def points_device(pcm16k_tensors) -> List[numpy.ndarray]:
    """The points of each recording of a batch (device f32 tensors of 16 kHz
    mono samples), 64 recordings per launch set."""
    import torch
    out: List[numpy.ndarray] = []
    tensors = list(pcm16k_tensors)
    for i in range(0, len(tensors), MAX_REC):
        group = [t.reshape(-1) for t in tensors[i:i + MAX_REC]]
        lengths = [int(t.numel()) for t in group]
        offsets = [0] * len(group)
        for k in range(1, len(group)):
            offsets[k] = offsets[k - 1] + lengths[k - 1]
        if sum(lengths) == 0:
            out.extend(numpy.zeros(0, numpy.int32) for _ in group)
            continue
        pcm = group[0] if len(group) == 1 else torch.cat(group)
        points, _ = run_device(pcm, offsets, lengths)
        host = points.cpu().numpy()
        pos = 0
        for n in lengths:
            k = max(n_frames(n) - 1, 0)
            out.append(host[pos:pos + k])
            pos += k
    return out


def score_from_points(points):
    points_sorted = sorted(points)
    k0 = int(len(points) * 0.75)
    k1 = int(len(points) * 0.95)
    return 10 * numpy.mean(points_sorted[k0:k1])


def apply_correction_curve_202001C(raw_score):
    s = raw_score - 10
    return max(100 * s / (s + 18), 0)


def score_table(points, n_samples: int) -> dict:
    """calculate's result document from the points (:99-125)."""
    points = list(points)
    half_window_size = WINDOW_SIZE // 2
    table = []
    entry_count = (len(points) + 31) // BIN_20_WIDTH
    for e in range(entry_count):
        q = 0
        if e:
            q = e * (len(points) - BIN_20_WIDTH) // (entry_count - 1)
        raw_score = score_from_points(points[q:q + BIN_20_WIDTH])
        score = apply_correction_curve_202001C(raw_score)
        entry = {}
        entry["begin_s"] = round(q * half_window_size / SAMPLE_RATE)
        entry["end_s"] = round((q + BIN_20_WIDTH) * half_window_size / SAMPLE_RATE)
        entry["index_percent"] = round(score, 1)
        table.append(entry)
    result = {}
    result["cacophony_index_old"] = table
    result["cacophony_index_old_version"] = VERSION
    if table == []:
        p = n_samples / SAMPLE_RATE
        result["ci_warning"] = (
            "Cacophony Index requires at least 20 seconds of audio, but only %d seconds of audio were provided."
            % p
        )
    return result


def load_16k_device(source_file_name, device=None):
    """The file's samples at 16 kHz mono as a device f32 tensor."""
    import torch
    from . import audio
    from .resample import resample_device
    if str(source_file_name).endswith(".opus"):
        raise ValueError(f"{source_file_name}: Opus needs a codec this build does not have")
    frames, sr = audio.decode(source_file_name)
    x = torch.from_numpy(frames).to(torch.device(device or "cuda"))
    if sr != SAMPLE_RATE:
        x = resample_device(x, sr, SAMPLE_RATE)
    return x


def calculate(source_file_name, device=None) -> dict:
    x = load_16k_device(source_file_name, device)
    points = points_device([x])[0]
    return score_table(points, int(x.numel()))
