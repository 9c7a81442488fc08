"""Time the old cacophony index on the device (aa_ci_run: ci_bands, ci_points)
against the reference's frame loop on this host.

    python tools/ci_bench.py [--seconds 60] [--batch 64] [--launches 30]

HIP events around each launch set, after warm-up; the median and the fastest:
  * one clip of `seconds` at 16 kHz,
  * a batch of `batch` such clips in one aa_ci_run,
  * 48 -> 16 kHz resampling (aa_resample_poly) plus the index on one clip.
The host figure is the reference's loop on one clip, single thread: numpy's
window product, scipy.fftpack.dct and Python's sum(x * x) per band, then the
comparisons (src/cacophony_index.py:53-97).  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "audio-analysis_amd"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))


def host_points(x, window, edges):
    import scipy.fftpack
    prev, points = None, []
    for off in range(1024, len(x) - 3072, 1024):
        dct = scipy.fftpack.dct(window * x[off:off + 2048])
        bins = np.array([sum(v * v) for v in np.split(dct, edges)[1:-1]])
        if prev is not None:
            points.append(sum(bins * 2 < prev) + sum(bins > prev * 2))
        prev = bins
    return points


def timed(launch, launches):
    import torch
    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for e0, e1 in ev:
        e0.record()
        launch()
        e1.record()
    torch.cuda.synchronize()
    ms = [e0.elapsed_time(e1) for e0, e1 in ev]
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--launches", type=int, default=30)
    a = ap.parse_args()

    import ctypes as C

    import torch

    from aa_amd import _lib
    from aa_amd import cacophony_index as ci
    from aa_amd.resample import resample_device
    from tools import synth

    if not torch.cuda.is_available():
        raise SystemExit("ci_bench needs a GPU")
    if not 1 <= a.batch <= ci.MAX_REC:
        raise SystemExit(f"--batch must be in 1..{ci.MAX_REC}")
    dev = torch.device("cuda:0")
    x16 = synth.clip(3, seconds=a.seconds, sr=ci.SAMPLE_RATE)
    x48 = synth.clip(3, seconds=a.seconds, sr=48000)
    n = len(x16)
    frames = ci.n_frames(n)
    out = {"samples_per_clip": n, "frames_per_clip": frames, "batch": a.batch, "launches": a.launches}

    window, edges = ci.window(), ci.band_edges()
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        ref = host_points(x16, window, edges)
        host.append((time.perf_counter() - t0) * 1e3)
    out["host_ms_per_clip"] = {"median": float(np.median(host)), "min": float(min(host))}

    d16 = torch.from_numpy(x16).to(dev)
    ws = torch.empty(a.batch * frames * ci.BANDS * 8, dtype=torch.uint8, device=dev)
    points_buf = torch.empty(a.batch * frames, dtype=torch.int32, device=dev)
    points, _ = ci.run_device(d16, [0], [n], workspace=ws)
    out["points_equal_host"] = points.cpu().numpy().tolist() == [int(p) for p in ref]
    L, plan = _lib.lib(), ci._plan(dev)

    def launcher(pcm, offsets, lengths):
        """aa_ci_run with its arguments made once: the timed region holds the
        call alone, not the Python that prepares it."""
        k = len(offsets)
        off, ln = (C.c_int64 * k)(*offsets), (C.c_int64 * k)(*lengths)
        args = (plan._h, _lib.dptr(pcm), off, ln, k, _lib.dptr(ws), int(ws.numel()), None, _lib.dptr(points_buf),
                _lib.stream_ptr())
        return lambda: _lib.check(L.aa_ci_run(*args), "aa_ci_run")

    out["gpu_ms_1_clip"] = timed(launcher(d16, [0], [n]), a.launches)

    batch = d16.repeat(a.batch)
    r = timed(launcher(batch, [k * n for k in range(a.batch)], [n] * a.batch), a.launches)
    r["frames_per_s"] = a.batch * frames / (r["median"] * 1e-3)
    out[f"gpu_ms_{a.batch}_clips"] = r

    d48 = torch.from_numpy(x48).to(dev)
    y = resample_device(d48, 48000, ci.SAMPLE_RATE)  # the filter bank is built and uploaded once
    buf = torch.empty_like(y)
    index = launcher(buf, [0], [int(buf.numel())])

    def resampled():
        resample_device(d48, 48000, ci.SAMPLE_RATE, out=buf)
        index()
    out["gpu_ms_resample_48k_plus_1_clip"] = timed(resampled, a.launches)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
