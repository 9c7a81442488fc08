"""Time the old cacophony index on the device (aa_ci_run: ci_bands, ci_points)
against the reference's frame loop on this host.

    python tools/ci_bench.py [--seconds 60] [--batch 64] [--launches 30]
                             [--resample-batch] [--corpus N] [--out PATH]

HIP events around each launch set, after warm-up; the median and the fastest:
  * one clip of `seconds` at 16 kHz,
  * a batch of `batch` such clips in one aa_ci_run,
  * 48 -> 16 kHz resampling (aa_resample_poly) plus the index on one clip.
The host figure is the reference's loop on one clip, single thread: numpy's
window product, scipy.fftpack.dct and Python's sum(x * x) per band, then the
comparisons (src/cacophony_index.py:53-97).  Prints one JSON line.

--resample-batch: aa_resample_batch over 16 staged int16 clips of `seconds`
in one launch against the two-step way on the same buffers, 16 x
(aa_pcm_s16_to_f32 + aa_resample_poly), from 48, 44.1 and 96 kHz to 16 kHz;
the outputs are compared bit for bit first.
--corpus N: N files of `seconds` as 48 kHz PCM16 WAV, then as MP3 with
mp3="gpu": corpus.run(old_cacophony_index=True) against a loop of
cacophony_index.calculate in the same process, three alternating pairs after
one warm-up pair; and one CiBatchAnalyser run's phase times (wall and CPU time
of the lane threads: wait_decode, to_16k, index, post).
--out PATH: the JSON line also goes to PATH.
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


def spread(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "n": len(v)}


def resample_batch_bench(dev, seconds, launches, clips=16):
    """{rate: timings} of one aa_resample_batch against clips x the two-step path."""
    import torch

    from aa_amd import _lib
    from aa_amd.ci_batch import resample_batch
    from aa_amd.resample import _bank, out_length
    from tools import synth
    L = _lib.lib()
    out = {}
    for sr in (48000, 44100, 96000):
        x = synth.clip(5, seconds=seconds, sr=sr)
        q = torch.from_numpy(np.round(x * 32768.0).astype(np.int16))
        n_in, n_out = int(q.numel()), out_length(int(q.numel()), sr, 16000)
        s16 = q.repeat(clips).to(dev)
        tmp = torch.empty(n_in, dtype=torch.float32, device=dev)
        y_two = torch.zeros(clips * n_out, dtype=torch.float32, device=dev)
        y_one = torch.ones(clips * n_out, dtype=torch.float32, device=dev)
        Lr, M, half, taps, bank = _bank(sr, 16000, dev)
        segs = [_lib.RsSegment(src_off=k * n_in, n_in=n_in, dst_off=k * n_out, n_out=n_out, kind=_lib.AA_RS_S16,
                               channels=1) for k in range(clips)]
        segs_dev = torch.empty(clips * 40, dtype=torch.uint8, device=dev)
        resample_batch(s16, None, segs, sr, y_one, segs_dev=segs_dev)  # (uploads the table once)
        st = _lib.stream_ptr()
        one_args = (_lib.dptr(s16), int(s16.numel()), None, 0, _lib.dptr(segs_dev), clips, n_out, _lib.dptr(bank), Lr,
                    M, taps, half, _lib.dptr(y_one), int(y_one.numel()), st)

        def one():
            _lib.check(L.aa_resample_batch(*one_args), "aa_resample_batch")

        def two():
            for k in range(clips):
                _lib.check(L.aa_pcm_s16_to_f32(_lib.dptr(s16) + 2 * k * n_in, n_in, 1, _lib.dptr(tmp), st), "widen")
                _lib.check(L.aa_resample_poly(_lib.dptr(tmp), n_in, _lib.dptr(bank), Lr, M, taps, half,
                                              _lib.dptr(y_two) + 4 * k * n_out, n_out, st), "aa_resample_poly")

        one()
        two()
        torch.cuda.synchronize()
        r = {"clips": clips, "n_in": n_in, "n_out": n_out, "L": Lr, "M": M, "taps": taps,
             "bit_equal": bool(torch.equal(y_one.view(torch.int32), y_two.view(torch.int32))),
             "two_step_ms": timed(two, launches), "batch_ms": timed(one, launches)}
        r["speedup_median"] = r["two_step_ms"]["median"] / r["batch_ms"]["median"]
        r["gfma_per_s_batch"] = clips * n_out * taps / (r["batch_ms"]["median"] * 1e-3) / 1e9
        out[str(sr)] = r
    return out


def corpus_bench(dev, seconds, n_files, pairs=3):
    """Batched corpus runs of the index against the per-file loop, WAV and MP3 (mp3="gpu")."""
    import tempfile

    from aa_amd import cacophony_index as ci
    from aa_amd import corpus
    from aa_amd.ci_batch import CiBatchAnalyser
    from tools import synth
    from tools.mp3_bench import make_clip
    out = {}
    with tempfile.TemporaryDirectory() as td:
        td = Path(td)
        kinds = {"wav": [], "mp3": []}
        mp3 = make_clip(seconds)
        for k in range(n_files):
            p = td / f"c{k}.wav"
            synth.write_wav(p, synth.clip(100 + k % 8, seconds=seconds, sr=48000), sr=48000)
            kinds["wav"].append(str(p))
            p = td / f"c{k}.mp3"
            p.write_bytes(mp3)
            kinds["mp3"].append(str(p))
        for kind, files in kinds.items():
            loop, batched, same = [], [], True
            for rnd in range(pairs + 1):  # the first pair warms both paths up (pinned slots, banks, plans)
                t0 = time.perf_counter()
                single = {k: ci.calculate(f) for k, f in enumerate(files)}
                t1 = time.perf_counter()
                res = corpus.run(files, None, mp3="gpu", old_cacophony_index=True)
                t2 = time.perf_counter()
                same &= all({kk: v for kk, v in res[k].items() if kk != "processing_time_seconds"} == single[k]
                            for k in single)
                if rnd:
                    loop.append((t1 - t0) * 1e3)
                    batched.append((t2 - t1) * 1e3)
            ba = CiBatchAnalyser(device=dev, batch=16, lanes=corpus.default_lanes(), mp3="gpu")
            t0 = time.perf_counter()
            ba.run(list(enumerate(files)))
            wall = (time.perf_counter() - t0) * 1e3
            out[kind] = {"files": n_files, "documents_equal": bool(same), "loop_ms": spread(loop),
                         "batched_ms": spread(batched),
                         "speedup_median": float(np.median(loop) / np.median(batched)),
                         "phases": {"wall_ms": wall, "lanes": min(ba.n_lanes, -(-n_files // 16)),
                                    "lane_wall_ms": {k: 1e3 * v for k, v in ba.timing.t.items()},
                                    "lane_cpu_ms": {k: 1e3 * v for k, v in ba.timing.cpu.items()}}}
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--resample-batch", action="store_true")
    ap.add_argument("--corpus", type=int, default=0, help="files of the corpus comparison (0: skip)")
    ap.add_argument("--out", default=None, help="also write the JSON line here")
    a = ap.parse_args()
    if a.corpus:
        from aa_amd.corpus import raise_hw_queues
        raise_hw_queues()  # as python -m aa_amd.corpus does, before the first GPU call

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
    if a.resample_batch:
        out["resample_batch"] = resample_batch_bench(dev, a.seconds, a.launches)
    if a.corpus:
        out["corpus"] = corpus_bench(dev, a.seconds, a.corpus)
    print(json.dumps(out))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
