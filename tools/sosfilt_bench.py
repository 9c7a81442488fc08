"""Time the device band-pass filter (aa_sosfilt_run: sos_local, sos_carry,
sos_output) against scipy's sosfilt on this host.

    python tools/sosfilt_bench.py [--seconds 60] [--tracks 1,16] [--launches 30]

Per track count: HIP events around each aa_sosfilt_run over `tracks` spans of
`seconds` at 48 kHz (band-pass 800-3000 Hz, two sections), after warm-up; the
median and the fastest launch.  scipy.signal.sosfilt is timed on one such span
(float32 in, float64 arithmetic, as windows.filtered_sources calls it).
Prints one JSON line.
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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--tracks", default="1,16")
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--band", default="800,3000")
    a = ap.parse_args()

    import torch
    from scipy.signal import sosfilt as scipy_sosfilt

    from aa_amd import _lib, sosfilt
    from aa_amd.windows import butter_bandpass
    from tools import synth

    if not torch.cuda.is_available():
        raise SystemExit("sosfilt_bench needs a GPU")
    dev = torch.device("cuda:0")
    f0, f1 = (float(v) for v in a.band.split(","))
    sos = butter_bandpass(f0, f1, synth.SR)
    x = synth.clip(3, seconds=a.seconds)
    n = len(x)
    out = {"samples_per_track": n, "band_hz": [f0, f1], "sections": int(len(sos)), "launches": a.launches,
           "chunk": sosfilt.CHUNK, "block": sosfilt.BLOCK}

    host = []
    for _ in range(5):
        t0 = time.perf_counter()
        y = scipy_sosfilt(sos, x).astype(np.float32)
        host.append((time.perf_counter() - t0) * 1e3)
    out["scipy_ms_per_track"] = {"median": float(np.median(host)), "min": float(min(host))}

    L = _lib.lib()
    for tracks in (int(t) for t in a.tracks.split(",")):
        pcm = torch.empty(2 * tracks * n, dtype=torch.float32, device=dev)
        pcm[:tracks * n] = torch.from_numpy(x).to(dev).repeat(tracks)
        jobs = [sosfilt.plan_job(sos, k * n, n, (tracks + k) * n) for k in range(tracks)]
        sosfilt.check_ranges(jobs, int(pcm.numel()))
        arr = (_lib.SosJob * tracks)(*jobs)
        need = int(L.aa_sosfilt_workspace_bytes(arr, tracks))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        jobs_dev = torch.frombuffer(memoryview(arr).cast("B"), dtype=torch.uint8).to(dev)

        def launch():
            _lib.check(L.aa_sosfilt_run(_lib.dptr(pcm), int(pcm.numel()), _lib.dptr(jobs_dev), tracks, n,
                                        _lib.dptr(ws), need, _lib.stream_ptr()), "aa_sosfilt_run")
        for _ in range(5):
            launch()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
              for _ in range(a.launches)]
        for e0, e1 in ev:
            e0.record()
            launch()
            e1.record()
        torch.cuda.synchronize()
        ms = [e0.elapsed_time(e1) for e0, e1 in ev]
        got = pcm[tracks * n:(tracks + 1) * n].cpu().numpy()
        out[f"gpu_ms_{tracks}_tracks"] = {"median": float(np.median(ms)), "min": float(min(ms)),
                                          "max": float(max(ms)),
                                          "samples_per_s": tracks * n / (float(np.median(ms)) * 1e-3)}
        out[f"mismatch_share_{tracks}_tracks"] = float(np.mean(got != y))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
