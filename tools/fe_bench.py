"""Time the front end's STFT + mel stage (fe_stft_mel_small, fe_stft_mel,
fe_stft_mel_4096) per configuration.

    python tools/fe_bench.py [--windows 64] [--seconds 3] [--runs 30] [--configs 256:64:80,...]

Per (n_fft, hop, n_mels): one aa_fe_run over `windows` windows of `seconds` at
48 kHz (htk filterbank, dB on, normalize on) per run, after warm-up; the stft
stage's HIP-event time from aa_fe_set_timing / aa_fe_stage_time, read back
after every run: the median and the fastest of `runs`, the time per frame and
the share of the FP32 vector peak that aa_fe_stage_info's flops reach in the
median.  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "audio-analysis_amd"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

CONFIGS = "256:64:80,512:128:80,1024:256:80,1024:256:160,2048:512:80,4096:640:160"
PEAK_F32_TFLOPS = 157.3  # MI355X FP32 vector peak
STFT_STAGE = 1


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--configs", default=CONFIGS)
    a = ap.parse_args()

    import torch

    from aa_amd.frontend import FeSettings, FrontEnd, pack_windows
    from tools import synth

    if not torch.cuda.is_available():
        raise SystemExit("fe_bench needs a GPU")
    dev = torch.device("cuda:0")
    win_len = int(synth.SR * a.seconds)
    stride = win_len // 2  # overlapping windows, as the scheduler lays them
    x = synth.clip(3, seconds=(stride * (a.windows - 1) + win_len) / synth.SR)
    pcm = torch.from_numpy(x).to(dev)
    views = [(i * stride, win_len, 0) for i in range(a.windows)]
    win = torch.from_numpy(pack_windows(views, len(x), win_len=win_len)).to(dev)
    out = {"windows": a.windows, "seconds": a.seconds, "runs": a.runs, "peak_f32_tflops": PEAK_F32_TFLOPS,
           "configs": []}
    for spec in a.configs.split(","):
        n_fft, hop, n_mels = (int(v) for v in spec.split(":"))
        s = FeSettings(sr=synth.SR, segment_length=a.seconds, n_fft=n_fft, hop_length=hop, n_mels=n_mels,
                       htk=True)
        fe = FrontEnd(s, dev)
        res = torch.empty(fe.out_shape(a.windows), dtype=torch.float32, device=dev)
        name, flops, _ = fe.stage_info(STFT_STAGE)
        for _ in range(a.warmup):
            fe.run(pcm, win, out=res)
        torch.cuda.synchronize()
        fe.set_timing(True, stages=[STFT_STAGE])
        ms = []
        for _ in range(a.runs):
            fe.run(pcm, win, out=res)
            torch.cuda.synchronize()
            total, count = fe.stage_time(STFT_STAGE)
            assert count == 1, count
            ms.append(total)
        fe.set_timing(False)
        med = float(np.median(ms))
        frames = a.windows * fe.T
        out["configs"].append({
            "n_fft": n_fft, "hop": hop, "n_mels": n_mels, "kernel": name, "frames": frames,
            "stft_us": {"median": med * 1e3, "min": float(min(ms)) * 1e3},
            "ns_per_frame": {"median": med * 1e6 / frames, "min": float(min(ms)) * 1e6 / frames},
            "tflops": flops * a.windows / (med * 1e-3) / 1e12,
            "share_of_f32_peak": flops * a.windows / (med * 1e-3) / 1e12 / PEAK_F32_TFLOPS,
        })
    print(json.dumps(out))


if __name__ == "__main__":
    main()
