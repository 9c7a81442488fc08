"""Time the front end's STFT + mel stage (fe_stft_mel_small, fe_stft_mel,
fe_stft_mel_4096, fe_stft_mel_mixed) per configuration, and state its error.

    python tools/fe_bench.py [--windows 64] [--seconds 3] [--runs 30] [--rounds 1]
                             [--configs 256:64:80,4800:640:160,4096:640:160:full,...]

Per n_fft:hop:n_mels[:full] -- any n_fft the front end accepts, the powers of
two and the multiples of 16 with factors 2, 3, 5 (4800, 2400, 1200); `full`
spreads the bands over 0 Hz .. Nyquist instead of 50 .. 11000 Hz, which at
4096 selects fe_stft_mel over the wave-per-frame kernel: one aa_fe_run over
`windows` windows of `seconds` at 48 kHz (htk filterbank, dB on, normalize on)
per run, after warm-up; the stft stage's HIP-event time from aa_fe_set_timing
/ aa_fe_stage_time, read back after every run: the median and the fastest of
`runs` x `rounds`, the time per frame and the share of the FP32 vector peak
that aa_fe_stage_info's flops reach in the median.  With `rounds` > 1 the
list is walked forwards and backwards in turn, so that no configuration
always follows the same neighbour.  The error column is the largest
|log-mel - float64 oracle| in dB over the first window.  Prints one JSON line.
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

CONFIGS = ("256:64:80,512:128:80,1024:256:80,1024:256:160,2048:512:80,4096:640:160,"
           "1200:300:80,2400:600:80,4800:640:160")
PEAK_F32_TFLOPS = 157.3  # MI355X FP32 vector peak
STFT_STAGE = 1


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--configs", default=CONFIGS)
    a = ap.parse_args()

    import torch

    from aa_amd.frontend import FeSettings, FrontEnd, pack_windows
    from oracle import fe_oracle
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
    out = {"windows": a.windows, "seconds": a.seconds, "runs": a.runs, "rounds": a.rounds,
           "peak_f32_tflops": PEAK_F32_TFLOPS, "configs": []}
    ends, times, errs = [], [], []
    for spec in a.configs.split(","):
        f = spec.split(":")
        n_fft, hop, n_mels = (int(v) for v in f[:3])
        band = dict(fmin=0, fmax=synth.SR // 2) if f[3:] == ["full"] else {}
        s = FeSettings(sr=synth.SR, segment_length=a.seconds, n_fft=n_fft, hop_length=hop, n_mels=n_mels,
                       htk=True, **band)
        fe = FrontEnd(s, dev)
        res = torch.empty(fe.out_shape(a.windows), dtype=torch.float32, device=dev)
        for _ in range(a.warmup):
            fe.run(pcm, win, out=res)
        torch.cuda.synchronize()
        cfg = dict(sr=s.sr, hop_length=s.hop_length, n_mels=s.n_mels, fmin=s.fmin, fmax=s.fmax, n_fft=s.n_fft,
                   power=s.power, db_scale=s.db_scale, htk=s.htk, break_freq=s.break_freq, normalize=s.normalize,
                   mean_sub=s.mean_sub, channels=s.channels)
        errs.append(float(np.abs(res[0].cpu().numpy() - fe_oracle.window_logmel(x[:win_len], cfg)).max()))
        ends.append((spec, fe, res))
        times.append([])
    for rd in range(a.rounds):
        order = range(len(ends)) if rd % 2 == 0 else reversed(range(len(ends)))
        for i in order:
            _, fe, res = ends[i]
            fe.run(pcm, win, out=res)  # (the round's own warm-up after another configuration)
            torch.cuda.synchronize()
            fe.set_timing(True, stages=[STFT_STAGE])
            for _ in range(a.runs):
                fe.run(pcm, win, out=res)
                torch.cuda.synchronize()
                total, count = fe.stage_time(STFT_STAGE)
                assert count == 1, count
                times[i].append(total)
            fe.set_timing(False)
    for (spec, fe, _), ms, err in zip(ends, times, errs):
        name, flops, _ = fe.stage_info(STFT_STAGE)
        med = float(np.median(ms))
        frames = a.windows * fe.T
        out["configs"].append({
            "config": spec, "n_fft": fe.s.n_fft, "hop": fe.s.hop_length, "n_mels": fe.s.n_mels, "kernel": name,
            "frames": frames,
            "stft_us": {"median": med * 1e3, "min": float(min(ms)) * 1e3},
            "ns_per_frame": {"median": med * 1e6 / frames, "min": float(min(ms)) * 1e6 / frames},
            "tflops": flops * a.windows / (med * 1e-3) / 1e12,
            "share_of_f32_peak": flops * a.windows / (med * 1e-3) / 1e12 / PEAK_F32_TFLOPS,
            "logmel_err_db": err,
        })
    print(json.dumps(out))


if __name__ == "__main__":
    main()
