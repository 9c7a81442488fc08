"""Time FLAC decode on the device (aa_flac_decode_device) against the host
route (aa_flac_decode on one thread) and, optionally, a FLAC corpus through
the batched path in both modes.

    python tools/flac_bench.py [--seconds 60] [--encode-seconds 6] [--clips 1,16,64] [--launches 30]
                               [--clip-file F.flac] [--corpus FILES --pairs 5]

The clip: a tools/synth signal on the PCM16 grid, mono 48 kHz, encoded by the
test encoder (tests/flac_writer.py) as a common encoder would (LPC order 8,
4096-sample blocks, partition order 4).  That encoder is Python; by default
only --encode-seconds distinct seconds are encoded and their frames repeated
with fresh frame numbers (header CRC-8 and frame CRC-16 redone) up to
--seconds; the output says so ("distinct_seconds").  --clip-file caches the
stream.

Per clip count N, HIP events around `launches` repetitions after warm-up,
medians with min and max:
  device_path   N clips' compressed bytes and frame table from pinned memory,
                aa_flac_decode_device, aa_pcm_s16_to_f32
  decode_kernel aa_flac_decode_device alone;  widen_kernel: aa_pcm_s16_to_f32 alone
and on this host, one thread, per clip: the index pass (flac_gpu.index) and
the host route the corpus path takes today (audio.decode_flac, the numpy
conversion to mono float32, the blocking upload of the float32 samples).

--corpus FILES: FILES copies of the clip through BatchAnalyser(flac="host")
and (flac="gpu") in --pairs alternating pairs after a warm-up run of each;
wall seconds per run, medians and spread.  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "audio-analysis_amd", ROOT / "tests"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))


def _crc16_fast(data: bytes, _tab=[]) -> int:
    if not _tab:
        for i in range(256):
            c = i << 8
            for _ in range(8):
                c = ((c << 1) ^ 0x8005) & 0xFFFF if c & 0x8000 else (c << 1) & 0xFFFF
            _tab.append(c)
    c = 0
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ _tab[(c >> 8) ^ b]
    return c


def make_clip(seconds: float, distinct: float) -> bytes:
    import flac_writer as fw
    from tools import synth
    block = 4096
    y = np.round(synth.clip(7, seconds=min(distinct, seconds)) * 32768).clip(-32768, 32767).astype(np.int64)
    y = y[:len(y) // block * block]
    kind = {"kind": "lpc", "order": 8, "porder": 4}
    frames = [fw.frame([y[i:i + block]], 16, 48000, k, kinds=[kind]) for k, i in enumerate(range(0, len(y), block))]
    want = int(round(seconds * 48000)) // block
    out = []
    for k in range(want):
        f = frames[k % len(frames)]
        if k >= len(frames):  # the same samples under frame number k
            old = 4 + len(fw._utf8(k % len(frames))) + 1
            head = f[:4] + fw._utf8(k)
            f = head + bytes([fw.crc8(head)]) + f[old:-2]
            f += _crc16_fast(f).to_bytes(2, "big")
        out.append(f)
    return fw.stream(out, 48000, 1, 16, want * block, block)


def _stats(ms):
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}


def _events(fn, launches, torch):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return _stats([e0.elapsed_time(e1) for e0, e1 in ev])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--encode-seconds", type=float, default=6.0)
    ap.add_argument("--clips", default="1,16,64")
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--clip-file", default=None)
    ap.add_argument("--corpus", type=int, default=0)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    a = ap.parse_args()

    import torch

    from aa_amd import _lib, audio, flac_gpu
    from aa_amd.corpus import raise_hw_queues

    raise_hw_queues()  # as corpus.main and bench.py do, before the first GPU call
    if not torch.cuda.is_available():
        raise SystemExit("flac_bench needs a GPU")
    dev = torch.device("cuda:0")
    if a.clip_file and os.path.exists(a.clip_file):
        data = Path(a.clip_file).read_bytes()
    else:
        data = make_clip(a.seconds, a.encode_seconds)
        if a.clip_file:
            Path(a.clip_file).write_bytes(data)
    info, tab = flac_gpu.index(data)
    n = info.total_frames
    out = {"samples_per_clip": n, "compressed_bytes_per_clip": len(data), "frames_per_clip": len(tab),
           "distinct_seconds": min(a.encode_seconds, a.seconds) if not a.clip_file else "see --clip-file",
           "launches": a.launches, "workgroup_frames": flac_gpu.WG}
    L = _lib.lib()

    # ---- this host, one thread, per clip
    t_idx, t_dec, t_np, t_up = [], [], [], []
    buf = np.frombuffer(data, np.uint8)
    for _ in range(5):
        t0 = time.perf_counter()
        flac_gpu.index(buf)
        t1 = time.perf_counter()
        q, ch, sr = audio.decode_flac(data)
        t2 = time.perf_counter()
        f32 = audio._to_mono(q, ch)
        t3 = time.perf_counter()
        d = torch.empty(len(f32), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        d.copy_(torch.from_numpy(f32), non_blocking=False)
        torch.cuda.synchronize()
        t5 = time.perf_counter()
        t_idx.append((t1 - t0) * 1e3)
        t_dec.append((t2 - t1) * 1e3)
        t_np.append((t3 - t2) * 1e3)
        t_up.append((t5 - t4) * 1e3)
    out["host_index_ms_per_clip"] = _stats(t_idx)
    out["host_route_ms_per_clip"] = {"aa_flac_decode_and_s16": _stats(t_dec), "numpy_to_mono_f32": _stats(t_np),
                                     "blocking_upload_f32": _stats(t_up),
                                     "median_total": float(np.median(t_dec) + np.median(t_np) + np.median(t_up))}
    ref16 = q.astype(np.int16)

    # ---- the device
    for N in (int(c) for c in a.clips.split(",")):
        tabN = flac_gpu.concat([tab] * N, [k * len(data) for k in range(N)], [k * n for k in range(N)])
        comp_pin = torch.from_numpy(np.tile(buf, N)).pin_memory()
        tab_pin = torch.from_numpy(tabN.view(np.uint8).reshape(-1).copy()).pin_memory()
        comp = torch.empty_like(comp_pin, device=dev)
        tab_dev = torch.empty_like(tab_pin, device=dev)
        s16 = torch.empty(N * n, dtype=torch.int16, device=dev)
        pcm = torch.empty(N * n, dtype=torch.float32, device=dev)
        status = torch.empty(len(tabN), dtype=torch.int32, device=dev)
        ws = torch.empty(max(flac_gpu.workspace_bytes(tabN) // 4, 1), dtype=torch.int32, device=dev)

        def upload():
            comp.copy_(comp_pin, non_blocking=True)
            tab_dev.copy_(tab_pin, non_blocking=True)

        def decode():
            flac_gpu.decode_device(comp, tab_dev, len(tabN), status, ws, out_s16=s16)

        def widen():
            _lib.check(L.aa_pcm_s16_to_f32(_lib.dptr(s16), N * n, 1, _lib.dptr(pcm), _lib.stream_ptr()), "widen")

        def path():
            upload()
            decode()
            widen()

        r = {"device_path_ms": _events(path, a.launches, torch), "decode_kernel_ms": _events(decode, a.launches, torch),
             "widen_kernel_ms": _events(widen, a.launches, torch), "upload_ms": _events(upload, a.launches, torch),
             "workspace_mib": ws.numel() * 4 / 2 ** 20}
        r["device_path_ms_per_clip"] = r["device_path_ms"]["median"] / N
        r["samples_per_s_decode_kernel"] = N * n / (r["decode_kernel_ms"]["median"] * 1e-3)
        r["status_all_ok"] = not bool(status.count_nonzero())
        r["s16_equal_to_host_decoder"] = bool(np.array_equal(s16[(N - 1) * n:].cpu().numpy(), ref16))
        out[f"clips_{N}"] = r
        del comp_pin, tab_pin, comp, tab_dev, s16, pcm, status, ws

    # ---- a FLAC corpus through the batched path, both modes, alternating
    if a.corpus:
        from aa_amd.batch import BatchAnalyser
        from aa_amd.corpus import default_lanes
        from tools.make_models import make_ensemble
        with tempfile.TemporaryDirectory() as td:
            td = Path(td)
            make_ensemble(td / "models")
            models = [str(td / "models" / m / "audioModel.keras") for m in ("model1", "model2")]
            first = td / "c0.flac"
            first.write_bytes(data)
            jobs = [(0, str(first))]
            for k in range(1, a.corpus):
                p = td / f"c{k}.flac"
                try:
                    os.link(first, p)
                except OSError:
                    p.write_bytes(data)
                jobs.append((k, str(p)))
            ba = {m: BatchAnalyser(models, False, device=dev, batch=a.batch, lanes=default_lanes(), flac=m)
                  for m in ("host", "gpu")}
            docs = {}
            for m in ("host", "gpu"):  # warm-up: pinned slots, workspaces, kernels
                docs[m] = ba[m].run(jobs)
            strip = lambda r: json.dumps({k: {kk: vv for kk, vv in v.items() if kk != "processing_time_seconds"}
                                          for k, v in r.items()}, sort_keys=True)
            secs = {"host": [], "gpu": []}
            for _ in range(a.pairs):
                for m in ("host", "gpu"):
                    t0 = time.perf_counter()
                    ba[m].run(jobs)
                    secs[m].append(time.perf_counter() - t0)
            audio_s = a.corpus * n / 48000.0
            med = {m: float(np.median(v)) for m, v in secs.items()}
            out["corpus"] = {
                "files": a.corpus, "audio_seconds": audio_s, "batch": a.batch, "lanes": default_lanes(),
                "pairs": a.pairs, "documents_equal": strip(docs["host"]) == strip(docs["gpu"]),
                "seconds": secs, "median_seconds": med,
                "audio_s_per_s": {m: audio_s / med[m] for m in med},
                "spread": {m: (max(v) - min(v)) / med[m] for m, v in secs.items()},
                "gpu_gain": med["host"] / med["gpu"] - 1.0}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
