"""Time MP3 decode on the device (aa_mp3_decode_device) against the host
route (aa_mp3_decode on one thread) and, optionally, an MP3 corpus through the
batched path in both modes.

    python tools/mp3_bench.py [--seconds 60] [--clips 1,16] [--launches 20] [--corpus FILES --pairs 5]

The clip: the 21 audio frames of tests/golden/mp3/invalid_keypress.mp3
(libmp3lame: real entropy statistics, every block type, the bit reservoir;
the first frame has main_data_begin 0, so the block can follow itself) tiled
up to --seconds, without the Info frame (nothing is trimmed).  The output
says how many distinct frames there are ("distinct_frames").

Per clip count N, HIP events around `launches` repetitions after warm-up,
medians with min and max:
  device_path   N clips' main data and tables from pinned memory,
                aa_mp3_decode_device (unpack, hybrid, synth + s16),
                aa_pcm_s16_to_f32
  decode_ms     aa_mp3_decode_device alone;  widen_ms: aa_pcm_s16_to_f32 alone
and on this host, one thread, per clip: the index pass (mp3_gpu.index) and the
host route the corpus path takes by default (audio.decode_mp3, the numpy
conversion to s16 and mono float32, the blocking upload of the float32
samples).

--corpus FILES: FILES copies of the clip through BatchAnalyser(mp3="host") and
(mp3="gpu") in --pairs alternating pairs after a warm-up run of each; wall
seconds per run, medians and spread.  Prints one JSON line.
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

REAL = ROOT / "tests" / "golden" / "mp3" / "invalid_keypress.mp3"


def make_clip(seconds: float) -> bytes:
    """The fixture's audio frames (behind its ID3v2 tag and Info frame), tiled."""
    data = REAL.read_bytes()
    tag = 10 + ((data[6] << 21) | (data[7] << 14) | (data[8] << 7) | data[9])
    kbps = (0, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320)[data[tag + 2] >> 4]
    info_len = 144000 * kbps // 44100 + ((data[tag + 2] >> 1) & 1)
    audio = data[tag + info_len:]
    assert audio[:2] == b"\xff\xfb"
    tiles = max(1, int(np.ceil(seconds * 44100 / (21 * 1152))))
    return audio * tiles


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
    ap.add_argument("--clips", default="1,16")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--corpus", type=int, default=0)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    a = ap.parse_args()
    data = make_clip(a.seconds)

    import torch

    from aa_amd import _lib, audio, mp3_gpu as mg
    from aa_amd.corpus import raise_hw_queues

    raise_hw_queues()  # as corpus.main and bench.py do, before the first GPU call
    if not torch.cuda.is_available():
        raise SystemExit("mp3_bench needs a GPU")
    dev = torch.device("cuda:0")
    ix = mg.index(data)
    if ix is None:
        raise SystemExit("the clip is not indexable")
    st = ix.stream[0]
    n, ch = int(st["frames"]), int(st["channels"])
    out = {"frames_per_clip": n, "channels": ch, "sample_rate": int(st["sample_rate"]),
           "file_bytes_per_clip": len(data), "mp3_frames_per_clip": len(ix.frames),
           "payload_bytes_per_clip": int(ix.payload.size), "distinct_frames": 21, "launches": a.launches,
           "workgroup_lanes": mg.WG}
    L = _lib.lib()

    # ---- this host, one thread, per clip
    t_idx, t_dec, t_np, t_up = [], [], [], []
    buf = np.frombuffer(data, np.uint8)
    for _ in range(3):
        t0 = time.perf_counter()
        mg.index(buf)
        t1 = time.perf_counter()
        f, c, sr = audio.decode_mp3(data)
        t2 = time.perf_counter()
        q = audio._float_to_s16(f)
        f32 = audio._to_mono(q, c)
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
    out["host_route_ms_per_clip"] = {"aa_mp3_decode": _stats(t_dec), "numpy_s16_and_mono_f32": _stats(t_np),
                                     "blocking_upload_f32": _stats(t_up),
                                     "median_total": float(np.median(t_dec) + np.median(t_np) + np.median(t_up))}
    ref16 = q.astype(np.int16)

    # ---- the device
    mg.tables_device(dev)
    for N in (int(c) for c in a.clips.split(",")):
        b = mg.concat([ix] * N, [k * ix.payload.size for k in range(N)], [k * n * ch for k in range(N)])
        nb = mg.workspace_bytes(len(b.frames))
        pins = [torch.from_numpy(np.ascontiguousarray(t).view(np.uint8).reshape(-1).copy()).pin_memory()
                for t in (np.tile(ix.payload, N), b.frames, b.streams)]
        devs = [torch.empty_like(t, device=dev) for t in pins]
        s16 = torch.empty(N * n * ch, dtype=torch.int16, device=dev)
        pcm = torch.empty(N * n, dtype=torch.float32, device=dev)
        status = torch.empty(4 * len(b.frames), dtype=torch.int32, device=dev)
        ws = torch.empty(max(nb // 8, 1), dtype=torch.int64, device=dev)

        def upload():
            for d_, p_ in zip(devs, pins):
                d_.copy_(p_, non_blocking=True)

        def decode():
            mg.decode_device(devs[0], devs[1], len(b.frames), devs[2], len(b.streams), status, ws, out_s16=s16)

        def widen():
            _lib.check(L.aa_pcm_s16_to_f32(_lib.dptr(s16), N * n, ch, _lib.dptr(pcm), _lib.stream_ptr()), "widen")

        def path():
            upload()
            decode()
            widen()

        r = {"device_path_ms": _events(path, a.launches, torch), "decode_ms": _events(decode, a.launches, torch),
             "widen_ms": _events(widen, a.launches, torch), "upload_ms": _events(upload, a.launches, torch),
             "workspace_mib": nb / 2 ** 20}
        r["device_path_ms_per_clip"] = r["device_path_ms"]["median"] / N
        r["frames_per_s_decode"] = N * n / (r["decode_ms"]["median"] * 1e-3)
        r["status_all_ok"] = not bool(status.count_nonzero())
        r["s16_equal_to_host_decoder"] = bool(np.array_equal(s16[(N - 1) * n * ch:].cpu().numpy(), ref16))
        out[f"clips_{N}"] = r
        del pins, devs, s16, pcm, status, ws

    # ---- an MP3 corpus through the batched path, both modes, alternating
    if a.corpus:
        from aa_amd.batch import BatchAnalyser
        from aa_amd.corpus import default_lanes
        from tools.make_models import make_ensemble
        with tempfile.TemporaryDirectory() as td:
            td = Path(td)
            make_ensemble(td / "models")
            models = [str(td / "models" / m / "audioModel.keras") for m in ("model1", "model2")]
            first = td / "c0.mp3"
            first.write_bytes(data)
            jobs = [(0, str(first))]
            for k in range(1, a.corpus):
                p = td / f"c{k}.mp3"
                try:
                    os.link(first, p)
                except OSError:
                    p.write_bytes(data)
                jobs.append((k, str(p)))
            ba = {m: BatchAnalyser(models, False, device=dev, batch=a.batch, lanes=default_lanes(), mp3=m)
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
            audio_s = a.corpus * n / float(st["sample_rate"])
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
