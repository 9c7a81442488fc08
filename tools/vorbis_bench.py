"""Time Ogg Vorbis decode on the device (aa_vorbis_decode_device) against the
host route (aa_vorbis_decode on one thread) and, optionally, a Vorbis corpus
through the batched path in both modes.

    python tools/vorbis_bench.py [--seconds 60] [--encode-seconds 2] [--channels 2] [--clips 1,16]
                                 [--launches 20] [--clip-file F.ogg] [--corpus FILES --pairs 5]

The clip: a tools/synth signal, 48 kHz, encoded by the test encoder
(tests/vorbis_writer.py: floor 1, coupled residue 2 when stereo, blocks 256 /
2048, mostly long).  That encoder is Python; only --encode-seconds distinct
seconds are encoded and their audio packets repeated (tests/vorbis_cases.py
`repeat`) up to --seconds; the output says so ("distinct_seconds").
--clip-file caches the stream.

Per clip count N, HIP events around `launches` repetitions after warm-up,
medians with min and max:
  device_path   N clips' packet bytes, tables and setups from pinned memory,
                aa_vorbis_decode_device (unpack, IMDCT + window, overlap-add +
                s16), aa_pcm_s16_to_f32
  decode_ms     aa_vorbis_decode_device alone;  widen_ms: aa_pcm_s16_to_f32 alone
and on this host, one thread, per clip: the index pass (vorbis_gpu.index) and
the host route the corpus path takes today (audio.decode_vorbis, the numpy
conversion to s16 and mono float32, the blocking upload of the float32
samples).

--corpus FILES: FILES copies of the clip through BatchAnalyser(vorbis="host")
and (vorbis="gpu") in --pairs alternating pairs after a warm-up run of each;
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


def make_clip(seconds: float, distinct: float, channels: int) -> bytes:
    import vorbis_cases as vc
    import vorbis_writer as vw
    from tools import synth
    distinct = min(distinct, seconds)
    x = synth.clip(7, seconds=distinct)
    if channels == 2:
        x = np.stack([x, 0.5 * x[::-1]], 1)
    one = vw.encode(x, sr=48000, schedule=[1] * 14 + [0, 0], residue_type=2 if channels == 2 else 1)
    return vc.repeat(one, max(1, int(round(seconds / distinct))))


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
    ap.add_argument("--encode-seconds", type=float, default=2.0)
    ap.add_argument("--channels", type=int, default=2, choices=(1, 2))
    ap.add_argument("--clips", default="1,16")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--clip-file", default=None)
    ap.add_argument("--corpus", type=int, default=0)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--make-only", action="store_true", help="write --clip-file and stop (needs no GPU)")
    a = ap.parse_args()

    if a.clip_file and os.path.exists(a.clip_file):
        data = Path(a.clip_file).read_bytes()
    else:
        data = make_clip(a.seconds, a.encode_seconds, a.channels)
        if a.clip_file:
            Path(a.clip_file).write_bytes(data)
    if a.make_only:
        return

    import torch

    from aa_amd import _lib, audio, vorbis_gpu as vg
    from aa_amd.corpus import raise_hw_queues

    raise_hw_queues()  # as corpus.main and bench.py do, before the first GPU call
    if not torch.cuda.is_available():
        raise SystemExit("vorbis_bench needs a GPU")
    dev = torch.device("cuda:0")
    ix = vg.index(data)
    if ix is None:
        raise SystemExit("the clip is not indexable")
    st = ix.stream[0]
    n, ch = int(st["frames"]), int(st["channels"])
    out = {"frames_per_clip": n, "channels": ch, "sample_rate": int(st["sample_rate"]),
           "file_bytes_per_clip": len(data), "packets_per_clip": len(ix.packets),
           "payload_bytes_per_clip": int(ix.payload.size), "setup_bytes": int(ix.setup.size),
           "distinct_seconds": min(a.encode_seconds, a.seconds) if not a.clip_file else "see --clip-file",
           "launches": a.launches, "workgroup_packets": vg.WG}
    L = _lib.lib()

    # ---- this host, one thread, per clip
    t_idx, t_dec, t_np, t_up = [], [], [], []
    buf = np.frombuffer(data, np.uint8)
    for _ in range(5):
        t0 = time.perf_counter()
        vg.index(buf)
        t1 = time.perf_counter()
        f, c, sr = audio.decode_vorbis(data)
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
    out["host_route_ms_per_clip"] = {"aa_vorbis_decode": _stats(t_dec), "numpy_s16_and_mono_f32": _stats(t_np),
                                     "blocking_upload_f32": _stats(t_up),
                                     "median_total": float(np.median(t_dec) + np.median(t_np) + np.median(t_up))}
    ref16 = q.astype(np.int16)

    # ---- the device
    for N in (int(c) for c in a.clips.split(",")):
        b = vg.concat([ix] * N, [k * ix.payload.size for k in range(N)], [k * n * ch for k in range(N)])
        pl, nb = vg.plan(b.packets, b.streams)
        pins = [torch.from_numpy(np.ascontiguousarray(t).view(np.uint8).reshape(-1).copy()).pin_memory()
                for t in (np.tile(ix.payload, N), b.packets, b.streams, b.setups)]
        devs = [torch.empty_like(t, device=dev) for t in pins]
        s16 = torch.empty(N * n * ch, dtype=torch.int16, device=dev)
        pcm = torch.empty(N * n, dtype=torch.float32, device=dev)
        status = torch.empty(len(b.packets), dtype=torch.int32, device=dev)
        ws = torch.empty(max(nb // 8, 1), dtype=torch.int64, device=dev)

        def upload():
            for d_, p_ in zip(devs, pins):
                d_.copy_(p_, non_blocking=True)

        def decode():
            vg.decode_device(devs[0], devs[1], len(b.packets), devs[2], len(b.streams), devs[3], pl, status, ws,
                             out_s16=s16)

        def widen():
            _lib.check(L.aa_pcm_s16_to_f32(_lib.dptr(s16), N * n, ch, _lib.dptr(pcm), _lib.stream_ptr()), "widen")

        def path():
            upload()
            decode()
            widen()

        r = {"device_path_ms": _events(path, a.launches, torch), "decode_ms": _events(decode, a.launches, torch),
             "widen_ms": _events(widen, a.launches, torch), "upload_ms": _events(upload, a.launches, torch),
             "workspace_mib": nb / 2 ** 20, "distinct_setups": b.n_setups}
        r["device_path_ms_per_clip"] = r["device_path_ms"]["median"] / N
        r["frames_per_s_decode"] = N * n / (r["decode_ms"]["median"] * 1e-3)
        r["status_all_ok"] = not bool(status.count_nonzero())
        r["s16_equal_to_host_decoder"] = bool(np.array_equal(s16[(N - 1) * n * ch:].cpu().numpy(), ref16))
        out[f"clips_{N}"] = r
        del pins, devs, s16, pcm, status, ws

    # ---- a Vorbis corpus through the batched path, both modes, alternating
    if a.corpus:
        from aa_amd.batch import BatchAnalyser
        from aa_amd.corpus import default_lanes
        from tools.make_models import make_ensemble
        with tempfile.TemporaryDirectory() as td:
            td = Path(td)
            make_ensemble(td / "models")
            models = [str(td / "models" / m / "audioModel.keras") for m in ("model1", "model2")]
            first = td / "c0.ogg"
            first.write_bytes(data)
            jobs = [(0, str(first))]
            for k in range(1, a.corpus):
                p = td / f"c{k}.ogg"
                try:
                    os.link(first, p)
                except OSError:
                    p.write_bytes(data)
                jobs.append((k, str(p)))
            ba = {m: BatchAnalyser(models, False, device=dev, batch=a.batch, lanes=default_lanes(), vorbis=m)
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
