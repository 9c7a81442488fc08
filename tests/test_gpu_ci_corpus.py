"""Corpus runs of the old cacophony index (aa_amd/ci_batch.py, ``corpus.run(...,
old_cacophony_index=True)``, ``python -m aa_amd.corpus --old-cacophony-index``).

Two expectations.  The independent one: 16 kHz mono PCM16 files of the golden
clips need no resampling, so their documents must equal the restated index
(tests/ci_restated.py, float64 on the CPU) of the very samples -- after the
assertion, from the CPU data alone, that no band comparison of these clips is
within float64 noise of its threshold (tests/test_gpu_cacophony.py's rule).
And equality with the single-file path: every file of a mixed corpus (rates,
channel counts, encodings, decoder modes, a short clip, two bad files) gets the
document -- or the failure -- ``cacophony_index.calculate(path)`` gives for it
alone, at every batch size and lane count.
"""
import json
import struct
import subprocess
import sys
import wave
from pathlib import Path

import numpy as np
import pytest

import ci_restated

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "audio-analysis_amd"


def _docs(res):
    return {k: {kk: vv for kk, vv in v.items() if kk != "processing_time_seconds"} for k, v in res.items()}


def _q(x):
    """float samples of an int16-quantised clip -> the int16 values a PCM16 file carries."""
    q = np.round(np.asarray(x, np.float64) * 32768.0)
    assert np.array_equal(q / 32768.0, np.asarray(x, np.float64)) and np.abs(q).max() < 32768
    return q.astype(np.int16)


def _write_pcm(path, q, sr, width=2):
    """q: int16 [n] or [n, channels] -> a PCM WAV of `width` bytes per sample (24-bit: the int16 value << 8)."""
    q = np.asarray(q)
    ch = 1 if q.ndim == 1 else q.shape[1]
    with wave.open(str(path), "wb") as w:
        w.setnchannels(ch)
        w.setsampwidth(width)
        w.setframerate(sr)
        if width == 2:
            w.writeframes(q.astype("<i2").tobytes())
        else:
            v = (q.astype(np.int32).reshape(-1) << 8).astype("<i4")
            w.writeframes(v.view(np.uint8).reshape(-1, 4)[:, :3].tobytes())
    return str(path)


def _write_f32(path, x, sr):
    """A mono IEEE float32 WAV (format tag 3)."""
    data = np.asarray(x, "<f4").tobytes()
    fmt = struct.pack("<HHIIHH", 3, 1, sr, sr * 4, 4, 32)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(data)) + data
    Path(path).write_bytes(b"RIFF" + struct.pack("<I", len(body)) + body)
    return str(path)


# ---- the independent expectation ------------------------------------------
GOLDEN_16K = ["n320000", "n720000", "n5121", "n4096", "silence"]


def test_16k_files_equal_the_restated_index(gpu, tmp_path):
    from aa_amd import corpus
    from aa_amd import cacophony_index as ci
    files, want = [], {}
    for k, name in enumerate(GOLDEN_16K):
        x = ci_restated.case_clip(name)
        q = _q(x)
        ref = ci_restated.bins(q.astype(np.float32) / np.float32(32768.0))
        assert not ci_restated.near_decisions(ref).any(), name  # from the CPU data, before the GPU is consulted
        want[k] = ci.score_table(ci_restated.points(ref), len(q))
        files.append(_write_pcm(tmp_path / f"{name}.wav", q, 16000))
    assert len(want[0]["cacophony_index_old"]) == 1 and len(want[1]["cacophony_index_old"]) == 2
    assert want[3]["cacophony_index_old"] == [] and "ci_warning" in want[3] and "ci_warning" in want[2]
    for batch in (16, 2):
        res = corpus.run(files, None, batch=batch, old_cacophony_index=True)
        assert all(isinstance(r["processing_time_seconds"], float) for r in res.values())
        assert json.dumps(_docs(res), sort_keys=True) == json.dumps(want, sort_keys=True), batch


# ---- equality with the single-file path -----------------------------------
@pytest.fixture(scope="module")
def mixed(gpu, tmp_path_factory):
    """The corpus (files of 20 to 21 s, a 3 s clip, two bad files) and, per
    file, calculate()'s document or failure, computed once."""
    import flac_writer as fw
    import mp3_cases as mc
    import mp3_writer as mw
    import vorbis_cases as vc
    import vorbis_writer as vw
    from aa_amd import cacophony_index as ci
    from aa_amd import corpus
    d = tmp_path_factory.mktemp("ci_corpus")

    def clip(seed, seconds, sr):
        return _q(ci_restated.clip(seed, int(seconds * sr), sr=sr))

    files = []
    files.append(_write_pcm(d / "w48m.wav", clip(1, 20.5, 48000), 48000))
    a = clip(2, 20.0, 48000)
    files.append(_write_pcm(d / "w48s.wav", np.stack([a, a[::-1] // 2], 1), 48000))
    a = clip(3, 20.2, 44100)
    files.append(_write_pcm(d / "w441s.wav", np.stack([a, -(a[::-1] // 3)], 1), 44100))
    files.append(_write_pcm(d / "w8m.wav", clip(4, 21.0, 8000), 8000))
    files.append(_write_pcm(d / "w16m.wav", clip(5, 20.0, 16000), 16000))
    files.append(_write_pcm(d / "w24.wav", clip(6, 20.0, 48000), 48000, width=3))    # host route
    files.append(_write_f32(d / "wf32.wav", clip(7, 20.0, 32000) / 32768.0, 32000))  # host route
    y = clip(8, 20.0, 32000).astype(np.int64)
    frames = [fw.frame([y[i:i + 4096]], 16, 32000, k) for k, i in enumerate(range(0, len(y), 4096))]
    (d / "f.flac").write_bytes(fw.stream(frames, 32000, 1, 16, len(y), 4096))
    files.append(str(d / "f.flac"))
    x = ci_restated.clip(9, int(0.6 * 48000), sr=48000)
    ogg = vc.repeat(vw.encode(x, sr=48000, schedule=[1, 1, 0, 0, 1]), 33)            # 20.6 s
    (d / "v.ogg").write_bytes(ogg)
    files.append(str(d / "v.ogg"))
    c = mc.case("mono_long")
    (d / "m.mp3").write_bytes(mw.stream(list(c["frames"]) * 200, sr_index=c["sr_index"], channels=c["channels"]))
    files.append(str(d / "m.mp3"))                                                    # 800 frames: 20.9 s
    files.append(_write_pcm(d / "short.wav", clip(10, 3.0, 48000), 48000))
    (d / "cut.wav").write_bytes(Path(files[0]).read_bytes()[:20])                     # cut inside its fmt chunk
    files.append(str(d / "cut.wav"))
    (d / "x.opus").write_bytes(Path(files[4]).read_bytes())
    files.append(str(d / "x.opus"))
    files.append(_write_pcm(d / "last.wav", clip(11, 20.0, 44100), 44100))            # behind the bad files
    want = {}
    for k, f in enumerate(files):
        try:
            want[k] = ci.calculate(f)
        except Exception as e:
            want[k] = {corpus.FAILED: f"{type(e).__name__}: {e}"}
    return files, want


def test_the_mixed_corpus_is_what_it_claims(mixed):
    from aa_amd import corpus
    from aa_amd.audio import decode
    files, want = mixed
    bad = {k for k, w in want.items() if corpus.FAILED in w}
    assert {Path(files[k]).name for k in bad} == {"cut.wav", "x.opus"}
    assert want[11][corpus.FAILED] == "error: unpack requires a buffer of 16 bytes"  # struct.error, in the fmt chunk
    assert want[12][corpus.FAILED] == f"ValueError: {files[12]}: Opus needs a codec this build does not have"
    for k, f in enumerate(files):
        if k in bad:
            continue
        x, sr = decode(f)
        secs = len(x) / sr
        if Path(f).name == "short.wav":
            assert secs == 3.0 and want[k]["cacophony_index_old"] == [] and "3 seconds" in want[k]["ci_warning"]
        else:
            assert 20.0 <= secs <= 21.0, (f, secs)
            assert len(want[k]["cacophony_index_old"]) == 1 and "ci_warning" not in want[k], f
    assert {decode(files[k])[1] for k in range(len(files)) if k not in bad} == {48000, 44100, 8000, 16000, 32000}


@pytest.mark.parametrize("mode", ["gpu", "host"])
@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("batch", [1, 3, 16])
def test_corpus_equals_calculate_per_file(gpu, mixed, monkeypatch, batch, lanes, mode):
    from aa_amd import ci_batch, corpus, flac_gpu, mp3_gpu, vorbis_gpu
    files, want = mixed
    calls = {"flac": 0, "vorbis": 0, "mp3": 0, "resample": []}
    for name, mod in (("flac", flac_gpu), ("vorbis", vorbis_gpu), ("mp3", mp3_gpu)):
        def counted(*a, _real=mod.decode_device, _name=name, **kw):
            calls[_name] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(mod, "decode_device", counted)

    def resample_counted(s16, f32, segments, sr_in, *a, _real=ci_batch.resample_batch, **kw):
        calls["resample"].append((sr_in, len(list(segments))))
        return _real(s16, f32, segments, sr_in, *a, **kw)

    monkeypatch.setattr(ci_batch, "resample_batch", resample_counted)
    monkeypatch.setenv("AA_BATCH_LANES", str(lanes))
    res = corpus.run(files, None, batch=batch, flac=mode, vorbis=mode, mp3=mode, old_cacophony_index=True)
    assert sorted(res) == list(range(len(files)))
    for k, f in enumerate(files):
        got = dict(res[k])
        if corpus.FAILED not in got:
            assert isinstance(got.pop("processing_time_seconds"), float)
        assert json.dumps(got, sort_keys=True) == json.dumps(want[k], sort_keys=True), f
    # the decoders ran where the mode says, and every file off 16 kHz went through aa_resample_batch
    if mode == "gpu":
        assert calls["flac"] >= 1 and calls["vorbis"] >= 1 and calls["mp3"] >= 1
    else:
        assert calls["flac"] == calls["vorbis"] == calls["mp3"] == 0
    assert sum(n for _, n in calls["resample"]) == len(files) - 3  # all but w16m.wav and the two bad files
    if batch == 16:  # one batch: one launch per distinct input rate
        assert sorted(calls["resample"]) == [(8000, 1), (32000, 2), (44100, 3), (48000, 5)]


# ---- the CLI ---------------------------------------------------------------
def _child(args):
    r = subprocess.run([sys.executable, *args], capture_output=True, text=True, timeout=300, cwd=PKG)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_cli_prints_what_analyse_prints_per_file(gpu, tmp_path):
    files = [_write_pcm(tmp_path / "a.wav", _q(ci_restated.case_clip("n336000")), 16000),
             _write_pcm(tmp_path / "b.wav", _q(ci_restated.clip(21, 20 * 48000 + 5, sr=48000)), 48000),
             _write_pcm(tmp_path / "c.wav", _q(ci_restated.clip(22, 3 * 44100, sr=44100)), 44100)]
    out = json.loads(_child(["-m", "aa_amd.corpus", "--old-cacophony-index", "-o", *files]))
    assert [e["file"] for e in out] == files
    # analyse.py per file, in one child: its main() once per file, each printing its document
    script = ("import sys, analyse\n"
              "for f in sys.argv[1:]:\n"
              "    analyse.main([f, '--old-cacophony-index', '-o'])\n"
              "    print('\\x1e')\n")
    per_file = [json.loads(t) for t in _child(["-c", script, *files]).split("\x1e") if t.strip()]
    assert len(per_file) == 3
    for e, single in zip(out, per_file):
        assert isinstance(e["analysis_result"].pop("processing_time_seconds"), float)
        assert isinstance(single.pop("processing_time_seconds"), float)
        assert e["analysis_result"] == single
    assert len(per_file[1]["cacophony_index_old"]) == 1 and "ci_warning" in per_file[2]
    assert not any(Path(f).with_suffix(".txt").exists() for f in files)


def test_cli_writes_and_merges_sidecars(gpu, tmp_path, monkeypatch):
    from aa_amd import cacophony_index as ci
    from aa_amd import corpus
    files = [_write_pcm(tmp_path / "a.wav", _q(ci_restated.case_clip("n336000")), 16000),
             _write_pcm(tmp_path / "b.wav", _q(ci_restated.clip(23, 20 * 48000, sr=48000)), 48000)]
    (tmp_path / "b.txt").write_text(json.dumps({"location": "here", "analysis_result": {"stale": 1}}))
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", "16")  # (what main() would set; restored after the test)
    corpus.main([*files, "--old-cacophony-index", "--bird-model", "ignored.keras"])
    for f in files:
        side = json.loads(Path(f).with_suffix(".txt").read_text())
        res = side["analysis_result"]
        assert isinstance(res.pop("processing_time_seconds"), float)
        assert res == ci.calculate(f)
    assert json.loads((tmp_path / "b.txt").read_text())["location"] == "here"
    assert set(json.loads((tmp_path / "a.txt").read_text())) == {"analysis_result"}
