"""classify()'s model-group loop with a model whose metadata sets n_fft 4800
(= sr // 10 at 48 kHz; src/identify_tracks.py:472-497 reads the key,
librosa.stft takes any size): the front end follows it through
fe_stft_mel_mixed and the per-track means stay within the project's 1e-3 of
the CPU oracle.  The _run / _oracle / _model pattern of
tests/test_gpu_pipeline.py, restated."""
import json
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

META = {"n_fft": 4800, "hop_length": 640}


def _track(s, e, f0=0, f1=24000):
    return SimpleNamespace(start=s, end=e, freq_start=f0, freq_end=f1, length=e - s, results=[])


def _run(gpu, monkeypatch, frames, tracks, group, seed=5):
    from aa_amd import pipeline
    got = {}

    def capture(tr, sel, means, meta):
        for row, ti in enumerate(sel):
            got[ti] = means[row]
    monkeypatch.setattr(pipeline, "apply_group_scores", capture)
    np.random.seed(seed)
    pipeline.Classifier("bf16x3", device=gpu).classify_tracks(frames, 48000, tracks, [group])
    return got


def _oracle(frames, tracks, group, meta, seed=5):
    import bench
    from aa_amd.pipeline import fe_settings_from_meta
    from aa_amd.windows import filtered_sources, schedule
    from oracle import cnn_oracle, fe_oracle
    s = fe_settings_from_meta(meta, 48000)
    np.random.seed(seed)
    views, spans = schedule(len(frames), 48000, tracks, s.segment_length, 1.5, s.fmin, s.fmax, False,
                            return_spans=True)
    extra, views = filtered_sources(frames, 48000, tracks, views, spans, meta.get("filter_freq", False),
                                    meta.get("filter_below"), len(frames))
    buf = np.concatenate([frames, extra])
    cfg = bench.fe_config(s)
    out = {}
    for ti, tv in enumerate(views):
        if not tv:
            continue
        mel = np.stack([fe_oracle.window_logmel(bench.window_samples(buf, v, s.win_len), cfg) for v in tv])
        probs = np.stack([cnn_oracle.forward(p.with_suffix(".safetensors"), mel)[1] for p, _ in group])
        out[ti] = np.mean(np.mean(probs, axis=0), axis=0)
    return out


def _model(tmp_path, name, **kw):
    from tools.make_models import make_model
    p = make_model(tmp_path / name, name=name, seed=4, **kw)
    meta = json.loads((p.parent / "metadata.txt").read_text())
    return p.with_suffix(".keras"), meta


def test_nfft4800_model_matches_oracle(gpu, monkeypatch, tmp_path):
    from aa_amd.frontend import FrontEnd
    from aa_amd.pipeline import fe_settings_from_meta
    from tools import synth
    path, meta = _model(tmp_path, "m_n4800", meta_overrides=META)
    s = fe_settings_from_meta(meta, 48000)
    assert (s.n_fft, s.hop_length) == (4800, 640)
    assert FrontEnd(s, gpu).stage_info(1)[0] == "fe_stft_mel_mixed"
    frames = synth.clip(24, seconds=10.0)
    tracks = [_track(0.0, 10.0), _track(2.0, 4.5)]
    group = [(path, meta)]
    got = _run(gpu, monkeypatch, frames, tracks, group)
    ref = _oracle(frames, tracks, group, meta)
    assert sorted(got) == sorted(ref) == [0, 1]
    d = max(float(np.abs(got[k] - ref[k]).max()) for k in ref)
    print(f"n_fft 4800 / hop 640: max|d track mean| = {d:.2e}")
    assert d <= 1e-3
