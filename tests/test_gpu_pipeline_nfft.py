"""classify()'s model-group loop with a model whose metadata sets a short
n_fft (src/identify_tracks.py:472-497 reads it, librosa.stft takes any size):
the front end follows n_fft 1024 and 512 through fe_stft_mel_small and the
per-track means stay within the project's 1e-3 of the CPU oracle."""
import numpy as np
import pytest

from test_gpu_pipeline import _model, _oracle, _run, _track

pytestmark = pytest.mark.gpu

CASES = {
    "n1024_hop256": {"n_fft": 1024, "hop_length": 256},
    "n512_hop128_mel80": {"n_fft": 512, "hop_length": 128, "n_mels": 80},
}


@pytest.mark.parametrize("name", list(CASES))
def test_short_nfft_model_matches_oracle(gpu, monkeypatch, tmp_path, name):
    from aa_amd.pipeline import fe_settings_from_meta
    from tools import synth
    path, meta = _model(tmp_path, "m_" + name, meta_overrides=CASES[name])
    s = fe_settings_from_meta(meta, 48000)
    assert (s.n_fft, s.hop_length) == (CASES[name]["n_fft"], CASES[name]["hop_length"])
    frames = synth.clip(23, seconds=8.0)
    tracks = [_track(0.0, 8.0), _track(2.0, 4.5)]
    group = [(path, meta)]
    got = _run(gpu, monkeypatch, frames, tracks, group)
    ref = _oracle(frames, tracks, group, meta)
    assert sorted(got) == sorted(ref) == [0, 1]
    d = max(float(np.abs(got[k] - ref[k]).max()) for k in ref)
    print(f"{name}: max|d track mean| = {d:.2e}")
    assert d <= 1e-3
