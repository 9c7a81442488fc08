"""GPU parity: libaa.so front end vs the CPU oracle (oracle/fe_oracle.py).

Tolerance (stated, fp32): log-mel |delta| <= 1e-3 dB.  The reference computes
the STFT in float64 (librosa 0.11 + numpy pocketfft) and stores complex64;
the GPU transform is float32 throughout, so its error is ~1e-5 dB on noise-like
audio and ~6e-4 dB in the worst bands of a pure tone next to the -80 dB floor
(measured with a float32 pocketfft at the same configuration).  For the inputs
of test_generic_kernel_large_sizes a float32 FFT (scipy.fft.rfft on float32
frames, float32 mel sums) differs from the oracle by 1.1e-5 dB (full view) and
2.1e-4 dB (short view, whose zero-padded frames reach the -80 dB floor) at
n_fft 4096 with the full band, and by 7.6e-6 dB and 2.5e-4 dB at n_fft 8192: a
quarter of the gate at most.  Non-dB outputs
(power mel) compare with rtol 2e-4 relative to the window maximum.
"""
import numpy as np
import pytest
import torch

from oracle import fe_oracle
from tools import synth

pytestmark = pytest.mark.gpu

DB_TOL = 1e-3


def _setup(settings, clip, views):
    from aa_amd.frontend import FrontEnd, pack_windows
    fe = FrontEnd(settings)
    pcm = torch.from_numpy(clip).cuda()
    win = torch.from_numpy(pack_windows(views, len(clip), win_len=settings.win_len)).cuda()
    status = torch.zeros(len(views), dtype=torch.int32, device="cuda")
    out = fe.run(pcm, win, status=status)
    torch.cuda.synchronize()
    return out.cpu().numpy(), status.cpu().numpy()


def _raw_window(clip, view, win_len):
    src, n, left = view
    w = np.zeros(win_len, np.float32)
    w[left:left + n] = clip[src:src + n]
    return w


def _cfg(s):
    return dict(sr=s.sr, hop_length=s.hop_length, n_mels=s.n_mels, fmin=s.fmin, fmax=s.fmax,
                n_fft=s.n_fft, power=s.power, db_scale=s.db_scale, htk=s.htk,
                break_freq=s.break_freq, normalize=s.normalize, mean_sub=s.mean_sub,
                channels=s.channels)


CASES = {
    "default_htk": dict(htk=True),
    "hop281": dict(htk=True, hop_length=281),
    "slaney": dict(htk=False),
    "power1_nodb": dict(htk=True, power=1, db_scale=False),
    "nonorm_meansub_ch3": dict(htk=True, normalize=False, mean_sub=True, channels=3),
    "nfft2048_80mel": dict(htk=True, n_fft=2048, n_mels=80, break_freq=1000, hop_length=512),
}


@pytest.mark.parametrize("name", list(CASES))
def test_frontend_matches_oracle(gpu, name):
    from aa_amd.frontend import FeSettings
    s = FeSettings(**CASES[name])
    clip = synth.clip(3, seconds=7.0)
    # windows: three full, one straddling the end (zero padded), one short view
    views = [(0, s.win_len, 0), (72000, s.win_len, 0), (192000, 144000, 0),
             (300000, 36000, 50000), (5, 100000, 44000)]
    got, status = _setup(s, clip, views)
    assert (status == 0).all()
    for i, v in enumerate(views):
        ref = fe_oracle.window_logmel(_raw_window(clip, v, s.win_len), _cfg(s))
        g = got[i]
        assert g.shape == ref.shape
        if s.db_scale and not s.mean_sub:
            err = np.abs(g - ref).max()
            assert err <= DB_TOL, (name, i, err)
        elif s.db_scale:
            assert np.abs(g - ref).max() <= 2 * DB_TOL
        else:
            scale = np.abs(ref).max()
            assert np.abs(g - ref).max() <= 2e-4 * scale, (name, i)


# Two instantiations of fe_stft_mel that no other case reaches, on half-second
# windows (38 and 24 frames: a few 6-frame items per window, the first ones of a
# view that starts inside the window with a partial segment).
NEW_CASES = {
    "nfft4096_fullband": dict(htk=True, segment_length=0.5, fmin=0, fmax=24000),  # band outside X[2..1022]
    "nfft8192": dict(htk=True, segment_length=0.5, n_fft=8192, hop_length=1024),
}
# one full view; one short view whose left padding and centre padding meet in
# the first frames
NEW_VIEWS = [(0, 24000, 0), (30000, 9000, 1500)]


@pytest.mark.parametrize("name", list(NEW_CASES))
def test_generic_kernel_large_sizes(gpu, name):
    """fe_stft_mel<4096> (the fallback of n_fft 4096 when the kept band leaves
    X[2..1022]) and fe_stft_mel<8192> against the oracle at DB_TOL (the float32
    reference's own error for these inputs: module docstring)."""
    from aa_amd.frontend import FeSettings, FrontEnd
    s = FeSettings(**NEW_CASES[name])
    assert s.n_frames == {"nfft4096_fullband": 38, "nfft8192": 24}[name]
    assert FrontEnd(s).stage_info(1)[0] == "fe_stft_mel"
    clip = synth.clip(3, seconds=1.0)
    got, status = _setup(s, clip, NEW_VIEWS)
    assert (status == 0).all()
    for i, v in enumerate(NEW_VIEWS):
        ref = fe_oracle.window_logmel(_raw_window(clip, v, s.win_len), _cfg(s))
        assert got[i].shape == ref.shape
        err = np.abs(got[i] - ref).max()
        print(name, v, "max |delta| dB", err)
        assert err <= DB_TOL, (name, i, err)


def test_pure_tone_near_floor(gpu):
    from aa_amd.frontend import FeSettings
    s = FeSettings(htk=True)
    clip = synth.tone(1000.0, seconds=3.0)
    got, _ = _setup(s, clip, [(0, s.win_len, 0)])
    ref = fe_oracle.window_logmel(clip, _cfg(s))
    assert np.abs(got[0] - ref).max() <= DB_TOL
    # the window max sits at 0 dB up to log10f rounding (the reference clamps at
    # log_spec.max() - top_db, this build at -top_db: same within 1e-5 dB)
    assert abs(float(got[0].max())) <= 1e-5 and got[0].min() == -80.0


def test_normalization_bitexact(gpu):
    """db_scale off, power 1 and a single-bin-width filterbank would still mix
    bins; instead check normalize_data through the window statistics: a window
    whose samples are all equal is flagged (0/0 in normalize_data -> librosa
    raises), as is a window with a NaN or an empty view."""
    from aa_amd.frontend import FeSettings
    s = FeSettings(htk=True)
    clip = synth.clip(4, seconds=4.0)
    clip[150000] = np.nan
    views = [(0, s.win_len, 0), (50000, 142000, 0), (0, 0, 17), (1000, 10, 5)]
    const = np.full(200, 0.25, np.float32)
    clip2 = np.concatenate([clip, const])
    views.append((len(clip), 200, 0))  # 200 equal samples + zeros: fine (min 0, max 0.25)
    _, status = _setup(s, clip2, views)
    assert list(status) == [0, 1, 1, 0, 0]
    ones = np.full(s.win_len, 0.5, np.float32)
    _, st2 = _setup(s, ones, [(0, s.win_len, 0)])
    assert list(st2) == [1]
