"""GPU parity of the short-transform front end (fe_stft_mel_small: n_fft 256,
512 and 1024) against the CPU oracle (oracle/fe_oracle.py).

Tolerances are those of tests/test_gpu_frontend.py, stated there for f32 FFTs
against the float64 oracle: log-mel |delta| <= 1e-3 dB, 2e-3 dB with mean_sub
(the band mean is a second f32 sum over the frames), power output within 2e-4
of the window maximum.  Windows are 0.25 s (12000 samples), so every case has
a block that is not full, frames that reach into the centre padding on both
sides and, with the views below, zero padding on either side of the samples.
"""
import numpy as np
import pytest
import torch

from oracle import fe_oracle
from tools import synth

pytestmark = pytest.mark.gpu

DB_TOL = 1e-3

# (src, n_valid, pad_left): two full windows, one that straddles the end of the
# clip (zero padded), one short view set into the window, one shorter than n_fft/2
VIEWS = [(0, 12000, 0), (30000, 12000, 0), (40000, 8000, 0), (20000, 3000, 5000), (1000, 100, 0)]

CASES = {
    # T = 47 (odd); one empty mel row
    "n1024_hop256_mel160": dict(n_fft=1024, hop_length=256, n_mels=160),
    # T = 94; one empty row; two frames per wave
    "n512_hop128_mel80": dict(n_fft=512, hop_length=128, n_mels=80),
    # T = 188 = 4 * 47, not a multiple of 16
    "n256_hop64_mel40": dict(n_fft=256, hop_length=64, n_mels=40),
    # hop not a multiple of 4
    "n1024_hop281_mel80": dict(n_fft=1024, hop_length=281, n_mels=80),
    # hop > n_fft, T = 9: frames load their own samples
    "n1024_hop1500_mel80": dict(n_fft=1024, hop_length=1500, n_mels=80),
    # small odd hop, T = 325
    "n512_hop37_mel80": dict(n_fft=512, hop_length=37, n_mels=80),
    # 0 Hz .. Nyquist: kmin 1, kmax 127
    "n256_fullband": dict(n_fft=256, hop_length=64, n_mels=40, fmin=0, fmax=24000),
    "n1024_slaney": dict(n_fft=1024, hop_length=256, n_mels=80, htk=False),
    "n512_power1_nodb": dict(n_fft=512, hop_length=128, n_mels=80, power=1, db_scale=False),
    "n256_nonorm_meansub_ch3": dict(n_fft=256, hop_length=64, n_mels=40, normalize=False, mean_sub=True,
                                    channels=3),
}


def _settings(**kw):
    from aa_amd.frontend import FeSettings
    base = dict(sr=48000, segment_length=0.25, htk=True)
    base.update(kw)
    return FeSettings(**base)


def _run(settings, clip, views):
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


@pytest.fixture(scope="module")
def clip():
    return synth.clip(3, seconds=1.0)


@pytest.mark.parametrize("name", list(CASES))
def test_small_frontend_matches_oracle(gpu, clip, name):
    s = _settings(**CASES[name])
    assert s.win_len == 12000
    got, status = _run(s, clip, VIEWS)
    assert (status == 0).all()
    worst = 0.0
    for i, v in enumerate(VIEWS):
        ref = fe_oracle.window_logmel(_raw_window(clip, v, s.win_len), _cfg(s))
        g = got[i]
        assert g.shape == ref.shape == (s.n_mels, s.n_frames, s.channels)
        assert np.isfinite(g).all()
        err = float(np.abs(g - ref).max())
        if s.db_scale and not s.mean_sub:
            tol = DB_TOL
        elif s.db_scale:
            tol = 2 * DB_TOL
        else:
            tol = 2e-4 * float(np.abs(ref).max())
        worst = max(worst, err / tol)
        print(f"{name} view {i}: max|d| = {err:.3e} (tolerance {tol:.3e})")
        assert err <= tol, (name, i, err, tol)
    print(f"{name}: worst error / tolerance = {worst:.3f}")


def test_small_pure_tone_near_floor(gpu):
    s = _settings(n_fft=1024, hop_length=256, n_mels=160)
    tone = synth.tone(1000.0, seconds=0.25)
    got, _ = _run(s, tone, [(0, s.win_len, 0)])
    ref = fe_oracle.window_logmel(tone, _cfg(s))
    err = float(np.abs(got[0] - ref).max())
    print(f"pure tone 1024/256/160: max|d| = {err:.3e} dB")
    assert err <= DB_TOL
    # the window max sits at 0 dB up to log10f rounding; empty and far bands at the floor
    assert abs(float(got[0].max())) <= 1e-5 and got[0].min() == -80.0


def test_small_status_flags(gpu):
    """The window status of test_normalization_bitexact at n_fft 512: a NaN, an
    empty view and an all-equal window are flagged, short views are not."""
    s = _settings(n_fft=512, hop_length=128, n_mels=80)
    c = synth.clip(4, seconds=1.0).copy()
    c[20000] = np.nan
    views = [(0, s.win_len, 0), (15000, 12000, 0), (0, 0, 17), (1000, 10, 5)]
    const = np.full(200, 0.25, np.float32)
    c2 = np.concatenate([c, const])
    views.append((len(c), 200, 0))  # 200 equal samples + zeros: fine (min 0, max 0.25)
    _, status = _run(s, c2, views)
    assert list(status) == [0, 1, 1, 0, 0]
    ones = np.full(s.win_len, 0.5, np.float32)
    _, st2 = _run(s, ones, [(0, s.win_len, 0)])
    assert list(st2) == [1]


def test_small_blocks_do_not_depend_on_the_batch(gpu, clip):
    """70 windows in one run equal, bit for bit, the same windows five at a time."""
    from aa_amd.frontend import FrontEnd, pack_windows
    s = _settings(n_fft=256, hop_length=64, n_mels=40)
    views = [(401 * i, s.win_len - 60 - 57 * (i % 7), 13 * (i % 5)) for i in range(70)]
    fe = FrontEnd(s)
    pcm = torch.from_numpy(clip).cuda()
    win = torch.from_numpy(pack_windows(views, len(clip), win_len=s.win_len)).cuda()
    whole = fe.run(pcm, win).clone()
    parts = torch.cat([fe.run(pcm, win[i:i + 5].contiguous()).clone() for i in range(0, 70, 5)])
    torch.cuda.synchronize()
    assert whole.shape == parts.shape == (70, 40, s.n_frames, 1)
    assert torch.equal(whole, parts)
