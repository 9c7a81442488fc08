"""The front end's n_fft set on the host (no GPU call): aa_fe_create accepts the
powers of two 256..8192 and refuses everything else before any HIP call, and
the metadata keys of a short-transform model reach FeSettings unchanged."""
import ctypes as C

import numpy as np
import pytest

from aa_amd import _lib


@pytest.mark.parametrize("n_fft", [128, 1000, 3000, 16384])
def test_refused_sizes(n_fft):
    L = _lib.lib()
    h = C.c_void_p()
    cfg = _lib.FeConfig(win_len=144000, n_fft=n_fft, hop=640, n_mels=160, normalize=1,
                        db_scale=1, power=2.0, amin=1e-10, top_db=80.0, mean_sub=0, channels=1)
    fb = np.zeros((160, n_fft // 2 + 1), np.float32)
    rc = L.aa_fe_create(C.byref(cfg), fb.ctypes.data, C.byref(h))
    assert rc == _lib.AA_ERR_UNSUPPORTED == 3
    msg = L.aa_last_error()
    assert b"n_fft" in msg and b"256..8192" in msg and str(n_fft).encode() in msg
    assert not h.value


@pytest.mark.parametrize("n_fft,hop,frames", [(256, 64, 2251), (512, 128, 1126), (1024, 256, 563),
                                              (1024, 281, 513)])
def test_settings_from_meta_carry_short_sizes(n_fft, hop, frames):
    from aa_amd.pipeline import fe_settings_from_meta
    s = fe_settings_from_meta({"n_fft": n_fft, "hop_length": hop, "n_mels": 80, "htk": True}, 48000)
    assert (s.n_fft, s.hop_length, s.n_mels, s.win_len) == (n_fft, hop, 80, 144000)
    assert s.n_frames == frames == 1 + 144000 // hop
    fb = s.filterbank()
    assert fb.shape == (80, n_fft // 2 + 1) and np.isfinite(fb).all()
