"""Front-end plans for tests/test_fe_plan.py and the recorder of its golden
(tests/golden/make_fe_plan_golden.py): configurations, filterbanks, and what one
plan yields as plain JSON values."""
import ctypes as C
import hashlib

import numpy as np

from aa_amd.frontend import FeSettings

N_WIN = (1, 64)
IMAGES = ("hann", "tw", "tw2", "rows", "vals", "cimg4096")


def _case(n_fft, hop, n_mels, fb=None, edit=None, **kw):
    cfg = dict(win_len=144000, n_fft=n_fft, hop=hop, n_mels=n_mels, normalize=1, db_scale=1, power=2.0,
               amin=1e-10, top_db=80.0, mean_sub=0, channels=1, out_f16=0)
    cfg.update({k: kw.pop(k) for k in list(kw) if k in cfg})
    if fb is None:
        fb = FeSettings(n_fft=n_fft, hop_length=hop, n_mels=n_mels, htk=True, **kw).filterbank()
    fb = np.ascontiguousarray(fb, np.float32).copy()
    if edit:
        edit(fb)
    return cfg, fb


def _zero_band(fb):
    fb[7] = 0.0


def _all_zero(fb):
    fb[:] = 0.0


def cases():
    """name -> (aa_fe_config fields, dense filterbank)."""
    out = {f"bench_{n}_{h}_{m}": _case(n, h, m) for n, h, m in
           [(256, 64, 80), (512, 128, 80), (1024, 256, 80), (1024, 256, 160), (2048, 512, 80), (4096, 640, 160)]}
    out["nfft4096_fullband"] = _case(4096, 640, 160, fmin=0, fmax=24000)  # fe_stft_mel: the band leaves X[2..1022]
    out["nfft8192"] = _case(8192, 1024, 160)
    out["nfft256_fullband_40"] = _case(256, 64, 40, fmin=0, fmax=24000)
    out["nfft4096_200"] = _case(4096, 640, 200)  # 256 slots, 56 of them empty, uneven lane loads
    out["zero_band_4096"] = _case(4096, 640, 160, edit=_zero_band, mean_sub=1, channels=3, out_f16=1)
    out["zero_band_1024"] = _case(1024, 281, 80, edit=_zero_band, power=1.0)
    out["all_zero_4096"] = _case(4096, 640, 160, edit=_all_zero)
    out["all_zero_512"] = _case(512, 128, 80, edit=_all_zero)
    return out


def refusals():
    return {"hop_too_large": _case(2048, 8000, 80),
            "dense_filterbank_1024": _case(1024, 256, 64, fb=np.ones((64, 513), np.float32))}


def describe(L, make, cfg, fb, info, image):
    """What `make` (aa_fe_plan, or the recorder's aa_fe_create) yields.
    info(handle, n_win) -> dict of the aa_fe_info fields; image(handle, which)
    -> bytes."""
    from aa_amd import _lib
    c = _lib.FeConfig(**cfg)
    h = C.c_void_p()
    rc = make(C.byref(c), fb.ctypes.data, C.byref(h))
    if rc != 0:
        return {"rc": rc, "error": L.aa_last_error().decode()}
    name = C.create_string_buffer(64)
    assert L.aa_fe_stage_info(h, 1, name, 64, None, None) == 0
    out = {"rc": 0, "n_frames": L.aa_fe_n_frames(h), "stage1": name.value.decode(),
           "info": {str(n): info(h, n) for n in N_WIN},
           "workspace": {str(n): int(L.aa_fe_workspace_bytes(h, n)) for n in N_WIN},
           "images": {}}
    for w, nm in enumerate(IMAGES):
        b = image(h, w)
        out["images"][nm] = [len(b), hashlib.sha256(b).hexdigest()]
    L.aa_fe_destroy(h)
    return out
