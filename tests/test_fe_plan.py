"""The front-end planner on the CPU (aa_fe_plan / aa_fe_plan_info /
aa_fe_plan_image, no GPU).

* Every field of the plan -- kernel, T, kmin, kmax, nnz, nparts, LDS bytes and
  grid at 1 and 64 windows, the workspace sizes, the stft stage's name, and the
  byte length + SHA-256 of the six images -- equals what the commit named in
  tests/golden/fe_plan_parent.json computed for the same configurations and
  filterbanks (recorded by tests/golden/make_fe_plan_golden.py from its
  aa_fe_create, with the upload writing its bytes to files instead of the
  device); the refusals return that commit's codes and aa_last_error texts.
* Two layouts are stated independently in numpy, from their descriptions in
  csrc/aa_fe_plan.h (CSR rows and values; fe_stft_mel_4096's image), not from
  the packers.
"""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

import fe_plan_cases as fc
from aa_amd import _lib

GOLDEN = Path(__file__).resolve().parent / "golden" / "fe_plan_parent.json"


def info(h, n_win):
    v = _lib.FeInfo()
    assert _lib.lib().aa_fe_plan_info(h, n_win, C.byref(v)) == 0
    return {f: int(getattr(v, f)) for f, _ in _lib.FeInfo._fields_}


def image(h, which):
    L = _lib.lib()
    n = C.c_size_t()
    assert L.aa_fe_plan_image(h, which, None, 0, C.byref(n)) == 0
    buf = np.zeros(n.value, np.uint8)
    assert L.aa_fe_plan_image(h, which, buf.ctypes.data, buf.size, C.byref(n)) == 0
    return buf.tobytes()


def plan(cfg, fb):
    L = _lib.lib()
    return fc.describe(L, L.aa_fe_plan, cfg, fb, info, image)


def planned(cfg, fb):
    h = C.c_void_p()
    assert _lib.lib().aa_fe_plan(C.byref(_lib.FeConfig(**cfg)), fb.ctypes.data, C.byref(h)) == 0
    return h


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


@pytest.mark.parametrize("case", sorted(fc.cases()))
def test_plan_equals_parent(golden, case):
    want = golden["cases"][case]
    got = plan(*fc.cases()[case])
    assert want["rc"] == 0 and got["rc"] == 0, got
    for k in ("n_frames", "stage1", "info", "workspace", "images"):
        assert got[k] == want[k], k
    assert got == want


@pytest.mark.parametrize("name", sorted(fc.refusals()))
def test_refusal_equals_parent(golden, name):
    want = golden["refusals"][name]
    assert want["rc"] == _lib.AA_ERR_UNSUPPORTED
    assert plan(*fc.refusals()[name]) == want


def test_cases_cover_what_they_are_meant_to(golden):
    c = golden["cases"]
    assert {k: v["stage1"] for k, v in c.items() if k.startswith("bench_")} == {
        "bench_256_64_80": "fe_stft_mel_small", "bench_512_128_80": "fe_stft_mel_small",
        "bench_1024_256_80": "fe_stft_mel_small", "bench_1024_256_160": "fe_stft_mel_small",
        "bench_2048_512_80": "fe_stft_mel", "bench_4096_640_160": "fe_stft_mel_4096"}
    for k, v in c.items():
        assert v["info"]["1"]["kernel"] == _lib.AA_FE_K[v["stage1"]], k
        assert (v["images"]["cimg4096"][0] > 0) == ("4096" in k), k
    assert c["nfft4096_fullband"]["stage1"] == "fe_stft_mel" and c["nfft4096_fullband"]["info"]["1"]["kmax"] > 1022
    assert c["nfft8192"]["stage1"] == "fe_stft_mel" and c["nfft8192"]["n_frames"] == 141
    assert c["nfft4096_200"]["stage1"] == "fe_stft_mel_4096"
    assert c["all_zero_4096"]["info"]["1"] | {"grid": 0, "lds_bytes": 0} == {
        "kernel": 2, "T": 226, "kmin": 0, "kmax": 0, "nnz": 0, "nparts": 38, "lds_bytes": 0, "grid": 0}
    assert "hop 8000 too large for the LDS segment" in golden["refusals"]["hop_too_large"]["error"]
    assert "too large for the LDS" in golden["refusals"]["dense_filterbank_1024"]["error"]


@pytest.mark.parametrize("n_fft", [128, 1000, 3000, 16384])
def test_refused_sizes_as_aa_fe_create(n_fft):
    """tests/test_fe_sizes.py through aa_fe_plan: the same code and text."""
    L = _lib.lib()
    cfg = _lib.FeConfig(win_len=144000, n_fft=n_fft, hop=640, n_mels=160, normalize=1,
                        db_scale=1, power=2.0, amin=1e-10, top_db=80.0, mean_sub=0, channels=1)
    fb = np.zeros((160, n_fft // 2 + 1), np.float32)
    got = []
    for make in (L.aa_fe_create, L.aa_fe_plan):
        h = C.c_void_p()
        got.append((make(C.byref(cfg), fb.ctypes.data, C.byref(h)), L.aa_last_error(), h.value))
    assert got[0] == got[1]
    rc, msg, handle = got[1]
    assert rc == _lib.AA_ERR_UNSUPPORTED == 3 and not handle
    assert b"n_fft" in msg and b"256..8192" in msg and str(n_fft).encode() in msg


def test_null_and_bad_sizes():
    L = _lib.lib()
    h = C.c_void_p()
    cfg, fb = fc.cases()["bench_2048_512_80"]
    assert L.aa_fe_plan(None, fb.ctypes.data, C.byref(h)) == _lib.AA_ERR_INVALID
    assert L.aa_last_error() == b"aa_fe_create: null argument"
    assert L.aa_fe_plan(C.byref(_lib.FeConfig(**cfg)), fb.ctypes.data, None) == _lib.AA_ERR_INVALID
    for bad in (dict(hop=0), dict(n_mels=0), dict(channels=0), dict(out_f16=2), dict(win_len=0)):
        assert L.aa_fe_plan(C.byref(_lib.FeConfig(**{**cfg, **bad})), fb.ctypes.data, C.byref(h)) == _lib.AA_ERR_INVALID
        assert L.aa_last_error() == b"aa_fe_create: bad sizes" and not h.value


def test_planned_plan_refuses_to_run():
    L = _lib.lib()
    h = planned(*fc.cases()["bench_2048_512_80"])
    x = np.zeros(4, np.float32)
    assert L.aa_fe_run(h, x.ctypes.data, 4, x.ctypes.data, 1, x.ctypes.data, None, x.ctypes.data, 1 << 30,
                       None) == _lib.AA_ERR_INVALID
    assert b"aa_fe_plan" in L.aa_last_error()
    assert L.aa_fe_set_timing(h, 2) == _lib.AA_ERR_INVALID
    assert L.aa_fe_stage_time(h, 1, None, None) == _lib.AA_ERR_INVALID
    assert L.aa_fe_n_stages(h) == 3
    n = C.c_size_t()
    small = np.zeros(8, np.uint8)
    assert L.aa_fe_plan_image(h, 0, small.ctypes.data, 8, C.byref(n)) == _lib.AA_ERR_INVALID and n.value == 2048 * 4
    assert L.aa_fe_plan_image(h, 6, None, 0, C.byref(n)) == _lib.AA_ERR_INVALID
    assert L.aa_fe_plan_image(h, 5, None, 0, C.byref(n)) == 0 and n.value == 0  # no 4096 image at 2048
    assert L.aa_fe_destroy(h) == 0


# ---- layouts stated independently --------------------------------------------
def images_of(case):
    cfg, fb = fc.cases()[case]
    h = planned(cfg, fb)
    out = [image(h, w) for w in range(6)]
    v = info(h, 1)
    _lib.lib().aa_fe_destroy(h)
    return cfg, fb, v, out


@pytest.mark.parametrize("case", ["bench_1024_256_160", "zero_band_4096", "all_zero_512", "nfft4096_fullband"])
def test_csr_from_its_description(case):
    """aa_fe_plan.h: per band (first nonzero bin, count up to the last nonzero
    bin, offset of its values, 0), the values of [first, last] in band order;
    kmin / kmax the extreme bins over all bands (0, 0 when none); an all-zero
    band is (kmin, 0, offset, 0); an empty filterbank keeps one 0.0 value."""
    cfg, fb, v, img = images_of(case)
    rows = np.frombuffer(img[3], np.int32).reshape(-1, 4)
    vals = np.frombuffer(img[4], np.float32)
    nz = [np.flatnonzero(r) for r in fb]
    used = [k for k in nz if k.size]
    kmin = min(k[0] for k in used) if used else 0
    kmax = max(k[-1] for k in used) if used else 0
    assert (v["kmin"], v["kmax"]) == (kmin, kmax) and rows.shape == (cfg["n_mels"], 4)
    off = 0
    for m, k in enumerate(nz):
        if k.size == 0:
            assert tuple(rows[m]) == (kmin, 0, off, 0)
            continue
        n = k[-1] - k[0] + 1
        assert tuple(rows[m]) == (k[0], n, off, 0)
        assert (vals[off:off + n] == fb[m, k[0]:k[-1] + 1]).all()
        off += n
    assert v["nnz"] == off and vals.size == max(off, 1) and (off or vals[0] == 0.0)


@pytest.mark.parametrize("case", ["bench_4096_640_160", "nfft4096_200", "zero_band_4096", "all_zero_4096"])
def test_4096_image_from_its_description(case):
    """aa_fe_plan.h (fe_cimg4096): slots = n_mels rounded up to 64, 16 bytes
    each (first bin, padded length, value offset, band), then the values; a
    band's values are reversed (last bin first) and zero-padded at the front to
    a multiple of 4; empty slots are (kmin + 3, 0, 0, -1); every band sits in
    exactly one slot; the image is zero-padded to whole KiB."""
    cfg, fb, v, img = images_of(case)
    csr = np.frombuffer(img[3], np.int32).reshape(-1, 4)
    raw = np.frombuffer(img[5], np.uint8)
    nslot = (cfg["n_mels"] + 63) // 64 * 64
    slots = raw[:16 * nslot].view(np.int32).reshape(nslot, 4)
    vals = raw[16 * nslot:].view(np.float32)
    assert raw.size % 1024 == 0
    seen, end = [], 0
    for x, n4, off, band in slots:
        if band < 0:
            assert (x, n4, off, band) == (v["kmin"] + 3, 0, 0, -1)
            continue
        seen.append(band)
        first, n = csr[band][0], csr[band][1]
        assert x == first and n4 == (n + 3) // 4 * 4 and off % 4 == 0
        row = vals[off:off + n4]
        assert not row[:n4 - n].any() and (row[n4 - n:] == fb[band, first:first + n][::-1]).all()
        end = max(end, off + n4)
    assert sorted(seen) == list(range(cfg["n_mels"]))
    assert not vals[end:].any() and raw.size == (16 * nslot + 4 * end + 1023) // 1024 * 1024
    if case == "nfft4096_200":
        # 256 slots; the lanes' summed row lengths stay close (longest row first
        # to the least-loaded lane): no lane carries more than one longest row
        # above the lightest
        load = np.zeros(64, int)
        for i, s in enumerate(slots):
            load[i % 64] += s[1]
        assert nslot == 256 and load.max() - load.min() <= slots[:, 1].max()
