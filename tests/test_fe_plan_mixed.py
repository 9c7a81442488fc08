"""The front-end planner at the n_fft that are not powers of two (no GPU):
the accepted set (256..8192, a multiple of 16 whose sixteenth has no prime
factor but 2, 3, 5), the kernel and stage name, the pass schedule of
aa_fe_plan_passes, the tables, the refusals -- and a float64 numpy restatement
of the Stockham pass indexing that fe_stft_mel_mixed runs, fed with the plan's
own schedule and tables: it has to be a DFT."""
import ctypes as C

import numpy as np
import pytest

from aa_amd import _lib
from aa_amd.frontend import FeSettings

MIXED = [400, 720, 960, 1200, 1600, 1920, 2400, 3200, 3888, 4800, 6000, 6480, 7680, 7776]
REFUSED = [264, 1000, 3000, 4410, 2800, 8208, 240]
POW2 = [256, 1024, 2048, 4096, 8192]


def _cfg(n_fft, hop, n_mels=80, win_len=144000):
    return _lib.FeConfig(win_len=win_len, n_fft=n_fft, hop=hop, n_mels=n_mels, normalize=1, db_scale=1, power=2.0,
                         amin=1e-10, top_db=80.0, mean_sub=0, channels=1, out_f16=0)


def _hop(n_fft):
    return min(n_fft // 4, 1024)  # (a six-frame segment the LDS holds at every size)


def _plan(n_fft, hop=None, n_mels=80):
    hop = hop or _hop(n_fft)
    fb = np.ascontiguousarray(FeSettings(n_fft=n_fft, hop_length=hop, n_mels=n_mels, htk=True).filterbank(),
                              np.float32)
    h = C.c_void_p()
    rc = _lib.lib().aa_fe_plan(C.byref(_cfg(n_fft, hop, n_mels)), fb.ctypes.data, C.byref(h))
    assert rc == 0, (n_fft, _lib.lib().aa_last_error())
    return h


def _info(h):
    v = _lib.FeInfo()
    assert _lib.lib().aa_fe_plan_info(h, 1, C.byref(v)) == 0
    return v


def _stage1(h):
    name = C.create_string_buffer(64)
    fl, by = C.c_double(), C.c_double()
    assert _lib.lib().aa_fe_stage_info(h, 1, name, 64, C.byref(fl), C.byref(by)) == 0
    return name.value.decode(), fl.value, by.value


def _passes(h):
    L = _lib.lib()
    n = C.c_int32(-1)
    assert L.aa_fe_plan_passes(h, None, 0, C.byref(n)) == 0 and 1 <= n.value <= 8
    r = (C.c_int32 * 8)()
    assert L.aa_fe_plan_passes(h, r, 8, C.byref(n)) == 0
    return list(r[:n.value])


def _image(h, which, dtype):
    L = _lib.lib()
    n = C.c_size_t()
    assert L.aa_fe_plan_image(h, which, None, 0, C.byref(n)) == 0
    buf = np.zeros(n.value, np.uint8)
    assert L.aa_fe_plan_image(h, which, buf.ctypes.data, buf.size, C.byref(n)) == 0
    return buf.view(dtype)


@pytest.mark.parametrize("n_fft", MIXED)
def test_accepted_sizes_plan_the_mixed_kernel(n_fft):
    hop = _hop(n_fft)
    h = _plan(n_fft)
    v = _info(h)
    assert v.kernel == 3 == _lib.AA_FE_K["fe_stft_mel_mixed"]
    name, flops, nbytes = _stage1(h)
    assert name == "fe_stft_mel_mixed" and flops > 0 and nbytes > 0
    assert v.T == 1 + 144000 // hop == _lib.lib().aa_fe_n_frames(h)
    # the generic kernel's rules: six frames per block, one partial maximum per block, LDS inside the bound
    assert v.nparts == -(-v.T // 6) and v.grid == min(v.nparts, 256 * max(1, (160 * 1024) // (v.lds_bytes + 256)))
    assert 0 < v.lds_bytes <= 150 * 1024
    _lib.lib().aa_fe_destroy(h)


@pytest.mark.parametrize("n_fft", MIXED)
def test_schedule_properties(n_fft):
    h = _plan(n_fft)
    r = _passes(h)
    nc = n_fft // 2
    assert r[0] == 8 and set(r) <= {2, 3, 4, 5, 8} and len(r) <= 8
    assert int(np.prod(r)) == nc
    ns = 1
    for i, ri in enumerate(r):
        assert i == 0 or ns % 8 == 0
        ns *= ri
    # the documented order: 8s, 5s, one 4, 3s, one 2
    rank = {8: 0, 5: 1, 4: 2, 3: 3, 2: 4}
    assert [rank[x] for x in r] == sorted(rank[x] for x in r)
    assert r.count(4) <= 1 and r.count(2) <= 1 and not (4 in r and 2 in r)
    # a buffer that is too short: AA_ERR_INVALID with the count set
    L = _lib.lib()
    n = C.c_int32(-1)
    short = (C.c_int32 * 8)()
    assert L.aa_fe_plan_passes(h, short, len(r) - 1, C.byref(n)) == _lib.AA_ERR_INVALID and n.value == len(r)
    L.aa_fe_destroy(h)


def test_schedule_examples():
    want = {400: [8, 5, 5], 1200: [8, 5, 5, 3], 4800: [8, 5, 5, 4, 3], 2400: [8, 5, 5, 3, 2],
            7776: [8, 3, 3, 3, 3, 3, 2], 7680: [8, 8, 5, 4, 3], 6000: [8, 5, 5, 5, 3]}
    for n_fft, r in want.items():
        h = _plan(n_fft)
        assert _passes(h) == r, n_fft
        _lib.lib().aa_fe_destroy(h)


@pytest.mark.parametrize("n_fft", MIXED)
def test_tables_are_the_rounded_float64_definitions(n_fft):
    h = _plan(n_fft)
    nc = n_fft // 2
    hann = _image(h, 0, np.float32)
    tw = _image(h, 1, np.float32).reshape(-1, 2)
    tw2 = _image(h, 2, np.float32).reshape(-1, 2)
    assert hann.shape == (n_fft,) and tw.shape == (nc, 2) and tw2.shape == (nc + 1, 2)
    assert (hann == (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)).astype(np.float32)).all()
    for img, den, cnt in ((tw, nc, nc), (tw2, n_fft, nc + 1)):
        a = -2 * np.pi * np.arange(cnt) / den
        assert (img[:, 0] == np.cos(a).astype(np.float32)).all()
        assert (img[:, 1] == np.sin(a).astype(np.float32)).all()
    n = C.c_size_t()
    assert _lib.lib().aa_fe_plan_image(h, 5, None, 0, C.byref(n)) == 0 and n.value == 0
    assert _lib.lib().aa_fe_plan_image(h, 6, None, 0, C.byref(n)) == _lib.AA_ERR_INVALID
    _lib.lib().aa_fe_destroy(h)


@pytest.mark.parametrize("n_fft", REFUSED)
def test_refused_sizes(n_fft):
    L = _lib.lib()
    fb = np.zeros((80, n_fft // 2 + 1), np.float32)
    got = []
    for make in (L.aa_fe_plan, L.aa_fe_create):
        h = C.c_void_p()
        rc = make(C.byref(_cfg(n_fft, 64)), fb.ctypes.data, C.byref(h))
        msg = L.aa_last_error()
        assert rc == _lib.AA_ERR_UNSUPPORTED == 3 and not h.value
        assert b"n_fft" in msg and b"256..8192" in msg and str(n_fft).encode() in msg
        got.append(msg)
    assert got[0] == got[1]


def test_hop_too_large_for_the_segment():
    L = _lib.lib()
    fb = np.ascontiguousarray(FeSettings(n_fft=4800, hop_length=8000, n_mels=80, htk=True).filterbank(), np.float32)
    h = C.c_void_p()
    assert L.aa_fe_plan(C.byref(_cfg(4800, 8000)), fb.ctypes.data, C.byref(h)) == _lib.AA_ERR_UNSUPPORTED
    assert b"hop 8000 too large for the LDS segment" in L.aa_last_error() and not h.value


@pytest.mark.parametrize("n_fft", POW2)
def test_powers_of_two_keep_their_kernel(n_fft):
    hop = {256: 64, 1024: 256, 2048: 512, 4096: 640, 8192: 1024}[n_fft]
    h = _plan(n_fft, hop, 160 if n_fft >= 4096 else 80)
    want = {256: "fe_stft_mel_small", 1024: "fe_stft_mel_small", 2048: "fe_stft_mel", 4096: "fe_stft_mel_4096",
            8192: "fe_stft_mel"}[n_fft]
    assert _stage1(h)[0] == want and _info(h).kernel == _lib.AA_FE_K[want]
    r = _passes(h)
    assert int(np.prod(r)) == n_fft // 2
    if want == "fe_stft_mel":
        assert r == [8, 8, 8, n_fft // 1024]
    _lib.lib().aa_fe_destroy(h)


def test_generic_4096_reports_8_8_8_4():
    fb = np.ascontiguousarray(FeSettings(n_fft=4096, hop_length=640, n_mels=160, htk=True, fmin=0,
                                         fmax=24000).filterbank(), np.float32)
    h = C.c_void_p()
    assert _lib.lib().aa_fe_plan(C.byref(_cfg(4096, 640, 160)), fb.ctypes.data, C.byref(h)) == 0
    assert _stage1(h)[0] == "fe_stft_mel" and _passes(h) == [8, 8, 8, 4]
    _lib.lib().aa_fe_destroy(h)


# ---- the pass indexing restated in numpy (float64) ----------------------------
def _pidx(i):
    return i + (i >> 3)


def _stockham(z, radices, tw):
    """The passes as fe_stft_mel_mixed runs them on its padded buffers: pass 1
    reads point j + q NC/8 and writes 8 j + q; a later pass of radix r at
    sub-transform size NS reads src[pidx(j + q NB)], NB = NC / r, multiplies
    by tw[q k NC / (NS r)], k = j % NS, takes the r-point DFT over q and writes
    dst[pidx((j / NS) NS r + k + q NS)]."""
    nc = len(z)
    src = np.zeros(nc + nc // 8, complex)
    src[_pidx(np.arange(nc))] = z
    ns = 1
    for r in radices:
        nb = nc // r
        dft = np.exp(-2j * np.pi * np.outer(np.arange(r), np.arange(r)) / r)
        dst = np.full(nc + nc // 8, np.nan, complex)
        j = np.arange(nb)
        k = j % ns
        q = np.arange(r)[:, None]
        e = q * k * (nc // (ns * r))
        assert e.max() < nc  # the exponent needs no reduction mod NC
        v = src[_pidx(j + q * nb)] * tw[e]
        dst[_pidx((j // ns) * ns * r + k + q * ns)] = dft @ v
        assert ns == 1 or (np.array_equal(_pidx(j + q * nb), _pidx(j) + q * (nb + nb // 8)))
        src, ns = dst, ns * r
    return src[_pidx(np.arange(nc))]


@pytest.mark.parametrize("n_fft", [400, 1200, 4800, 7776])
def test_schedule_and_tables_describe_a_dft(n_fft):
    h = _plan(n_fft)
    nc = n_fft // 2
    r = _passes(h)
    tw = _image(h, 1, np.float32).astype(np.float64).reshape(-1, 2) @ np.array([1, 1j])
    tw2 = _image(h, 2, np.float32).astype(np.float64).reshape(-1, 2) @ np.array([1, 1j])
    _lib.lib().aa_fe_destroy(h)
    rng = np.random.default_rng(n_fft)
    x = rng.standard_normal(n_fft)
    z = x[0::2] + 1j * x[1::2]
    Z = _stockham(z, r, tw)
    assert np.abs(Z - np.fft.fft(z)).max() <= 2e-6 * np.abs(np.fft.fft(z)).max()
    # the real split, k = 0 and k = NC apart: X = E + W^k O
    X = np.empty(nc + 1, complex)
    X[0], X[nc] = Z[0].real + Z[0].imag, Z[0].real - Z[0].imag
    k = np.arange(1, nc)
    a, b = Z[k], np.conj(Z[nc - k])
    X[k] = 0.5 * (a + b) + tw2[k] * (-0.5j) * (a - b)
    ref = np.fft.rfft(x)
    err = np.abs(X - ref).max() / np.abs(ref).max()
    print(f"n_fft {n_fft} passes {r}: max|X - rfft| / peak = {err:.2e}")
    assert err <= 2e-6
