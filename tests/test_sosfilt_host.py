"""The host side of the device band-pass filter (aa_sosfilt_plan / _run's
argument checks, aa_amd/sosfilt.py): no GPU call.

The kernels (csrc/aa_sosfilt.hip) run scipy's sosfilt as a chunked scan: a
zero-input step of the 4-vector state is s <- P s, and chunk end states are
carried forward with the powers P^(CHUNK 2^k) that aa_sosfilt_plan makes.
Checked here: those powers against numpy's matrix_power in longdouble, the
plan's and the launch's rejections, and that filtered_sources_device selects,
remaps and places exactly as windows.filtered_sources does."""
import ctypes as C
import json
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from aa_amd import _lib, sosfilt
from aa_amd.windows import butter_bandpass, filtered_sources, schedule

ROOT = Path(__file__).resolve().parent.parent
FILTERS = [(800, 3000), (0, 2500), (50, 150), (100, 110), (2000, 9000), (0, 60), (11000, 23999)]
GOLD = json.loads((Path(__file__).parent / "golden" / "filtered.json").read_text())


def _step(sos, z, x):
    """scipy's direct-form-II-transposed step in scipy's order (Python floats
    are IEEE doubles, one rounding per operation, no contraction)."""
    for s, (b0, b1, b2, _, a1, a2) in enumerate(sos):
        y = b0 * x + z[s][0]
        z[s][0] = (b1 * x - a1 * y) + z[s][1]
        z[s][1] = b2 * x - a2 * y
        x = y
    return x


def _one_step_matrix(sos):
    P = np.zeros((4, 4))
    for j in range(2 * len(sos)):
        z = [[0.0, 0.0] for _ in sos]
        z[j // 2][j % 2] = 1.0
        _step([[float(c) for c in row] for row in sos], z, 0.0)
        P[:2 * len(sos), j] = [v for zz in z for v in zz]
    return P


@pytest.mark.parametrize("band", FILTERS)
def test_step_restatement_is_scipy_bit_for_bit(band):
    """The operation order the kernels use: equal to scipy.signal.sosfilt in
    float64, bit for bit."""
    from scipy.signal import sosfilt
    sos = butter_bandpass(band[0], band[1], 48000)
    rng = np.random.default_rng(3)
    x = rng.standard_normal(3000).astype(np.float32).astype(np.float64)
    rows = [[float(c) for c in row] for row in sos]
    z = [[0.0, 0.0] for _ in rows]
    y = np.array([_step(rows, z, float(v)) for v in x])
    assert np.array_equal(y, sosfilt(sos, x))


@pytest.mark.parametrize("band", FILTERS)
def test_plan_powers(band):
    sos = butter_bandpass(band[0], band[1], 48000)
    job = sosfilt.plan_job(sos, 5, 1000, 2000)
    assert (job.src, job.n, job.dst, job.n_sections, job.n_levels) == (5, 1000, 2000, len(sos), _lib.AA_SOS_LEVELS)
    assert np.array_equal(np.array(job.sos[:6 * len(sos)]).reshape(-1, 6), sos)
    P = _one_step_matrix(sos)
    got = np.array(job.p[:]).reshape(4, 4)
    assert np.abs(got - P).max() <= 2 * np.spacing(np.abs(P).max())
    Pl = P.astype(np.longdouble)
    pw = np.array(job.pw[:]).reshape(_lib.AA_SOS_LEVELS, 4, 4)
    for k in range(_lib.AA_SOS_LEVELS):
        ref = np.linalg.matrix_power(Pl, _lib.AA_SOS_CHUNK << k)
        top = float(np.abs(ref).max())
        err = float(np.abs(pw[k].astype(np.longdouble) - ref).max())
        assert err <= 2 * np.spacing(top), (band, k, err, top)
        assert np.isfinite(pw[k]).all()


def _plan(sos, n_sections, src=0, n=10, dst=100, job=True):
    sos = np.ascontiguousarray(sos, np.float64)
    j = _lib.SosJob()
    rc = _lib.lib().aa_sosfilt_plan(sos.ctypes.data, n_sections, src, n, dst, C.byref(j) if job else None)
    return rc, _lib.lib().aa_last_error()


def test_plan_rejections():
    good = butter_bandpass(800, 3000, 48000)
    assert _plan(good, 2)[0] == _lib.AA_OK
    assert _plan(good, 2, n=0)[0] == _lib.AA_OK
    assert _plan(good, 2, n=_lib.AA_SOS_MAX_N)[0] == _lib.AA_OK
    three = np.concatenate([good, good[:1]])
    for ns in (0, 3):
        rc, msg = _plan(three, ns)
        assert rc == _lib.AA_ERR_INVALID and b"n_sections" in msg
    bad = good.copy()
    bad[1, 3] = 0.5
    rc, msg = _plan(bad, 2)
    assert rc == _lib.AA_ERR_INVALID and b"a0" in msg
    bad = good.copy()
    bad[0, 4] = np.nan
    rc, msg = _plan(bad, 2)
    assert rc == _lib.AA_ERR_INVALID and b"not finite" in msg
    for n in (-1, _lib.AA_SOS_MAX_N + 1):
        rc, msg = _plan(good, 2, n=n)
        assert rc == _lib.AA_ERR_INVALID and b"n " in msg
    rc, msg = _plan(good, 2, src=-1)
    assert rc == _lib.AA_ERR_INVALID and b"offset" in msg
    rc, msg = _plan(good, 2, job=False)
    assert rc == _lib.AA_ERR_INVALID and b"null" in msg
    assert _lib.lib().aa_sosfilt_plan(None, 2, 0, 10, 100, C.byref(_lib.SosJob())) == _lib.AA_ERR_INVALID
    # an unstable section (pole outside the unit circle): its powers overflow
    rc, msg = _plan([[1.0, 0.0, 0.0, 1.0, -4.0, 3.0]], 1)
    assert rc == _lib.AA_ERR_INVALID and b"unstable" in msg


def test_run_argument_checks_without_gpu():
    """Everything aa_sosfilt_run can refuse, it refuses before any launch:
    these calls never reach the HIP runtime (the buffers are host memory)."""
    L = _lib.lib()
    job = sosfilt.plan_job(butter_bandpass(800, 3000, 48000), 0, 5000, 5000)
    jobs = (_lib.SosJob * 1)(job)
    need = L.aa_sosfilt_workspace_bytes(jobs, 1)
    assert need == 1 * 1 * (256 * 4 + 8) * 8
    assert L.aa_sosfilt_workspace_bytes(jobs, 0) == 0 and L.aa_sosfilt_workspace_bytes(None, 1) == 0
    two = (_lib.SosJob * 2)(job, sosfilt.plan_job(butter_bandpass(0, 60, 48000), 0, 3 * 8192 + 1, 0))
    assert L.aa_sosfilt_workspace_bytes(two, 2) == 2 * 4 * (256 * 4 + 8) * 8
    pcm = np.zeros(10000, np.float32)
    ws = np.zeros(need // 8 + 2, np.float64)
    wsp = ws.ctypes.data + (-ws.ctypes.data) % 16
    jp = C.addressof(jobs)
    assert L.aa_sosfilt_run(None, 10000, jp, 1, 5000, wsp, need, None) == _lib.AA_ERR_INVALID
    assert b"null" in L.aa_last_error()
    assert L.aa_sosfilt_run(pcm.ctypes.data, 10000, None, 1, 5000, wsp, need, None) == _lib.AA_ERR_INVALID
    assert L.aa_sosfilt_run(pcm.ctypes.data, 10000, jp, 1, 5000, None, need, None) == _lib.AA_ERR_INVALID
    assert L.aa_sosfilt_run(pcm.ctypes.data, 10000, jp, -1, 5000, wsp, need, None) == _lib.AA_ERR_INVALID
    # a job longer than the buffer cannot lie inside it
    assert L.aa_sosfilt_run(pcm.ctypes.data, 4999, jp, 1, 5000, wsp, need, None) == _lib.AA_ERR_INVALID
    assert b"outside" in L.aa_last_error()
    assert L.aa_sosfilt_run(pcm.ctypes.data, 10000, jp, 1, _lib.AA_SOS_MAX_N + 1, wsp, need,
                            None) == _lib.AA_ERR_INVALID
    assert L.aa_sosfilt_run(pcm.ctypes.data, 10000, jp, 1, 5000, wsp, need - 1, None) == _lib.AA_ERR_WORKSPACE
    assert b"workspace" in L.aa_last_error()
    # nothing to do is not an error, with or without a workspace
    assert L.aa_sosfilt_run(pcm.ctypes.data, 10000, jp, 0, 0, None, 0, None) == _lib.AA_OK


def test_python_range_checks():
    """What the device cannot report, aa_amd.sosfilt refuses on the host:
    ranges outside the buffer, a destination over a source or another one."""
    sos = butter_bandpass(0, 2500, 48000)
    ok = [sosfilt.plan_job(sos, 0, 100, 200), sosfilt.plan_job(sos, 50, 100, 300)]  # overlapping sources are fine
    sosfilt.check_ranges(ok, 400)
    with pytest.raises(ValueError, match="outside"):
        sosfilt.check_ranges(ok, 399)
    with pytest.raises(ValueError, match="overlapping"):
        sosfilt.check_ranges([sosfilt.plan_job(sos, 0, 100, 200), sosfilt.plan_job(sos, 0, 100, 299)], 1000)
    with pytest.raises(ValueError, match="overwritten"):
        sosfilt.check_ranges([sosfilt.plan_job(sos, 0, 100, 99)], 1000)
    with pytest.raises(ValueError, match="overwritten"):
        sosfilt.check_ranges([sosfilt.plan_job(sos, 0, 100, 500), sosfilt.plan_job(sos, 550, 10, 700)], 1000)
    sosfilt.check_ranges([sosfilt.plan_job(sos, 0, 100, 100)], 200)  # adjacent


def _clip(n, seed):
    rng = np.random.default_rng(seed)
    return (np.round(rng.standard_normal(n) * 0.1 * 32768) / 32768).astype(np.float32)


def _track(s, e, f0, f1):
    return SimpleNamespace(start=s, end=e, freq_start=f0, freq_end=f1, length=e - s)


@pytest.mark.parametrize("case", range(len(GOLD)))
@pytest.mark.parametrize("rec_off", [0, 12345])
def test_views_and_jobs_match_the_host_function(case, rec_off):
    g = GOLD[case]
    sr = g["sr"]
    frames = _clip(g["clip_seconds"] * sr, g["clip_seed"])
    tracks = [_track(*t) for t in g["tracks"]]
    np.random.seed(g["seed"])
    views, spans = schedule(len(frames), sr, tracks, g["segment_length"], g["segment_stride"], g["fmin"],
                            g["fmax"], g["pad_short_tracks"], return_spans=True)
    base = len(frames) + 77
    extra, host_views = filtered_sources(frames, sr, tracks, views, spans, g["filter_freqs"], g["filter_below"], base)
    n_pcm = rec_off + len(frames)
    jobs, dev_views = sosfilt.filtered_sources_device(None, n_pcm, rec_off, sr, tracks, views, spans,
                                                      g["filter_freqs"], g["filter_below"], base)
    assert dev_views == host_views
    # the jobs tile the tail as the host's copies do: in track order, back to back from base
    picked = [(t, sp) for t, tv, sp in zip(tracks, views, spans)
              if tv and (g["filter_freqs"] or (g["filter_below"] and t.freq_end < g["filter_below"]))]
    assert len(jobs) == len(picked) > 0
    at = base
    for j, (t, (a, b)) in zip(jobs, picked):
        assert (j.src, j.n, j.dst) == (rec_off + a, b - a, rec_off + at)
        sos = butter_bandpass(t.freq_start, t.freq_end, sr)
        assert j.n_sections == len(sos) and np.array_equal(np.array(j.sos[:6 * len(sos)]).reshape(-1, 6), sos)
        at += b - a
    assert at - base == len(extra)


def test_filter_design_errors_surface_as_on_the_host():
    """butter() refuses a band edge at Nyquist; the device route raises the
    very same error the host route does."""
    tracks = [_track(0.0, 3.0, 100, 24000)]
    views, spans = [[(0, 144000, 0)]], [(0, 144000)]
    frames = np.zeros(144000, np.float32)
    with pytest.raises(ValueError) as host:
        filtered_sources(frames, 48000, tracks, views, spans, True, None, 144000)
    with pytest.raises(ValueError) as dev:
        sosfilt.filtered_sources_device(None, 144000, 0, 48000, tracks, views, spans, True, None, 144000)
    assert str(dev.value) == str(host.value)
    with pytest.raises(ValueError, match="outside"):
        sosfilt.filtered_sources_device(None, 1000, 0, 48000, [_track(0.0, 3.0, 100, 2000)], views, spans, True,
                                        None, 144000)


def test_constants_mirror_the_header():
    text = (ROOT / "include" / "aa.h").read_text()
    hdr = {k: int(v) for k, v in re.findall(r"^#define (AA_SOS_\w+) (\d+)", text, re.M)}
    assert hdr == {"AA_SOS_MAX_SECTIONS": _lib.AA_SOS_MAX_SECTIONS, "AA_SOS_CHUNK": _lib.AA_SOS_CHUNK,
                   "AA_SOS_BLOCK": _lib.AA_SOS_BLOCK, "AA_SOS_LEVELS": _lib.AA_SOS_LEVELS,
                   "AA_SOS_MAX_N": _lib.AA_SOS_MAX_N}
    assert (sosfilt.CHUNK, sosfilt.BLOCK) == (hdr["AA_SOS_CHUNK"], hdr["AA_SOS_BLOCK"])
    assert hdr["AA_SOS_BLOCK"] == 256 * hdr["AA_SOS_CHUNK"]
    # the struct as the header spells it
    body = re.search(r"typedef struct aa_sos_job \{(.*?)\}", re.sub(r"/\*.*?\*/", "", text, flags=re.S), re.S).group(1)
    fields = [f.strip() for f in body.split(";") if f.strip()]
    assert fields == ["int64_t src, n, dst", "int32_t n_sections", "int32_t n_levels", "double sos[12]",
                      "double p[16]", "double pw[256]"]
    assert C.sizeof(_lib.SosJob) == 3 * 8 + 2 * 4 + (12 + 16 + 256) * 8
    assert _lib.SosJob.pw.offset == 32 + 28 * 8


def test_classifier_mode(monkeypatch):
    from aa_amd.pipeline import Classifier
    monkeypatch.delenv("AA_SOSFILT", raising=False)
    assert Classifier("bf16x3", device="cpu").sosfilt == "host"
    assert Classifier("bf16x3", device="cpu", sosfilt="gpu").sosfilt == "gpu"
    with pytest.raises(ValueError, match="sosfilt"):
        Classifier("bf16x3", device="cpu", sosfilt="fpga")
    monkeypatch.setenv("AA_SOSFILT", "gpu")
    assert Classifier("bf16x3", device="cpu").sosfilt == "gpu"
    assert Classifier("bf16x3", device="cpu", sosfilt="host").sosfilt == "host"
    monkeypatch.setattr(Classifier, "_shared", {})
    a = Classifier.shared("bf16x3", "cpu")
    b = Classifier.shared("bf16x3", "cpu", sosfilt="host")
    assert a.sosfilt == "gpu" and b.sosfilt == "host" and a is not b
    assert Classifier.shared("bf16x3", "cpu", sosfilt="gpu") is a
