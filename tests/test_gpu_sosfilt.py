"""The device band-pass filter (aa_sosfilt_run, csrc/aa_sosfilt.hip) against
scipy.signal.sosfilt in float64, and the classifier's "gpu" filter mode
against its "host" mode and the CPU oracle.

Tolerance of every sample comparison: with y64 = sosfilt(sos, x) in float64, a
device sample g passes iff

    |g - y64| <= 2^-24 |y64| + tau max|x|,  tau = 4 max|y_chunked - y64| / max|x|

2^-24 |y64| is the one rounding to f32.  y_chunked (``_chunked`` below) is a
float64 numpy restatement of the kernel's algorithm at the kernel's CHUNK, run
on the very input checked: chunks from zero state, the end states carried
forward by a Kogge-Stone scan with numpy's matrix_power (longdouble, rounded to
float64), chunks rerun from the carried states.  Its distance from y64 is what
handing a rounded state across chunk borders costs (1e-15 .. 2e-11 of max|x|
over the filters here, largest for the band against Nyquist); 4 is the
project's margin over an emulation.  Where no state is handed over (the first
chunk of every job) the device must equal float32(y64) bit for bit.
"""
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SR = 48000
FILTERS = [(800, 3000), (0, 2500), (50, 150), (100, 110), (2000, 9000), (0, 60), (11000, 23999)]
GUARD = np.float32(12345.0)
WAVE = 64  # lanes of one wave of the carry scan


def _consts():
    from aa_amd import sosfilt
    return sosfilt.CHUNK, sosfilt.BLOCK


def _lengths():
    L, B = _consts()
    return [1, L - 1, L, L + 1, B - 1, B, B + 1, 2 * B + L + 3, B * (WAVE + 1) + 17]


_SIGNAL = {}


def _signal():
    """tools/synth noise and chirps plus a 120 Hz tone, f32 on the PCM16 grid."""
    if "x" not in _SIGNAL:
        from tools import synth
        seconds = 45.0  # the longest job: 257 workgroup spans
        _SIGNAL["x"] = (synth.clip(7, seconds=seconds) + synth.tone(120.0, seconds=seconds, amp=0.25)).astype(
            np.float32)
    return _SIGNAL["x"]


def _sos(band):
    from aa_amd.windows import butter_bandpass
    return butter_bandpass(band[0], band[1], SR)


def _one_step_matrix(sos):
    """P: the state (z0, z1 per section) after one zero-input step from each
    unit state, in sosfilt's own arithmetic."""
    from scipy.signal import sosfilt
    ns = len(sos)
    P = np.zeros((4, 4))
    for j in range(2 * ns):
        zi = np.zeros((ns, 2))
        zi[j // 2, j % 2] = 1.0
        _, zf = sosfilt(sos, np.zeros(1), zi=zi)
        P[:2 * ns, j] = zf.reshape(-1)
    return P


def _chunked(sos, x, chunk):
    """The chunked algorithm in float64 numpy (the emulation, not the code
    under test)."""
    from scipy.signal import sosfilt
    ns, n = len(sos), len(x)
    C = -(-n // chunk)
    X = np.zeros(C * chunk)
    X[:n] = x
    X = X.reshape(C, chunk)
    _, zf = sosfilt(sos, X, axis=-1, zi=np.zeros((ns, C, 2)))
    # w_0 = 0, w_c = e_(c-1); the inclusive scan of w is each chunk's start state
    w = np.zeros((C, 4))
    w[1:, :2 * ns] = np.moveaxis(zf, 0, 1).reshape(C, 2 * ns)[:-1]
    Pl = _one_step_matrix(sos).astype(np.longdouble)
    k = 0
    while (1 << k) < C:
        d = 1 << k
        M = np.linalg.matrix_power(Pl, chunk * d).astype(np.float64)
        w[d:] = w[d:] + w[:-d] @ M.T
        k += 1
    zi = np.moveaxis(w[:, :2 * ns].reshape(C, ns, 2), 0, 1)
    Y, _ = sosfilt(sos, X, axis=-1, zi=np.ascontiguousarray(zi))
    return Y.reshape(-1)[:n]


_REF = {}


def _reference(band, x_key, x):
    """(y64, tau * max|x|) of one filter on one input, computed once."""
    key = (band, x_key)
    if key not in _REF:
        from scipy.signal import sosfilt
        L, _ = _consts()
        sos = _sos(band)
        x64 = x.astype(np.float64)
        y64 = sosfilt(sos, x64)
        dev = float(np.abs(_chunked(sos, x64, L) - y64).max()) if len(x) else 0.0
        y64.setflags(write=False)
        _REF[key] = (y64, 4.0 * dev)
    return _REF[key]


def _check(g, y64, slack, what):
    """The tolerance rule; returns (worst |g - y64| / slack, the share of the
    slack the worst sample uses beyond its f32 rounding, share of g != f32(y64))."""
    assert np.isfinite(g).all(), what
    err = np.abs(g.astype(np.float64) - y64)
    bound = 2.0 ** -24 * np.abs(y64) + slack
    bad = np.flatnonzero(err > bound)
    assert bad.size == 0, (what, int(bad[0]), float(err[bad[0]]), float(bound[bad[0]]))
    used = float(((err - 2.0 ** -24 * np.abs(y64)) / slack).max()) if slack else 0.0
    return (float(err.max() / slack) if slack else 0.0), used, float(np.mean(g != y64.astype(np.float32)))


def _up3(i):
    """The next offset that is 3 mod 4 (odd, and off the 16-byte grid)."""
    return i + (3 - i) % 4


def _launch(gpu, buf, specs):
    """specs: (band, src, n, dst); one aa_sosfilt_run over a device copy of buf."""
    import torch
    from aa_amd import sosfilt
    pcm = torch.from_numpy(buf).to(gpu)
    sosfilt.run(pcm, [sosfilt.plan_job(_sos(band), src, n, dst) for band, src, n, dst in specs])
    return pcm.cpu().numpy()


_GEOMETRY = {}


def _geometry(gpu, band):
    """Every length of _lengths() through one filter, one launch each; src and
    dst both 3 mod 4.  [(n, device output, input)]"""
    if band not in _GEOMETRY:
        x = _signal()
        out = []
        for i, n in enumerate(_lengths()):
            src = 3
            dst = _up3(src + n + 5)
            buf = np.full(dst + n + 9, GUARD, np.float32)
            xin = x[1000 * i:1000 * i + n]
            buf[src:src + n] = xin
            res = _launch(gpu, buf, [(band, src, n, dst)])
            keep = np.ones(len(buf), bool)
            keep[dst:dst + n] = False
            assert np.array_equal(res[keep], buf[keep]), (band, n)  # sources and guards untouched
            out.append((n, res[dst:dst + n], xin))
        _GEOMETRY[band] = out
    return _GEOMETRY[band]


@pytest.mark.parametrize("band", FILTERS)
def test_geometries(gpu, band):
    worst, used, mism = 0.0, -np.inf, 0.0
    for i, (n, g, xin) in enumerate(_geometry(gpu, band)):
        y64, slack = _reference(band, ("geo", i), xin)
        w, u, m = _check(g, y64, slack, (band, n))
        worst, used, mism = max(worst, w), max(used, u), max(mism, m)
        print(f"sosfilt {band} n={n}: tau*max|x|={slack:.2e}  max|g-y64|/(tau max|x|)={w:.4g}  "
              f"beyond f32 rounding: {u:.3f} of tau max|x|  g != f32(y64): {100 * m:.4f} %")
    print(f"sosfilt {band}: worst max|g-y64|/(tau max|x|) {worst:.4g} (f32 rounding included), "
          f"worst share of tau max|x| used beyond f32 rounding {used:.3f}, worst mismatch share {100 * mism:.4f} %")


@pytest.mark.parametrize("band", FILTERS)
def test_first_chunk_is_bit_exact(gpu, band):
    """No carry enters the first chunk: any contraction or reordering of the
    per-sample arithmetic shows here."""
    L, _ = _consts()
    for i, (n, g, xin) in enumerate(_geometry(gpu, band)):
        y64, _ = _reference(band, ("geo", i), xin)
        assert np.array_equal(g[:L].view(np.int32), y64[:L].astype(np.float32).view(np.int32)), (band, n)


@pytest.mark.parametrize("band", [(800, 3000), (0, 60)])
def test_carry_kernel_second_round(gpu, band):
    """More workgroup aggregates than the carry kernel scans in one round
    (256): the last state of a round enters the next."""
    _, B = _consts()
    n = 257 * B + 5
    x = _signal()
    assert len(x) >= n
    src, dst = 3, _up3(3 + n + 2)
    buf = np.full(dst + n + 4, GUARD, np.float32)
    buf[src:src + n] = x[:n]
    res = _launch(gpu, buf, [(band, src, n, dst)])
    y64, slack = _reference(band, ("long", n), x[:n])
    w, u, m = _check(res[dst:dst + n], y64, slack, (band, n))
    print(f"sosfilt {band} n={n}: max|g-y64|/(tau max|x|)={w:.4g}  beyond f32 rounding: {u:.3f} of tau max|x|  "
          f"g != f32(y64): {100 * m:.4f} %")
    assert (res[dst + n:] == GUARD).all() and (res[:src] == GUARD).all()


def _multi_specs():
    L, B = _consts()
    lengths = [1, L + 1, B - 1, B + 1, 2 * B + L + 3, 3 * B + 5]
    bands = [(800, 3000), (0, 2500), (50, 150), (0, 60), (800, 3000), (0, 2500)]  # 2 sections, 1, 2, 1, ...
    srcs = [1 + 5 * i for i in range(6)]  # overlapping sources, every alignment
    region = max(s + n for s, n in zip(srcs, lengths))
    specs, at = [], region + 3
    for band, s, n in zip(bands, srcs, lengths):
        specs.append((band, s, n, at))
        at += n + 1 + len(specs)  # guard gaps of growing width: every dst alignment
    return specs, region, at + 8


def test_multi_job_launch(gpu):
    specs, region, total = _multi_specs()
    buf = np.full(total, GUARD, np.float32)
    buf[:region] = _signal()[5000:5000 + region]
    first = _launch(gpu, buf, specs)
    again = _launch(gpu, buf, specs)
    assert np.array_equal(first.view(np.int32), again.view(np.int32))  # deterministic
    keep = np.ones(total, bool)
    for band, src, n, dst in specs:
        alone = _launch(gpu, buf, [(band, src, n, dst)])
        assert np.array_equal(first[dst:dst + n].view(np.int32), alone[dst:dst + n].view(np.int32)), (band, n)
        y64, slack = _reference(band, ("multi", src, n), buf[src:src + n])
        _check(first[dst:dst + n], y64, slack, (band, n))
        keep[dst:dst + n] = False
    assert np.array_equal(first[keep].view(np.int32), buf[keep].view(np.int32))  # guards and the source region


@pytest.mark.parametrize("band", [(800, 3000), (0, 2500)])
def test_nan_poisons_what_follows_and_nothing_before(gpu, band):
    L, B = _consts()
    n, k = 2 * B + L + 3, B + L // 2
    src, dst = 3, _up3(3 + n + 1)
    buf = np.full(dst + n + 2, GUARD, np.float32)
    buf[src:src + n] = _signal()[:n]
    buf[src + k] = np.nan
    res = _launch(gpu, buf, [(band, src, n, dst)])
    g = res[dst:dst + n]
    y64, slack = _reference(band, ("nan", k), buf[src:src + k])  # causal: outputs < k see x[:k] only
    _check(g[:k], y64, slack, (band, "before the NaN"))
    assert np.isnan(g[k:]).all()
    assert (res[dst + n:] == GUARD).all()


# ---- the classifier's "gpu" mode ------------------------------------------------------------

def _track(s, e, f0=0, f1=24000):
    return SimpleNamespace(start=s, end=e, freq_start=f0, freq_end=f1, length=e - s, results=[])


def _tracks():
    return [_track(0.5, 6.0, 800, 3000), _track(6.5, 11.0, 2000, 9000), _track(3.0, 4.0, 0, 2500)]


def _model(tmp_path, name, **kw):
    import json
    from tools.make_models import make_model
    p = make_model(tmp_path / name, name=name, seed=4, **kw)
    meta = json.loads((p.parent / "metadata.txt").read_text())
    return p.with_suffix(".keras"), meta


def _oracle(frames, tracks, group, meta, seed=5):
    """As tests/test_gpu_pipeline.py computes it: host sosfilt, CPU log-mel, CPU CNN."""
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


def _no_host_samples():
    raise AssertionError("the gpu filter mode must not ask for host samples")


def _capture(monkeypatch):
    from aa_amd import pipeline
    got = {}

    def capture(tr, sel, means, meta):
        for row, ti in enumerate(sel):
            got[(id(tr), ti)] = means[row].copy()
    monkeypatch.setattr(pipeline, "apply_group_scores", capture)
    return got


@pytest.mark.parametrize("mode", ["filter_freq", "filter_below"])
def test_pipeline_gpu_mode(gpu, monkeypatch, tmp_path, mode):
    import torch
    from aa_amd import pipeline
    from tools import synth
    over = {"filter_freq": True} if mode == "filter_freq" else {"filter_below": 4000}
    path, meta = _model(tmp_path, "m_" + mode, meta_overrides=over)
    frames = synth.clip(21, seconds=12.0)
    group = [(path, meta)]
    got = _capture(monkeypatch)

    tracks = _tracks()
    rec = pipeline.BatchRec(n=len(frames), off=0, tracks=tracks, frames=_no_host_samples, seed=None)
    np.random.seed(5)
    clf = pipeline.Classifier("bf16x3", device=gpu, sosfilt="gpu")
    res = clf.classify_batch(torch.from_numpy(frames).to(gpu), 48000, [rec], [group], raise_errors=True)
    assert not isinstance(res[0], BaseException)
    dev = {ti: v for (tid, ti), v in got.items() if tid == id(tracks)}

    host_tracks = _tracks()
    np.random.seed(5)
    pipeline.Classifier("bf16x3", device=gpu, sosfilt="host").classify_tracks(frames, 48000, host_tracks, [group])
    host = {ti: v for (tid, ti), v in got.items() if tid == id(host_tracks)}

    ref = _oracle(frames, _tracks(), group, meta)
    assert sorted(dev) == sorted(host) == sorted(ref) == [0, 1, 2]
    d_ref = max(float(np.abs(dev[k] - ref[k]).max()) for k in ref)
    d_host = max(float(np.abs(dev[k] - host[k]).max()) for k in ref)
    print(f"{mode}: gpu filter vs oracle {d_ref:.2e}, vs host filter mode {d_host:.2e}")
    assert d_ref <= 1e-3
    assert d_host <= 1e-5


def test_batched_recordings_score_as_alone(gpu, monkeypatch, tmp_path):
    """Two recordings in one classify_batch, the second at an odd offset: each
    gets, bit for bit, the scores it gets alone at offset 0."""
    import torch
    from aa_amd import pipeline
    from tools import synth
    path, meta = _model(tmp_path, "m_batch", meta_overrides={"filter_freq": True})
    group = [(path, meta)]
    a = synth.clip(31, seconds=9.0)[:-3]   # 431997 samples: b starts off the 16-byte grid
    b = synth.clip(32, seconds=7.0)
    got = _capture(monkeypatch)
    clf = pipeline.Classifier("bf16x3", device=gpu, sosfilt="gpu")

    def rec(x, off, tracks, seed):
        return pipeline.BatchRec(n=len(x), off=off, tracks=tracks, frames=_no_host_samples, seed=seed)

    def tracks_a():
        return [_track(0.5, 6.0, 800, 3000), _track(3.0, 4.0, 0, 2500)]

    def tracks_b():
        return [_track(1.0, 6.5, 2000, 9000), _track(0.0, 2.0, 50, 150)]

    ta, tb = tracks_a(), tracks_b()
    both = torch.from_numpy(np.concatenate([a, b])).to(gpu)
    res = clf.classify_batch(both, 48000, [rec(a, 0, ta, 11), rec(b, len(a), tb, 12)], [group], raise_errors=True)
    assert not any(isinstance(r, BaseException) for r in res)
    sa, sb = tracks_a(), tracks_b()
    clf.classify_batch(torch.from_numpy(a).to(gpu), 48000, [rec(a, 0, sa, 11)], [group], raise_errors=True)
    clf.classify_batch(torch.from_numpy(b).to(gpu), 48000, [rec(b, 0, sb, 12)], [group], raise_errors=True)
    for batch, solo in ((ta, sa), (tb, sb)):
        for ti in range(2):
            x, y = got[(id(batch), ti)], got[(id(solo), ti)]
            assert np.array_equal(x.view(np.int32), y.view(np.int32)), (ti, x, y)
