"""The old cacophony index on the device (csrc/aa_cacophony.hip, aa_amd/
cacophony_index.py) against the reference's recorded results
(tests/golden/cacophony_index.json) and the restated algorithm
(tests/ci_restated.py, pinned to the reference by tests/test_cacophony_host.py).

Band energies: digital silence must give exactly 0.0; elsewhere the relative
deviation from the restated float64 energies (scipy.fftpack.dct) is gated at
8 x the deviation numpy's FFT through Makhoul's formula -- another float64
algorithm -- shows on the same frames.  The factor covers a different
factorisation, FMA in the butterflies and tree-ordered sums.

Points: a decision ``2 cur < prev`` / ``cur > 2 prev`` can differ from the
reference's only where the ratio cur / prev is within float64 noise of 1/2 or
2.  The tests first assert, from the CPU data alone, that no comparison of
their inputs is within 1e-9 (relative) of either, then require every decision
-- hence the points -- to equal the reference's outright.
"""
import json
from pathlib import Path

import numpy as np
import pytest

import ci_restated

pytestmark = pytest.mark.gpu

GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "cacophony_index.json").read_text())
CASES = GOLDEN["cases"]
FACTOR = 8.0

# the ragged batch: (clip, samples kept); 12289 follows a recording without a
# frame, the long one a recording with a single frame
RAGGED = [("n5121", 5121), ("n4096", 4096), ("n960000", 12289), ("n4097", 4097), ("silence", 336000)]
GAPS = [1, 3, 5, 2, 7]  # samples in front of each recording: no offset is a multiple of 4


@pytest.fixture(scope="module")
def ragged():
    clips = [ci_restated.case_clip(name)[:n] for name, n in RAGGED]
    offsets, parts, pos = [], [], 0
    for x, g in zip(clips, GAPS):
        parts.append(np.full(g, 0.25, np.float32))  # a leak across a boundary would show
        pos += g
        offsets.append(pos)
        parts.append(x)
        pos += len(x)
    assert all(o % 4 for o in offsets)
    ref = [ci_restated.bins(x) for x in clips]
    alt = [ci_restated.bins_makhoul(x) for x in clips]
    return {"clips": clips, "offsets": offsets, "lengths": [len(x) for x in clips],
            "pcm": np.concatenate(parts), "ref": ref, "alt": alt}


def _rel(a, ref):
    live = ref != 0
    return np.abs(a - ref)[live] / ref[live]


def _decisions(b):
    if len(b) < 2:
        return np.zeros((0, 10), bool), np.zeros((0, 10), bool)
    return b[1:] * 2 < b[:-1], b[1:] > b[:-1] * 2


def _run(gpu, pcm, offsets, lengths, want_bins=True):
    import torch
    from aa_amd import cacophony_index as ci
    x = torch.from_numpy(pcm).to(gpu)
    points, bins = ci.run_device(x, offsets, lengths, want_bins=want_bins)
    torch.cuda.synchronize()
    return points.cpu().numpy(), None if bins is None else bins.cpu().numpy()


def _split(points, bins, lengths):
    out, r, p = [], 0, 0
    for n in lengths:
        F = ci_restated.n_frames(n)
        out.append((points[p:p + max(F - 1, 0)], None if bins is None else bins[r:r + F]))
        r += F
        p += max(F - 1, 0)
    assert p == len(points) and (bins is None or r == len(bins))
    return out


def test_bins_of_a_ragged_batch(gpu, ragged):
    points, bins = _run(gpu, ragged["pcm"], ragged["offsets"], ragged["lengths"])
    assert bins.dtype == np.float64 and bins.shape == (sum(map(len, ragged["ref"])), 10)
    ref, alt = np.concatenate(ragged["ref"]), np.concatenate(ragged["alt"])
    silent = ~ref.any(axis=1)
    assert silent.sum() > 90
    assert not bins[silent].any() and not np.signbit(bins[silent]).any()  # exactly +0.0
    assert (bins[~silent] > 0).all()
    bound = FACTOR * _rel(alt, ref).max()
    dev = _rel(bins, ref)
    per_band = [float(_rel(bins[:, b], ref[:, b]).max()) for b in range(10)]
    print(f"band energies: max rel dev GPU {dev.max():.3e}, numpy-FFT Makhoul {bound / FACTOR:.3e}, "
          f"gate {bound:.3e}; per band {['%.1e' % v for v in per_band]}")
    assert bound < 1e-12  # the yardstick itself is float64 noise
    assert dev.max() <= bound
    # the same batch again: bit-equal
    points2, bins2 = _run(gpu, ragged["pcm"], ragged["offsets"], ragged["lengths"])
    assert bins2.tobytes() == bins.tobytes() and points2.tobytes() == points.tobytes()


def test_points_of_a_batch_equal_each_recording_alone(gpu, ragged):
    points, bins = _run(gpu, ragged["pcm"], ragged["offsets"], ragged["lengths"])
    parts = _split(points, bins, ragged["lengths"])
    assert [len(p) for p, _ in parts] == [1, 0, 8, 0, 324]
    for (p, b), x, ref in zip(parts, ragged["clips"], ragged["ref"]):
        assert not ci_restated.near_decisions(ref).any()  # from the CPU data, before the GPU is consulted
        alone_p, alone_b = _run(gpu, x, [0], [len(x)])
        assert alone_p.tolist() == p.tolist()
        assert alone_b.tobytes() == b.tobytes()
        assert p.tolist() == ci_restated.points(ref).tolist()
    # the workspace route (bins_out NULL) gives the same points
    p_ws, none = _run(gpu, ragged["pcm"], ragged["offsets"], ragged["lengths"], want_bins=False)
    assert none is None and p_ws.tolist() == points.tolist()


def test_points_equal_the_reference_for_every_fixture_case(gpu):
    names = sorted(CASES)
    clips = [ci_restated.case_clip(n) for n in names]
    refs = [ci_restated.bins(x) for x in clips]
    near = sum(int(ci_restated.near_decisions(r).sum()) for r in refs)
    assert near == 0  # asserted from the CPU data first: the rule below excuses nothing here
    lengths = [len(x) for x in clips]
    offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]]).tolist()
    points, bins = _run(gpu, np.concatenate(clips), offsets, lengths)
    for name, (p, b), ref in zip(names, _split(points, bins, lengths), refs):
        lo, hi = _decisions(b)
        rlo, rhi = _decisions(ref)
        far = ~ci_restated.near_decisions(ref)
        assert np.array_equal(lo[far], rlo[far]) and np.array_equal(hi[far], rhi[far]), name
        assert p.tolist() == (lo.sum(axis=1) + hi.sum(axis=1)).tolist(), name  # ci_points on its own bins
        assert p.tolist() == CASES[name]["points"], name


def test_points_device_batches_tensors(gpu):
    import torch
    from aa_amd import cacophony_index as ci
    names = ["n4096", "n5121", "n4096", "n336000", "n4096"]  # no frame: first, between and last
    got = ci.points_device([torch.from_numpy(ci_restated.case_clip(n)).to(gpu) for n in names])
    assert [g.tolist() for g in got] == [CASES[n]["points"] for n in names]
    assert ci.points_device([]) == []


def _write_case(tmp_path, name):
    from tools import synth
    p = tmp_path / f"{name}.wav"
    synth.write_wav(p, ci_restated.case_clip(name), sr=16000)
    return p


def test_calculate_and_cli_on_a_16k_wav(gpu, tmp_path, capsys):
    from aa_amd import analyse
    from aa_amd import cacophony_index as ci
    import cacophony_index as shim
    want = CASES["n336000"]["result"]
    wav = _write_case(tmp_path, "n336000")
    got = ci.calculate(str(wav))
    assert json.dumps(got, sort_keys=True) == CASES["n336000"]["result_json"]
    assert shim.calculate is ci.calculate
    capsys.readouterr()
    analyse.main([str(wav), "--old-cacophony-index", "-o"])
    doc = json.loads(capsys.readouterr().out)
    assert isinstance(doc.pop("processing_time_seconds"), float)
    assert doc == want
    assert not wav.with_suffix(".txt").exists()
    analyse.main([str(wav), "--old-cacophony-index"])
    side = json.loads(wav.with_suffix(".txt").read_text())
    res = side["analysis_result"]
    assert isinstance(res.pop("processing_time_seconds"), float)
    assert res == want


def test_short_clip_gives_the_reference_warning(gpu, tmp_path):
    from aa_amd import cacophony_index as ci
    got = ci.calculate(str(_write_case(tmp_path, "n287999")))
    assert json.dumps(got, sort_keys=True) == CASES["n287999"]["result_json"]
    assert got["cacophony_index_old"] == [] and got["ci_warning"] == (
        "Cacophony Index requires at least 20 seconds of audio, but only 17 seconds of audio were provided.")
    tiny = ci.calculate(str(_write_case(tmp_path, "n4096")))
    assert json.dumps(tiny, sort_keys=True) == CASES["n4096"]["result_json"]


def test_48k_recording_resamples_then_scores(gpu, tmp_path):
    """The 720000-sample case at 48 kHz (2,160,000 samples): the device's
    48 -> 16 kHz samples against the resampling oracle, then the pipeline's
    index against the restated index of those very samples."""
    from aa_amd import cacophony_index as ci
    from aa_amd.audio import decode
    from oracle import resample_oracle as ro
    from tools import synth
    x48 = ci_restated.clip(ci_restated.SEEDS["n720000"], 3 * 720000, sr=48000)
    wav = tmp_path / "c48.wav"
    synth.write_wav(wav, x48, sr=48000)
    raw, sr = decode(str(wav))
    assert sr == 48000 and np.array_equal(raw, x48)
    x16 = ci.load_16k_device(str(wav), gpu).cpu().numpy()
    assert x16.dtype == np.float32 and len(x16) == 720000
    err = np.abs(x16 - ro.resample(raw, 48000, 16000)).max()
    print(f"48000 -> 16000: max|d| {err:.2e}")
    assert err <= 1e-5  # tests/test_gpu_resample.py's tolerance
    ref = ci_restated.bins(x16)
    assert not ci_restated.near_decisions(ref).any()
    want = ci.score_table(ci_restated.points(ref), len(x16))
    got = ci.calculate(str(wav))
    assert len(got["cacophony_index_old"]) == 2
    assert json.dumps(got, sort_keys=True) == json.dumps(want, sort_keys=True)
