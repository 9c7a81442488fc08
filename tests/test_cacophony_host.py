"""The old cacophony index's host side (aa_amd/cacophony_index.py, the aa_ci_*
argument checks) against the reference's recorded results
(tests/golden/cacophony_index.json, made by tests/golden/make_ci_golden.py
from src/cacophony_index.py).  No GPU."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

import ci_restated
from aa_amd import _lib
from aa_amd import cacophony_index as ci

GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "cacophony_index.json").read_text())
CASES = GOLDEN["cases"]


def test_fixture_holds_every_case():
    assert set(CASES) == set(ci_restated.CASES)
    for name, c in CASES.items():
        assert c["n_samples"] == ci_restated.CASES[name]
        assert len(c["points"]) == max(ci_restated.n_frames(c["n_samples"]) - 1, 0)
    assert [len(CASES[n]["result"]["cacophony_index_old"]) for n in
            ("n4096", "n4097", "n5121", "n287999", "n320000", "n336000", "n720000", "n960000")] == \
        [0, 0, 0, 0, 1, 1, 2, 3]
    assert "only 17 seconds" in CASES["n287999"]["result"]["ci_warning"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_score_table_reproduces_the_reference_document(name):
    c = CASES[name]
    got = ci.score_table(np.asarray(c["points"], np.int32), c["n_samples"])
    assert json.dumps(got, sort_keys=True) == c["result_json"]
    assert json.dumps(ci.score_table(list(c["points"]), c["n_samples"]), sort_keys=True) == c["result_json"]


def _reference_table(points):
    """The table by the formulas of the issue, written independently of
    score_table: sorted slice mean, the 202001C curve, q spacing."""
    n = len(points)
    count = (n + 31) // 312
    rows = []
    for e in range(count):
        q = e * (n - 312) // (count - 1) if e else 0
        w = sorted(points[q:q + 312])
        raw = 10 * np.mean(w[int(len(w) * 0.75):int(len(w) * 0.95)])
        s = raw - 10
        rows.append((q, max(100 * s / (s + 18), 0)))
    return rows


@pytest.mark.parametrize("n", [280, 281, 311, 312, 313, 624, 933])
def test_score_table_entry_count_and_spacing(n):
    rng = np.random.default_rng(n)
    pts = [int(v) for v in rng.integers(0, 21, n)]
    doc = ci.score_table(pts, 1024 * (n + 1) + 3072 + 1)
    want = _reference_table(pts)
    table = doc["cacophony_index_old"]
    assert len(table) == len(want) == (n + 31) // 312
    assert len(table) == {280: 0, 281: 1, 311: 1, 312: 1, 313: 1, 624: 2, 933: 3}[n]
    for row, (q, score) in zip(table, want):
        assert row == {"begin_s": round(q * 1024 / 16000), "end_s": round((q + 312) * 1024 / 16000),
                       "index_percent": round(score, 1)}
    assert ("ci_warning" in doc) == (n == 280)
    assert doc["cacophony_index_old_version"] == "2020-01-20_A"


def test_score_table_all_zero_and_all_twenty():
    zero = ci.score_table([0] * 312, 400000)
    assert ci.score_from_points([0] * 312) == 0
    # raw score 0 is below the curve's zero crossing: max(..., 0) keeps the integer 0
    assert json.dumps(zero["cacophony_index_old"]) == '[{"begin_s": 0, "end_s": 20, "index_percent": 0}]'
    full = ci.score_table([20] * 312, 400000)
    assert ci.score_from_points([20] * 312) == 200
    assert full["cacophony_index_old"][0]["index_percent"] == round(100 * 190 / 208, 1) == 91.3


def test_short_clip_warning_wording():
    doc = ci.score_table([], 16000 * 18 - 1)
    assert doc == {"cacophony_index_old": [], "cacophony_index_old_version": "2020-01-20_A",
                   "ci_warning": "Cacophony Index requires at least 20 seconds of audio, "
                                 "but only 17 seconds of audio were provided."}


def test_n_frames_matches_the_reference_range():
    L = _lib.lib()
    for n in list(range(0, 8201)) + [320000, 336000, 720000, 960000]:
        assert L.aa_ci_n_frames(n) == len(range(1024, n - 3072, 1024)) == ci_restated.n_frames(n), n
    assert L.aa_ci_n_frames(320000) == 309 and L.aa_ci_n_frames(960000) == 934


def test_edges_and_window_are_numpys():
    assert ci.band_edges().tolist() == GOLDEN["edges"] == ci_restated.edges().tolist()
    assert GOLDEN["edges"] == [25, 38, 60, 93, 145, 226, 351, 546, 848, 1318, 2048]
    assert np.array_equal(ci.window(), np.hanning(2048))


def test_plan_rejects_bad_edges_without_a_gpu():
    ok = ci.Plan(host_only=True)
    ok.close()
    e = ci.band_edges().astype(np.int32)
    down = e.copy()
    down[4] = down[3] - 1
    with pytest.raises(_lib.AAError, match="edges decrease at 4"):
        ci.Plan(edges=down, host_only=True)
    high = e.copy()
    high[10] = 2049
    with pytest.raises(_lib.AAError, match="edge 10 is 2049"):
        ci.Plan(edges=high, host_only=True)
    neg = e.copy()
    neg[0] = -1
    with pytest.raises(_lib.AAError, match="edge 0 is -1"):
        ci.Plan(edges=neg, host_only=True)
    # aa_ci_create makes the same checks before it touches the device
    h = C.c_void_p()
    w = ci.window()
    assert _lib.lib().aa_ci_create(w.ctypes.data, high.ctypes.data, C.byref(h)) == _lib.AA_ERR_INVALID
    assert b"edge 10" in _lib.lib().aa_last_error()
    assert _lib.lib().aa_ci_create(None, e.ctypes.data, C.byref(h)) == _lib.AA_ERR_INVALID
    bad = w.copy()
    bad[7] = np.nan
    with pytest.raises(_lib.AAError, match=r"window\[7\]"):
        ci.Plan(win=bad, host_only=True)


def test_run_rejects_bad_arguments_before_any_hip_call():
    L = _lib.lib()
    plan = ci.Plan(host_only=True)
    off = (C.c_int64 * 2)(0, 336000)
    ln = (C.c_int64 * 2)(336000, 5121)
    need = L.aa_ci_workspace_bytes(ln, 2)
    assert need == (325 + 2) * 10 * 8
    assert L.aa_ci_workspace_bytes(ln, 0) == 0 and L.aa_ci_workspace_bytes(None, 2) == 0
    fake = C.c_void_p(4096)  # never dereferenced: every call below fails before a launch
    assert L.aa_ci_run(None, fake, off, ln, 2, fake, need, None, fake, None) == _lib.AA_ERR_INVALID
    assert L.aa_ci_run(plan._h, None, off, ln, 2, fake, need, None, fake, None) == _lib.AA_ERR_INVALID
    assert L.aa_ci_run(plan._h, fake, None, ln, 2, fake, need, None, fake, None) == _lib.AA_ERR_INVALID
    assert L.aa_ci_run(plan._h, fake, off, None, 2, fake, need, None, fake, None) == _lib.AA_ERR_INVALID
    assert L.aa_ci_run(plan._h, fake, off, ln, 2, fake, need, None, None, None) == _lib.AA_ERR_INVALID
    assert b"null argument" in L.aa_last_error()
    assert L.aa_ci_run(plan._h, fake, off, ln, 65, fake, need, None, fake, None) == _lib.AA_ERR_INVALID
    assert L.aa_ci_run(plan._h, fake, off, ln, 2, fake, need - 1, None, fake, None) == _lib.AA_ERR_WORKSPACE
    assert b"workspace" in L.aa_last_error()
    assert L.aa_ci_run(plan._h, fake, off, ln, 2, None, need, None, fake, None) == _lib.AA_ERR_WORKSPACE
    neg = (C.c_int64 * 2)(-4, 336000)
    assert L.aa_ci_run(plan._h, fake, neg, ln, 2, fake, need, None, fake, None) == _lib.AA_ERR_INVALID
    # a host-only plan cannot launch, and says so after the argument checks
    assert L.aa_ci_run(plan._h, fake, off, ln, 2, fake, need, None, fake, None) == _lib.AA_ERR_INVALID
    assert b"aa_ci_plan" in L.aa_last_error()
    plan.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_restated_algorithm_reproduces_the_reference(name):
    """tests/ci_restated.py is what the GPU tests compare with: its points
    equal the reference's, its band energies the reference's bit for bit."""
    c = CASES[name]
    x = ci_restated.case_clip(name)
    b = ci_restated.bins(x)
    assert b.shape == (ci_restated.n_frames(len(x)), 10)
    assert ci_restated.points(b).tolist() == c["points"]
    assert [[float(v).hex() for v in row] for row in b[:8]] == c["bins_first8"]
    if name == "silence" and len(b):
        f0, f1 = -(-(len(x) // 3) // 1024), (2 * len(x) // 3 - 2048) // 1024 - 1
        assert f1 - f0 > 90 and not b[f0:f1].any() and b[:f0 - 2].all()
    assert not ci_restated.near_decisions(b).any()
    if len(b):
        dev = np.abs(ci_restated.bins_makhoul(x) - b) / np.where(b == 0, 1.0, b)
        assert dev.max() < 1e-13
