"""Generate tests/golden/cacophony_index.json by importing the REFERENCE's
cacophony_index (read-only, from /root/reference/src) and running its
``calculate`` on the tests' seeded clips.

Run in the build container (the GPU box has no /root/reference):

    python tests/golden/make_ci_golden.py

``common.load_audio_file_as_numpy_array`` (ffmpeg) is replaced by a function
that returns the seeded float32 clip (tests/ci_restated.py ``case_clip``); the
reference's own ``get_ci_bins`` is wrapped to record what it returns.  Per
case the fixture holds the reference's result document, its points, and the
float64 band energies of the first 8 frames as ``float.hex``; plus the band
edges the reference computes.  No samples and none of the reference's text
are stored.
"""
from __future__ import annotations

import json
import math
import sys
from pathlib import Path

import numpy as np

REF = Path("/root/reference/src")
OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT.parent))
sys.dont_write_bytecode = True

import ci_restated  # noqa: E402


def main():
    sys.path.insert(0, str(REF))
    import scipy.fftpack  # noqa: F401  (the reference reaches it through scipy.signal)
    import common
    import cacophony_index as ref

    common.check_python_version = lambda: None
    cases = {}
    for name, n in ci_restated.CASES.items():
        x = ci_restated.case_clip(name)
        assert x.dtype == np.float32 and len(x) == n
        common.load_audio_file_as_numpy_array = lambda path, sr, x=x: x
        seen = []
        inner = ref.get_ci_bins

        def recording(source_trim, sample_rate, inner=inner, seen=seen):
            b = inner(source_trim, sample_rate)
            seen.append(b)
            return b

        ref.get_ci_bins = recording
        try:
            result = ref.calculate(name + ".wav")
        finally:
            ref.get_ci_bins = inner
        pts = []
        for prev, cur in zip(seen, seen[1:]):
            pts.append(int(sum(cur * 2 < prev) + sum(cur > prev * 2)))
        cases[name] = {
            "n_samples": n,
            "seed": ci_restated.SEEDS[name],
            "result": json.loads(json.dumps(result)),
            "result_json": json.dumps(result, sort_keys=True),
            "points": pts,
            "bins_first8": [[float(v).hex() for v in b] for b in seen[:8]],
        }
    cut = 100 * 2 * 2048 // 16000
    edges = np.logspace(math.log10(cut), math.log10(2048), num=11, dtype=int)
    doc = {"edges": [int(e) for e in edges], "cases": cases}
    (OUT / "cacophony_index.json").write_text(json.dumps(doc, indent=1, sort_keys=True) + "\n")
    for name, c in cases.items():
        print(name, len(c["points"]), c["result_json"][:100])


if __name__ == "__main__":
    main()
