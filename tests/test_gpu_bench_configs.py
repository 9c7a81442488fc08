"""The bench's non-default configurations run end to end on the GPU and
print one contract-shaped JSON line (BASELINE configs[2] stream: --config 3;
configs[3] corpus of WAV files through the analyse path: --config 4;
configs[4] fp16 log-mel + fp8: --precision fp8 --logmel f16)."""
import json
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def _bench(*args):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), *args], capture_output=True, text=True, timeout=240,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "ms_per_step", "config", "dtype"):
        assert k in line
    assert line["value"] > 0
    return line


def test_bench_config4_corpus(gpu):
    line = _bench("--config", "4", "--files", "3")
    assert line["config"]["documents_gathered"] == 3


def test_bench_config3_stream(gpu):
    line = _bench("--config", "3", "--clips", "24")
    assert line["config"]["records_gathered"] == 24


def test_bench_configs4_fp16_logmel_fp8(gpu):
    line = _bench("--full", "--precision", "fp8", "--logmel", "f16", "--steps", "5", "--warmup", "2", "--secondary=",
                  "--cpu-seconds", "0")
    assert line["dtype"] == "fp8 (fp16 log-mel)"
    assert "roofline" in line and line["roofline"]["achieved"] > 0


@pytest.mark.parametrize("pipeline", ["0", "1", "2"])
def test_bench_step_modes_hold_the_gate(gpu, pipeline):
    """The headline step back to back (0), with the next batch's front end
    overlapped (1) and with two batches in flight on two streams (2, the
    default): each asserts the 1e-3 logit gate on its own 64 windows (a step
    on clip pair 0 after the timed loop, against the CPU oracle)."""
    line = _bench("--full", "--pipeline", pipeline, "--steps", "6", "--warmup", "2", "--secondary=",
                  "--cpu-seconds", "0")
    assert line["parity_gate"]["pass"]
    assert line["max_abs_dlogit"]["bf16x3"] <= 1e-3
    assert line["steps"] == 6


def test_bench_plain_run_is_lean_and_dumps_outputs(gpu, tmp_path):
    """A plain run times its steps and prints the line, nothing else; with
    --dump-outputs it writes what the last timed step computed as float32
    arrays: the step's 64 log-mels, logits, probabilities and the two track
    means -- the mean of the 39 and of the 25 windows' probabilities."""
    import numpy as np
    line = _bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "dump"))
    assert line["steps"] == 3 and line["warmup"] == 1
    assert line["higher_is_better"] is True and line["unit"] == "audio-s/s" and line["dtype"] == "bf16x3"
    assert line["ms_per_step"] > 0
    # value = 3 steps x 64 windows x 60/39 audio-s over the timed 3 x ms_per_step
    assert line["value"] == pytest.approx(64 * 60.0 / 39 / (line["ms_per_step"] * 1e-3), rel=1e-3)
    for k in ("roofline", "secondary", "cpu_baseline", "parity_gate", "max_abs_dlogit", "full_record"):
        assert k not in line, k
    arrays = {p.stem: np.load(p) for p in (tmp_path / "dump").glob("*.npy")}
    assert set(arrays) == {"logmel", "logits", "probs", "track_mean"}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 10 ** 6
    n_labels = arrays["logits"].shape[1]
    assert arrays["logmel"].shape[:2] == (64, 160)
    assert arrays["logits"].shape == arrays["probs"].shape == (64, n_labels)
    assert arrays["track_mean"].shape == (2, n_labels)
    assert arrays["logits"].std() > 0
    # a float32 sum of n <= 39 values in [0, 1] rounds n - 1 times, each by <= 2^-24 of a partial sum <= n:
    # the mean is within 38 x 2^-24 = 2.3e-6 of the exact one, whatever the order of summation
    ref = np.stack([arrays["probs"][:39].astype(np.float64).mean(0), arrays["probs"][39:].astype(np.float64).mean(0)])
    assert np.abs(arrays["track_mean"] - ref).max() <= 2.5e-6
