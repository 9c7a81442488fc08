"""aa_graph_forward computes, bit for bit, the logits that the commit named
in tests/golden/graph_plan_parent.json computed on an MI355X for the node
tables of tests/graph_tables.py (tests/golden/graph_pin_parent.npz: 3 windows
of pin_input, split-bf16 and f32, with and without AA_GRAPH_NOFUSE): by direct
launches, by the capture launched on the second call with the same buffers,
and by its replay on the third."""
from pathlib import Path

import numpy as np
import pytest

import graph_tables as gt
from aa_amd import _lib

pytestmark = pytest.mark.gpu

PIN = Path(__file__).resolve().parent / "golden" / "graph_pin_parent.npz"


@pytest.fixture(scope="module")
def pinned():
    with np.load(PIN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def tables():
    return gt.tables()


@pytest.mark.parametrize("variant", ["bf16x3_fused", "bf16x3_nofuse", "f32_fused", "f32_nofuse"])
@pytest.mark.parametrize("case", gt.CASES)
def test_logits_equal_parent_bitwise(gpu, pinned, tables, monkeypatch, case, variant):
    prec, fuse = variant.split("_")
    if fuse == "nofuse":
        monkeypatch.setenv("AA_GRAPH_NOFUSE", "1")
    else:
        monkeypatch.delenv("AA_GRAPH_NOFUSE", raising=False)
    want = pinned[f"{case}:{variant}"]
    assert want.shape[0] == 3 and np.isfinite(want).all()
    runs = gt.forward3(_lib.lib(), tables[case], prec, gt.pin_input(case, tables[case]))
    for how, got in zip(("direct", "captured", "replayed"), runs):
        assert got.shape == want.shape, how
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (how, np.abs(got - want).max())
