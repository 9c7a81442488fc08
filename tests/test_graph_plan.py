"""The graph planner on the CPU (aa_graph_plan / aa_graph_node_plan /
aa_graph_plan_layout / aa_graph_node_image, no GPU).

* Every field of the plan -- per node: name, flops, bytes, shape, launch
  variant, tiles, split, fusions, post-fusion inputs / activation, last use,
  workspace offset, byte length + SHA-256 of the four images; per graph: the
  workspace layout and sizes -- equals what the commit named in
  tests/golden/graph_plan_parent.json computed for the same node tables
  (recorded there from its aa_graph_create with the uploads kept on the host,
  the launch variant by its graph_run_node's if-chain), in split-bf16 and f32,
  with and without AA_GRAPH_NOFUSE.  The file keeps a node as its name, its
  launch variant and one digest over all of its fields (graph_tables.
  node_digest), which keeps it a tenth of the size; a node that differs is
  printed in full.  Every rejection returns that commit's code and
  aa_last_error text.
* The allocator's contract is restated independently for every one of these
  plans (equal to the recorded ones by the test above).
* The f32 stem's [C_out / 32][K][32] image and the [C_out][K] transpose are
  restated in numpy from their descriptions, not from the packers.

Not reachable from a node table: "node %d: empty output" (a window's output
is >= 1 once the input covers it, filters / units >= 1 are checked first) and
the launch AA_GK_F32_LDS_3x3x3 (every 3x3 conv over 3 channels that is not an
MFMA conv gets the scalar-path image, so it plans as AA_GK_F32_S).
"""
import ctypes as C
import json
import os
from pathlib import Path

import numpy as np
import pytest

import graph_tables as gt
from aa_amd import _lib

GOLDEN = Path(__file__).resolve().parent / "golden" / "graph_plan_parent.json"
VARIANTS = ["bf16x3_fused", "bf16x3_nofuse", "f32_fused", "f32_nofuse"]
GK = _lib.AA_GK
UNREACHABLE = {"f32_lds_3x3x3"}


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


@pytest.fixture(scope="module")
def tables():
    return gt.tables()


@pytest.fixture(scope="module")
def plans(tables):
    """(case, variant) -> the plan this build makes"""
    before = os.environ.get("AA_GRAPH_NOFUSE")
    out = {}
    try:
        for case in gt.CASES:
            for variant in VARIANTS:
                prec, fuse = variant.split("_")
                if fuse == "nofuse":
                    os.environ["AA_GRAPH_NOFUSE"] = "1"
                else:
                    os.environ.pop("AA_GRAPH_NOFUSE", None)
                out[case, variant] = gt.describe(_lib.lib(), tables[case], prec)
    finally:
        os.environ.pop("AA_GRAPH_NOFUSE", None)
        if before is not None:
            os.environ["AA_GRAPH_NOFUSE"] = before
    return out


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", gt.CASES)
def test_plan_equals_parent(golden, plans, case, variant):
    want = golden["cases"][case][variant]
    got = plans[case, variant]
    assert {k: v for k, v in got.items() if k != "nodes"} == want["head"]
    assert [n["name"] for n in got["nodes"]] == [w[0] for w in want["nodes"]]
    for i, (g, w) in enumerate(zip(got["nodes"], want["nodes"])):
        assert gt.node_digest(g) == w, (i, g)


def test_every_launch_variant_is_recorded(golden, plans):
    seen = {n[1] for vs in golden["cases"].values() for d in vs.values() for n in d["nodes"]}
    assert seen == {v for k, v in GK.items() if k not in UNREACHABLE}
    # both sides of gconv_x3p_fits among the C_out-16 wide kernels
    wide = golden["cases"]["wide_cout16"]["bf16x3_fused"]["nodes"]
    by_kernel = lambda k: {n[0] for n in wide if n[1] == GK[k] and "_1x1_" not in n[0]}
    assert by_kernel("x3p") == {"conv_gx3_3x3_s1_32_16", "conv_gx3_5x3_s1_32_16"}
    assert by_kernel("x3t_256x16") == {"conv_gx3_5x5_s1_32_16", "conv_gx3_4x6_s1_32_16", "conv_gx3_3x7_s1_32_16",
                                       "conv_gx3_1x10_s1_32_16"}
    # the fixtures hold what they are meant to
    fused, plain = plans["effnetv2_c3", "bf16x3_fused"]["nodes"], plans["effnetv2_c3", "bf16x3_nofuse"]["nodes"]
    assert sum(n["skip"] for n in fused) > 10 and not any(n["skip"] or n["nolaunch"] for n in plain)
    assert any(n["scale_src"] >= 0 for n in fused) and any(n["res_src"] >= 0 for n in fused)
    assert gt.EFFNETV2_T == gt.smallest_split_k_T()
    hb = plans["hand_built", "f32_fused"]["nodes"]
    affine = [n["images"] for n in hb if n["name"].startswith("affine_")]
    assert [[im[1][0] > 0, im[2][0] > 0] for im in affine] == [[True, False], [False, True]]
    assert any(n["last_use"] == i for i, n in enumerate(hb[:-1]) if not n["skip"])  # the dangling branch
    assert "dense_720_5" in [n["name"] for n in hb]


def test_allocator_contract(plans):
    """No two buffers that are live at the same time overlap; offsets are
    64-B aligned; the split-K partial sums lie behind every buffer; fused-away
    nodes own no range."""
    for (case, variant), head in plans.items():
        nodes = head["nodes"]
        n = len(nodes)
        size = lambda k: (nodes[k]["H"] * nodes[k]["W"] * nodes[k]["C"] + 15) // 16 * 16
        owners = [i for i in range(n) if not nodes[i]["skip"]]
        for i in range(n):
            readers = [j for j in owners if not nodes[j]["nolaunch"] and i in
                       (nodes[j]["in0"], nodes[j]["in1"], nodes[j]["scale_src"], nodes[j]["res_src"])]
            if nodes[i]["skip"]:
                assert not readers, (case, variant, i)  # nothing reads a buffer that does not exist
                continue
            want_last = n if i == n - 1 else max(readers + [i])
            assert nodes[i]["last_use"] == want_last, (case, variant, i)
            assert nodes[i]["off"] % 16 == 0 and nodes[i]["off"] + size(i) <= head["part_off"], (case, variant, i)
        # a pool written by its depthwise conv is live from that conv's launch
        born = {i: i for i in owners}
        for i in owners:
            if nodes[i]["pool_into"] >= 0:
                born[nodes[i]["pool_into"]] = i
        for a in owners:
            for b in owners:
                if a < b and born[b] <= nodes[a]["last_use"]:
                    lo, hi = nodes[a]["off"], nodes[a]["off"] + size(a)
                    assert nodes[b]["off"] >= hi or nodes[b]["off"] + size(b) <= lo, (case, variant, a, b)
        part = max([nd["split"] * nd["H"] * nd["W"] * nd["C"] for nd in nodes if nd["split"] > 1 and not nd["skip"]],
                   default=0)
        assert head["part_off"] % 64 == 0 and head["per_win"] >= head["part_off"] + part
        assert head["workspace_1"] >= 4 * head["per_win"] and head["workspace_7"] >= 28 * head["per_win"]


@pytest.mark.parametrize("name", sorted(gt.rejections()))
def test_rejection_equals_parent(golden, name):
    table, prec = gt.rejections()[name]
    want = golden["rejections"][name]
    assert want["rc"] != 0
    assert gt.describe(_lib.lib(), table, prec) == want


def test_argument_rejections(golden):
    L = _lib.lib()
    h = C.c_void_p()
    nodes, blob, (H, W, Cin) = gt.hand_built()
    calls = {"null_argument": (None, 0, None, 0, 1, 1, 1, 3),
             "bad_precision": (nodes, len(nodes), blob.ctypes.data, blob.size, H, W, Cin, 1),
             "input_shape": (nodes, len(nodes), blob.ctypes.data, blob.size, H, 0, Cin, 3)}
    for name, args in calls.items():
        rc = L.aa_graph_plan(*args, C.byref(h))
        assert {"rc": rc, "error": L.aa_last_error().decode()} == golden["rejections"][name]
    assert L.aa_graph_plan(nodes, len(nodes), blob.ctypes.data, blob.size, H, W, Cin, 3, None) == _lib.AA_ERR_INVALID
    assert len(golden["rejections"]) == len(gt.rejections()) + 3


def test_planned_graph_refuses_to_run():
    L = _lib.lib()
    nodes, blob, (H, W, Cin) = gt.hand_built()
    h = C.c_void_p()
    assert L.aa_graph_plan(nodes, len(nodes), blob.ctypes.data, blob.size, H, W, Cin, 0, C.byref(h)) == 0
    x = np.zeros(8, np.float32)
    assert L.aa_graph_forward(h, x.ctypes.data, 1, x.ctypes.data, None, x.ctypes.data, 1 << 30, None) == _lib.AA_ERR_INVALID
    assert b"aa_graph_plan" in L.aa_last_error()
    n = C.c_size_t()
    small = np.zeros(8, np.uint8)
    assert L.aa_graph_node_image(h, 1, 1, small.ctypes.data, 8, C.byref(n)) == _lib.AA_ERR_INVALID and n.value == 6 * 4
    assert L.aa_graph_node_image(h, 1, 4, None, 0, C.byref(n)) == _lib.AA_ERR_INVALID
    assert L.aa_graph_node_image(h, len(nodes), 0, None, 0, C.byref(n)) == _lib.AA_ERR_INVALID
    p = _lib.NodePlan()
    assert L.aa_graph_node_plan(h, -1, C.byref(p)) == _lib.AA_ERR_INVALID
    assert L.aa_graph_node_plan(h, 0, None) == _lib.AA_ERR_INVALID
    assert L.aa_graph_plan_layout(h, None) == _lib.AA_ERR_INVALID
    assert L.aa_graph_destroy(h) == 0


# ---- layouts stated independently --------------------------------------------
def test_f32_layouts_from_their_descriptions():
    """A 3x3 conv over 3 channels with 40 outputs in f32: image 0 is the
    kernel as [C_out][K], K = (ky * 3 + kx) * 3 + c (aa_gconv.h gconv_f32);
    image 3 the scalar-path stem [ceil(C_out / 32)][K][32], output o at
    [o / 32][k][o % 32], the channels past C_out zero (gconv_f32_s); image 1
    the bias."""
    t = gt.Tab(61, (8, 9, 3))
    t.conv(-1, 3, 40, k=(3, 3), pad=(1, 1, 1, 1), act="swish")
    nodes, blob, (H, W, Cin) = t.table()
    kern = blob[:27 * 40].reshape(27, 40)
    L = _lib.lib()
    h = C.c_void_p()
    assert L.aa_graph_plan(nodes, 1, blob.ctypes.data, blob.size, H, W, Cin, _lib.AA_PREC_F32, C.byref(h)) == 0
    w, b, b2, ws = (gt.image(L, h, 0, which).view(np.float32) for which in range(4))
    p = _lib.NodePlan()
    assert L.aa_graph_node_plan(h, 0, C.byref(p)) == 0 and p.kernel == GK["f32_s"]
    L.aa_graph_destroy(h)
    assert np.array_equal(w.reshape(40, 27), kern.T)
    assert np.array_equal(b, blob[27 * 40:]) and b2.size == 0
    assert ws.size == 2 * 27 * 32
    want = np.zeros((2, 27, 32), np.float32)
    for o in range(40):
        want[o // 32, :, o % 32] = kern[:, o]
    assert np.array_equal(ws.reshape(2, 27, 32), want)
