"""Every launch variant of the graph route, every output element, against a
float64 reference of that one node.

The other graph tests see these kernels through the logits of whole networks
(a global average pool and a Dense behind every map).  Here each case of
graph_node_cases.CASES is a tiny graph whose output IS the node under test
(the last node may be an [n][H][W][C] map), planned to one named aa_gkernel.
The reference (oracle.graph_node_oracle) computes that node in float64 on its
actual inputs -- producers are read with prefix graphs -- with a derived bound,
the activation taken over the interval's ends, and an element passes iff it is
finite and inside its interval.  The MFMA convs also pass the rms gate against
the CPU emulation of their arithmetic.

Every graph runs three times on one stream with identical buffers (direct
launches, the capture, its replay; bit-equal), its workspace filled with NaN
bytes before each run and its input between NaN guard bands
(graph_tables.forward3_guarded).

No case is skipped and there is no refusal list.  AA_GK_F32_LDS_3x3x3 stays
uncovered: no node table reaches it (test_graph_plan.UNREACHABLE).
"""
import numpy as np
import pytest

import graph_node_cases as gc
import graph_tables as gt
from aa_amd import _lib
from oracle import graph_node_oracle as go

pytestmark = pytest.mark.gpu


def gpu_run(L):
    """evaluate()'s `run` on the GPU: three bit-equal runs, the probabilities gfinal's."""
    def run(tab, prec, x):
        logits, probs, sig = gt.forward3_guarded(L, tab.table(), prec, x)
        for k in (1, 2):
            assert np.array_equal(logits[0], logits[k], equal_nan=True), f"run {k} differs from run 0"
            assert np.array_equal(probs[0], probs[k], equal_nan=True), f"probs of run {k} differ from run 0"
        lg = logits[0]
        if sig:  # 1 / (1 + expf(-v)) on the logits (a non-finite logit fails the caller's check)
            fin = np.isfinite(lg)
            lg64 = lg.astype(np.float64)
            err = np.abs(probs[0].astype(np.float64) - go.logistic64(lg64))
            assert np.all(err[fin] <= go.final_probs_bound(lg64)[fin]), "gfinal's sigmoid"
        else:
            assert np.array_equal(probs[0], lg, equal_nan=True), "probs are the logits without an output sigmoid"
        return lg
    return run


def tile_position(case, plan, idx):
    """Where element idx = (window, y, x, c) sits in its block's tile."""
    if case.kernel not in gc.TILE or case.mode != "node":
        return ""
    w_, y_, x_, c_ = idx
    p, d = plan[case.node], case.tab().nodes[case.node]
    bm, bn = gc.TILE[case.kernel]
    if case.kernel == "x3p":
        return f"; tile row {y_ % gc.PATCH}, column {x_ % gc.PATCH} (16 x 16), c % {bn} = {c_ % bn}"
    pix = y_ * p["W"] + x_
    if (d["kh"], d["kw"], d["sh"], d["sw"], d["pt"], d["pl"]) == (1, 1, 1, 1, 0, 0):
        pix += w_ * p["H"] * p["W"]  # the windows' pixels run flattened
    return f"; pixel % {bm} = {pix % bm} (tile {pix // bm}), c % {bn} = {c_ % bn}"


@pytest.mark.parametrize("case", gc.CASES, ids=lambda c: c.name)
def test_node_against_float64(gpu, case):
    L = _lib.lib()
    e = gc.evaluate(case, L, gpu_run(L))
    chk, plan = e["check"], e["plan"]
    g = e["g"].astype(np.float64)
    lo, hi, r = chk["lo"], chk["hi"], chk["r"]
    assert g.shape == lo.shape, (g.shape, lo.shape)
    # the figure reported: distance from r in half widths (where the f32 ends coincide, in f32 roundings of r)
    half = np.maximum((hi - lo) / 2, go.U24 * np.abs(r) + go.TINY)
    with np.errstate(invalid="ignore"):
        worst = float(np.nanmax(np.abs(g - r) / half)) if np.isfinite(g).any() else float("inf")
    line = f"{case.name} [{case.kernel}{chk['extra']}] max |g - r| / B = {worst:.4f}"
    ratio = None
    if case.kernel in gc.TILE:
        emu = go.mfma_emulation(e["tab"].nodes, e["blob"], plan, case.node, e["bufs"])
        ratio = go.rms_ratio(g, chk, emu)
        line += f", rms ratio against the emulation = {ratio:.3f}"
    print(line)
    n, idx, ex = go.interval_violations(g, lo, hi)
    if n:
        pytest.fail(f"{case.name} [{case.kernel}]: {n} of {g.size} elements outside, worst (window {idx[0]}, y {idx[1]}, "
                    f"x {idx[2]}, c {idx[3]}) g={g[idx]!r} r={r[idx]!r} B={chk['B'][idx]:.3e} interval "
                    f"[{lo[idx]!r}, {hi[idx]!r}] ({ex:.3g} half widths out)" + tile_position(case, plan, idx))
    assert np.all(np.isfinite(g))
    if ratio is not None:
        assert ratio <= go.RMS_MARGIN, (case.name, ratio)


# ---- pairs the sources document as computing identical chains -----------------------------------------
def _conv_tab(in_shape, kernel, bias, k, pad, act, alpha=0.0):
    """A one-conv table with the given [kh][kw][C_in][C_out] kernel."""
    t = gt.Tab(0, in_shape)
    t.chunks += [kernel.ravel().astype(np.float32), bias.astype(np.float32)]
    off = (t.n, t.n + kernel.size)
    t.n += kernel.size + bias.size
    t.node("conv", -1, k=k, pad=pad, filters=kernel.shape[3], act=act, alpha=alpha, off=off)
    return t


@pytest.mark.parametrize("fast, cin, cout", [("f32_lds", 4, 36), ("f32_s", 3, 40), ("f32_lds_3x3x1", 1, 36)])
def test_f32_conv_kernels_are_bit_identical(gpu, fast, cin, cout):
    """gconv_f32_lds / gconv_f32_s document "the same chain as gconv_f32 ... the
    results are identical".  One 3x3 conv two ways: as it is (K <= 96: the staged
    kernel), and over 11 input channels whose extra channels have zero weights
    (K = 99 > GF32_KMAX: gconv_f32).  fma(0, x, acc) == acc for the finite x there,
    so the second chain is the first with no-ops in between."""
    L = _lib.lib()
    rng = np.random.default_rng(cin * 100 + cout)
    H, W, wide = 17, 19, 11
    kern = (rng.standard_normal((3, 3, cin, cout)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
    bias = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    kern_w = np.zeros((3, 3, wide, cout), np.float32)
    kern_w[:, :, :cin] = kern
    x_w = rng.standard_normal((3, H, W, wide)).astype(np.float32)
    x = np.ascontiguousarray(x_w[..., :cin])
    a = _conv_tab((H, W, cin), kern, bias, (3, 3), (1, 1, 1, 1), "leaky", 0.2)
    b = _conv_tab((H, W, wide), kern_w, bias, (3, 3), (1, 1, 1, 1), "leaky", 0.2)
    assert gc.GK_NAME[gc.plan_of(L, a, "bf16x3")["nodes"][0]["kernel"]] == fast
    assert gc.GK_NAME[gc.plan_of(L, b, "bf16x3")["nodes"][0]["kernel"]] == "f32"
    run = gpu_run(L)
    ga, gb = run(a, "bf16x3", x), run(b, "bf16x3", x_w)
    assert np.all(np.isfinite(ga)) and np.array_equal(ga, gb), int((ga != gb).sum())


@pytest.mark.parametrize("case", [c for c in gc.CASES if "gap" in c.fused], ids=lambda c: c.name)
def test_fused_depthwise_pool_equals_the_unfused_pair(gpu, monkeypatch, case):
    """gdwconv_pool* document the map and the pooled vector as equal to gdwconv +
    ggpool* "bit for bit": the same table with and without AA_GRAPH_NOFUSE."""
    L = _lib.lib()
    tab = case.tab()
    x = case.input(tab.in_shape)
    run = gpu_run(L)
    assert gc.GK_NAME[gc.plan_of(L, tab, case.prec)["nodes"][0]["kernel"]] == case.kernel
    fused = run(tab, case.prec, x)
    monkeypatch.setenv("AA_GRAPH_NOFUSE", "1")
    plain_plan = gc.plan_of(L, tab, case.prec)["nodes"]
    assert gc.GK_NAME[plain_plan[0]["kernel"]] in ("dw4", "dw1") and not plain_plan[1]["nolaunch"]
    assert gc.GK_NAME[plain_plan[1]["kernel"]] in ("gpool4", "gpool")
    plain = run(tab, case.prec, x)
    assert np.all(np.isfinite(fused)) and np.array_equal(fused, plain), int((fused != plain).sum())
