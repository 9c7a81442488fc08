"""The per-node checks of the graph kernels on the CPU: the case
table plans as intended, hits the edges it is meant to hit, and the interval
rule of oracle.graph_node_oracle accepts correct arithmetic and rejects
planted defects.  (The GPU side is test_gpu_graph_nodes.py.)

* Every case of graph_node_cases.CASES plans to its named launch variant with
  its named fusions; the variants covered are AA_GK minus
  test_graph_plan.UNREACHABLE (AA_GK_F32_LDS_3x3x3: no node table reaches it).
* Edges, from the plan and the tile sizes restated here from run_conv_mfma.
* A CPU emulation of the MFMA convs' arithmetic (bf16 hi + lo, hi.hi + lo.hi +
  hi.lo, float32 accumulation) lies inside the interval on every MFMA case.
* The emulation with one defect each is rejected.  Gate per defect, measured
  over the cases it applies to (the assertion is that one of the two gates
  rejects it in every such case):
    (a) lo.hi term dropped ......................... rms gate (~2^-10 A /
        sqrt(K) per element, close to B; on these cases the largest of a
        few thousand elements also leaves the interval, in all 30)
    (b) padding column read from the clamped pixel . interval
    (c) last channel quad of a partial chunk dropped  interval
    (d) SE scale of window w - 1 ................... interval
    (e) a wrong channel's bias on the last channel . interval
    (f) one split-K slice left out ................. interval
    (g) swish as relu at one element ............... interval
  No listed defect escapes both gates.
* Unit checks of the activation intervals and of the fast logistic's slack.
"""
import numpy as np
import pytest

import graph_node_cases as gc
from aa_amd import _lib
from oracle import graph_node_oracle as go
from test_graph_plan import UNREACHABLE

GK = _lib.AA_GK
MFMA_CASES = [c for c in gc.CASES if c.kernel in gc.TILE]


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


@pytest.fixture(scope="module")
def planned(L):
    """case name -> (tab, plan nodes)"""
    out = {}
    for c in gc.CASES:
        tab = c.tab()
        out[c.name] = (tab, gc.plan_of(L, tab, c.prec)["nodes"])
    return out


@pytest.fixture(scope="module")
def mfma(L, planned):
    """MFMA case name -> dict(tab, plan, blob, bufs (CPU stand-ins), check, emu)"""
    out = {}
    for c in MFMA_CASES:
        tab, plan = planned[c.name]
        blob = tab.table()[1]
        bufs = go.cpu_buffers(tab.nodes, blob, plan, c.input(tab.in_shape))
        chk = go.node_check(tab.nodes, blob, plan, c.node, bufs)
        emu = go.mfma_emulation(tab.nodes, blob, plan, c.node, bufs)
        out[c.name] = dict(tab=tab, plan=plan, blob=blob, bufs=bufs, check=chk, emu=emu)
    return out


# ---- plans -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", gc.CASES, ids=lambda c: c.name)
def test_case_plans_to_its_variant(planned, case):
    tab, plan = planned[case.name]
    launch = 0 if case.mode == "pooled" else case.node
    p = plan[launch]
    assert gc.GK_NAME[p["kernel"]] == case.kernel
    assert not p["skip"] and not p["nolaunch"]
    assert (p["scale_src"] >= 0) == ("se" in case.fused)
    assert (p["res_src"] >= 0) == ("res" in case.fused)
    assert (p["pool_into"] >= 0) == ("gap" in case.fused)
    if "gap" in case.fused:
        assert plan[1]["nolaunch"] and p["pool_into"] == 1
    # what the reference takes from the plan (activation, slope, sources) is what the table says:
    # the node's own where nothing is fused into it, the Multiply's and the Add's where they are
    d = tab.nodes[launch]
    if case.fused and case.mode == "node":
        mul, add = tab.nodes[4], tab.nodes[6]
        assert plan[4]["skip"] and plan[6]["skip"]  # the Multiply and the Add launch nothing
        assert (mul["in0"], mul["in1"], add["in0"], add["in1"]) == (-1, 3, launch, 0)
        assert (p["in0"], p["scale_src"], p["res_src"]) == (mul["in0"], mul["in1"], add["in1"])
        assert d["act"] == 0 and (p["act"], p["alpha"]) == (add["act"], np.float32(add["alpha"]))
        assert plan[7]["in0"] == launch  # the copy reads the conv
    else:
        assert (p["in0"], p["in1"]) == (d["in0"], d["in1"])
        assert (p["act"], p["alpha"]) == (d["act"], np.float32(d["alpha"]))
    for q, dq in zip(plan, tab.nodes):  # every other launched node, the producers among them
        if not q["skip"] and q is not p:
            assert (q["act"], q["alpha"]) == (dq["act"], np.float32(dq["alpha"]))
    assert len(tab.nodes) <= 8
    assert max(pl["H"] * pl["W"] for pl in plan) <= 4096 and tab.in_shape[0] * tab.in_shape[1] <= 4096


def test_every_reachable_variant_has_a_case():
    assert {c.kernel for c in gc.CASES} == set(GK) - UNREACHABLE
    assert any(c.n == 1 for c in MFMA_CASES) and all(c.n in (1, 3) for c in gc.CASES)


def test_activations_are_spread(planned):
    """none / relu / leaky / sigmoid / swish each met by an MFMA conv, an f32 conv, a
    depthwise conv and gsplit_reduce; the sigmoids among them are glogistic's (the
    node is not the output node)."""
    groups = {"mfma": set(gc.TILE), "f32": {"f32_s", "f32_lds_3x3x1", "f32_lds", "f32"},
              "dw": {"dw4", "dw1", "dwpool4_s1", "dwpool4_s2", "dwpool4_k3", "dwpool4", "dwpool"},
              "split": {"x3t_split_kc2", "x3t_split_kc1"}}
    for g, kernels in groups.items():
        seen = set()
        for c in gc.CASES:
            if c.kernel in kernels:
                tab, plan = planned[c.name]
                launch = 0 if c.mode == "pooled" else c.node
                act = go.ACTS[plan[launch]["act"]]
                assert act != "sigmoid" or launch != len(plan) - 1
                seen.add(act)
        assert seen == {None, "relu", "leaky", "sigmoid", "swish"}, (g, seen)


# ---- edges ---------------------------------------------------------------------------------------
def _is_pointwise(d):
    return (d["kh"], d["kw"], d["sh"], d["sw"], d["pt"], d["pl"]) == (1, 1, 1, 1, 0, 0)


@pytest.mark.parametrize("variant", gc.MFMA)
def test_mfma_edges(planned, variant):
    bm, bn = gc.TILE[variant]
    cases = [c for c in MFMA_CASES if c.kernel == variant]
    partial = pw_straddle = pad_c4 = odd_c = big_grid = False
    for c in cases:
        tab, plan = planned[c.name]
        p, d = plan[c.node], tab.nodes[c.node]
        assert p["bn"] == min(bn, 64) and p["cout_pad"] % bn == 0
        hw = p["H"] * p["W"]
        if variant == "x3p":
            partial |= p["H"] % gc.PATCH != 0 and p["W"] % gc.PATCH != 0   # partial in both directions
        else:
            pix = hw * c.n if _is_pointwise(d) else hw
            partial |= pix % bm != 0
            pw_straddle |= _is_pointwise(d) and c.n > 1 and hw % bm != 0 and bm % hw != 0
        pad_c4 |= p["C"] % 4 == 0 and p["cout_pad"] - p["C"] > 0
        odd_c |= p["C"] % 4 != 0
        grid = gc.launch_grid(p, d, c.n)
        blocks = grid[0] * grid[1] * grid[2]
        big_grid |= blocks >= 9 and blocks % 8 != 0   # xcd_order's remapped range and its tail
        if variant.startswith("x3t_split"):
            assert hw <= 128 and p["split"] > 1 and p["split"] * p["cslice"] * 32 == p["cin_pad"]
    assert partial and pad_c4 and odd_c and big_grid
    assert pw_straddle or variant == "x3p"


@pytest.mark.parametrize("template", ["gconv_x3t", "gconv_x3p"])
def test_mfma_input_channel_paths(planned, template):
    """C_in % 32 == 0, C_in % 8 == 0 with a partial chunk, C_in % 8 != 0 (scalar gather)."""
    cins = {planned[c.name][0].in_shape[2] for c in MFMA_CASES   # (unfused: the conv reads the graph input)
            if (c.kernel == "x3p") == (template == "gconv_x3p") and not c.fused}
    assert any(ci % 32 == 0 for ci in cins)
    assert any(ci % 8 == 0 and ci % 32 != 0 for ci in cins)
    assert any(ci % 8 != 0 for ci in cins)


def test_f32_and_depthwise_edges(planned):
    for kernel, cpb in (("f32_s", 32), ("f32_lds_3x3x1", 32), ("f32_lds", 32), ("f32", 8)):
        ps = [planned[c.name][1][c.node] for c in gc.CASES if c.kernel == kernel]
        assert any(p["C"] % cpb != 0 for p in ps), kernel
        assert any(p["H"] * p["W"] > 256 for p in ps), kernel   # more than one block of pixels
        if cpb == 32:  # float4 stores (a whole block of 32 channels, C_out % 4 == 0) and scalar ones
            assert any(p["C"] % 4 == 0 and p["C"] >= 32 for p in ps), kernel
            assert any(p["C"] % 4 != 0 or p["C"] % 32 != 0 for p in ps), kernel
    for kernel, cpb, stripes in (("dwpool4_s1", 32, 32), ("dwpool4_s2", 32, 32), ("dwpool4_k3", 32, 32),
                                 ("dwpool4", 32, 32), ("dwpool", 64, 16)):
        ps = [planned[c.name][1][0] for c in gc.CASES if c.kernel == kernel]
        assert {c.mode for c in gc.CASES if c.kernel == kernel} == {"map_x_pool", "pooled"}
        assert all(p["C"] % cpb != 0 and (p["H"] * p["W"]) % stripes != 0 for p in ps), kernel
    for kernel, stripes in (("gpool4", 32), ("gpool", 16)):
        hws = {planned[c.name][0].in_shape[0] * planned[c.name][0].in_shape[1] for c in gc.CASES if c.kernel == kernel}
        assert any(hw < stripes for hw in hws) and 32 in hws and any(hw > stripes and hw % stripes for hw in hws)


# ---- the harness on a stand-in for the GPU ----------------------------------------------------------
def test_reference_rounded_to_f32_passes_every_case(L):
    """evaluate() end to end with the float64 results rounded to f32 in the GPU's
    place: prefix graphs plan their producers on the same variant, shapes agree and
    the reference lies in its own interval."""
    run = gc.cpu_run(L)
    for c in gc.CASES:
        e = gc.evaluate(c, L, run)
        n, idx, ex = go.interval_violations(e["g"], e["check"]["lo"], e["check"]["hi"])
        assert n == 0, (c.name, n, idx, ex)


# ---- the emulation inside its bound; the defects outside ------------------------------------------
@pytest.mark.parametrize("case", MFMA_CASES, ids=lambda c: c.name)
def test_emulation_is_inside_the_interval(mfma, case):
    m = mfma[case.name]
    chk, emu = m["check"], m["emu"]
    n, idx, ex = go.interval_violations(emu, chk["lo"], chk["hi"])
    assert n == 0, (case.name, n, idx, ex)
    pre = go.mfma_emulation(m["tab"].nodes, m["blob"], [dict(p, act=0) for p in m["plan"]], case.node, m["bufs"])
    ratio = float((np.abs(pre - chk["y"]) / chk["B"]).max())
    print(f"{case.name}: emulation max |e - y| / B = {ratio:.3f}, rms (e - r) / A = "
          f"{np.sqrt(np.mean(((emu - chk['r']) / np.maximum(chk['A'], go.TINY)) ** 2)):.3e}")
    assert ratio <= 1.0


@pytest.mark.parametrize("defect", go.DEFECTS)
def test_defect_is_rejected(mfma, defect):
    applies, by_interval, by_rms = 0, 0, 0
    for c in MFMA_CASES:
        m = mfma[c.name]
        bad = go.mfma_emulation(m["tab"].nodes, m["blob"], m["plan"], c.node, m["bufs"], defect=defect)
        if bad is None:
            continue
        applies += 1
        n, idx, ex = go.interval_violations(bad, m["check"]["lo"], m["check"]["hi"])
        ratio = go.rms_ratio(bad, m["check"], m["emu"])
        by_interval += n > 0
        by_rms += ratio > go.RMS_MARGIN
        assert n > 0 or ratio > go.RMS_MARGIN, (defect, c.name, "escapes both gates", ratio)
    print(f"{defect}: {applies} cases, interval rejects {by_interval}, rms gate rejects {by_rms}")
    assert applies >= 2
    # (a) is ~2^-10 A / sqrt(K) per element, close to B: the interval catches it only through the
    # largest of many elements, so the rms gate is the one required to hold it
    assert (by_rms if defect == "lohi" else by_interval) == applies, defect


# ---- the interval code itself ---------------------------------------------------------------------
def test_swish_interval_contains_its_minimum():
    vmin = go.SWISH_MIN_V
    smin = float(go.act64(vmin, "swish"))
    assert abs(smin + 0.27846454276107) < 1e-12
    v = np.linspace(vmin - 1e-3, vmin + 1e-3, 2001)
    assert smin <= go.act64(v, "swish").min() + 1e-15   # it is the minimum
    lo, hi = go.act_interval(np.array([-1.4]), np.array([-1.1]), "swish")
    assert lo[0] <= smin < min(go.act64(-1.4, "swish"), go.act64(-1.1, "swish"))
    assert hi[0] >= max(go.act64(-1.4, "swish"), go.act64(-1.1, "swish"))
    # not containing it: the ends (decreasing left of the minimum, increasing right of it)
    lo, hi = go.act_interval(np.array([-3.0, 0.5]), np.array([-2.0, 0.6]), "swish")
    for k, (a, b) in enumerate(((-3.0, -2.0), (0.5, 0.6))):
        ends = sorted((float(go.act64(a, "swish")), float(go.act64(b, "swish"))))
        assert lo[k] <= ends[0] and hi[k] >= ends[1] and hi[k] - lo[k] < (ends[1] - ends[0]) + 1e-6


def test_sigmoid_interval_far_out():
    lo, hi = go.act_interval(np.array([-100.0, 100.0]), np.array([-100.0, 100.0]), "sigmoid")
    assert lo[0] <= 0.0 <= hi[0] and hi[0] <= 2.0 ** -125      # rcp(inf) = 0 is inside; nothing larger is
    assert lo[1] <= 1.0 <= hi[1] and lo[1] >= 1.0 - 2.0 ** -21
    assert np.all(np.isfinite([lo, hi]))
    assert go.gact_f32(np.float32(-100), "sigmoid") == 0.0 and go.gact_f32(np.float32(100), "sigmoid") == 1.0


def test_leaky_slopes_zero_and_one():
    v = np.array([-2.5, -1e-3, 0.0, 3.0])
    lo0, hi0 = go.act_interval(v - 0.1, v + 0.1, "leaky", 0.0)
    rl, rh = go.act_interval(v - 0.1, v + 0.1, "relu")
    assert np.array_equal(lo0, rl) and np.array_equal(hi0, rh)
    lo1, hi1 = go.act_interval(v - 0.1, v + 0.1, "leaky", 1.0)
    nl, nh = go.act_interval(v - 0.1, v + 0.1, None)
    assert np.array_equal(lo1, nl) and np.array_equal(hi1, nh)
    with pytest.raises(AssertionError):
        go.act_interval(v, v, "leaky", 1.5)


def test_logistic_slack_covers_the_four_roundings():
    """glogistic's chain in f32 with exp2 and rcp correctly rounded, and with each
    moved by one ulp either way (what "within 1 ulp" allows), stays within
    logistic_slack of the float64 logistic; the slack is no more than 21 ulp of the
    result where the argument is moderate (|v| <= 8)."""
    rng = np.random.default_rng(7)
    v = np.concatenate([np.linspace(-100, 100, 4001), rng.standard_normal(4000) * 4, [-87.5, -88.8, 88.8, 0.0]])
    v = v.astype(np.float32)
    want = go.logistic64(v.astype(np.float64))
    slack = go.logistic_slack(v)
    t = v * np.float32(-1.44269504088896341)
    with np.errstate(over="ignore", divide="ignore"):
        e0 = np.exp2(t.astype(np.float64)).astype(np.float32)
        for de in (-1, 0, 1):
            e = e0 if de == 0 else np.nextafter(e0, np.float32(np.inf * de))
            e = np.where(np.isfinite(e0), e, e0)
            d = np.float32(1) + e
            s0 = (1.0 / d.astype(np.float64)).astype(np.float32)
            for ds in (-1, 0, 1):
                s = s0 if ds == 0 else np.nextafter(s0, np.float32(np.inf * ds))
                err = np.abs(s.astype(np.float64) - want)
                assert np.all(err <= slack), (de, ds, float(v[np.argmax(err - slack)]))
    # and it is no blank cheque: at most (5 + 2 |v|) U24 s, i.e. 21 ulp of the result for |v| <= 8
    # (ulp(s) >= U24 s), 5 ulp-halves where 1 - s is small
    mod = np.abs(v) <= 8
    assert np.all(slack[mod] <= 21 * np.spacing(want[mod].astype(np.float32)).astype(np.float64) + go.TINY)
    assert np.all(slack[v >= 8] <= 3.01 * go.U24)
    # swish: the product's rounding on top
    sw = go.gact_f32(v, "swish").astype(np.float64)
    assert np.all(np.abs(sw - go.act64(v.astype(np.float64), "swish")) <= go.act_slack(v, "swish"))
