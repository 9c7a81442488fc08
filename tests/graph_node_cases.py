"""The case table of the per-node checks of the graph kernels: one
entry per launch variant (aa_gkernel) and edge, for test_graph_node_cases.py
(CPU: plans, edges, the rule's teeth) and test_gpu_graph_nodes.py (GPU: every
output element against oracle.graph_node_oracle).

A case is a tiny hand-built node table (graph_tables.Tab) whose output is the
node under test -- the last node, or an identity affine (a copy) behind it where
the planner must be allowed to fuse into it or where its sigmoid is to be the
kernels' own (the output node's is gfinal's).  `evaluate` runs a case through a
`run(table, precision, x) -> [n, L] float32` callable: it reads every producer
the node under test depends on with a prefix graph (the table cut after the
producer plus an identity affine, the producer on the same launch variant in
both plans), and returns the oracle's check next to the node's output.

AA_GK_F32_LDS_3x3x3 has no case: no node table reaches it
(test_graph_plan.UNREACHABLE).
"""
import zlib
from dataclasses import dataclass

import numpy as np

import graph_tables as gt
from oracle import graph_node_oracle as go

GK = gt._lib.AA_GK
GK_NAME = {v: k for k, v in GK.items()}
SAME_FIELDS = ("kernel", "bn", "cout_pad", "cin_pad", "split", "cslice", "skip", "nolaunch", "scale_src", "res_src",
               "pool_into", "in0", "in1", "act", "alpha", "H", "W", "C")

# pixel tile (BM) and channel tile (BN) of the MFMA variants (run_conv_mfma's template arguments)
TILE = {"x3p": (256, 16), "x3t_256x16": (256, 16), "x3t_128x32": (128, 32), "x3t_64x128": (64, 128),
        "x3t_split_kc2": (64, 64), "x3t_split_kc1": (64, 64), "x3t_64x64_kc2": (64, 64), "x3t_64x64_pd2": (64, 64),
        "x3t_64x64": (64, 64)}
MFMA = list(TILE)
PATCH = 16  # gconv_x3p's 16 x 16 output tile


@dataclass
class Case:
    name: str
    build: object            # () -> gt.Tab
    node: int                # the node under test
    kernel: str              # the aa_gkernel it must plan to
    prec: str = "bf16x3"
    n: int = 3
    mode: str = "node"       # "node"; "map_x_pool": dw -> gavgpool -> mul(dw, pool), the map through the product;
                             # "pooled": dw -> gavgpool -> copy, the vector the depthwise launch writes
    fused: tuple = ()        # of "se", "res", "gap": what graph_fuse must have put into the node
    positive: bool = False   # inputs in [0.1, 2] (pow)

    def tab(self):
        return self.build()

    def input(self, in_shape):
        rng = np.random.default_rng(zlib.crc32(self.name.encode()))
        shape = (self.n,) + tuple(in_shape)
        if self.positive:
            return rng.uniform(0.1, 2.0, shape).astype(np.float32)
        return rng.standard_normal(shape).astype(np.float32)


def _seed(name):
    return zlib.crc32(name.encode()) % (1 << 31)


def _set_act(t, i, act, alpha=0.2):
    t.nodes[i]["act"] = gt.ACT[act]
    if act == "leaky":
        t.nodes[i]["alpha"] = alpha


def _close(t, i, act):
    """An identity affine behind node i where the kernels' own sigmoid is wanted."""
    if act == "sigmoid":
        t.node("affine", i)


SAME = {(3, 3): (1, 1, 1, 1), (5, 3): (2, 2, 1, 1), (5, 5): (2, 2, 2, 2), (1, 1): (0, 0, 0, 0)}
CASES = []


def conv_case(kernel, hw, cin, cout, k=(1, 1), s=(1, 1), pad=None, act=None, prec="bf16x3", n=3, tag=""):
    pad = SAME[k] if pad is None else pad
    name = f"{kernel}-{k[0]}x{k[1]}s{s[0]}{s[1]}-{cin}to{cout}-{hw[0]}x{hw[1]}-{act or 'none'}-{prec}{tag}"

    def build():
        t = gt.Tab(_seed(name), (hw[0], hw[1], cin))
        i = t.conv(-1, cin, cout, k=k, s=s, pad=pad)
        _set_act(t, i, act)
        _close(t, i, act)
        return t
    CASES.append(Case(name, build, 0, kernel, prec=prec, n=n))


VALID = (0, 0, 0, 0)
BR = (0, 1, 0, 1)  # TF "same" at stride 2 on an odd map: bottom / right only
# ---- split-bf16 MFMA convs: the issue's shapes, enlarged where the grid has to reach 9 blocks --------
conv_case("x3p", (17, 19), 32, 16, (3, 3), act="swish")
conv_case("x3p", (17, 19), 24, 10, (5, 3), act="relu")
conv_case("x3p", (18, 17), 20, 12, (2, 2), pad=VALID, act="sigmoid")
conv_case("x3t_256x16", (35, 33), 32, 12, (3, 3), (2, 2), BR, act="leaky")
conv_case("x3t_256x16", (27, 29), 16, 16, (5, 5), act=None)
conv_case("x3t_256x16", (9, 11), 40, 6, act="swish")
conv_case("x3t_128x32", (39, 47), 16, 24, (3, 3), (2, 2), BR, act="relu")
conv_case("x3t_128x32", (7, 9), 48, 30, act="sigmoid")
conv_case("x3t_64x128", (5, 7), 32, 250, act="leaky")
conv_case("x3t_64x128", (9, 10), 40, 252, (3, 3), act="swish")
conv_case("x3t_split_kc2", (9, 11), 384, 40, act=None)
conv_case("x3t_split_kc2", (5, 5), 376, 38, act="relu")
conv_case("x3t_split_kc1", (9, 11), 448, 72, act="leaky")
conv_case("x3t_split_kc1", (3, 7), 436, 70, act="sigmoid")
conv_case("x3t_split_kc1", (4, 4), 480, 40, act="swish")
conv_case("x3t_64x64_kc2", (13, 15), 64, 48, (3, 3), act="relu")
conv_case("x3t_64x64_kc2", (13, 11), 56, 70, (3, 3), (2, 2), (1, 1, 1, 1), act="swish")
conv_case("x3t_64x64_kc2", (12, 11), 384, 40, act="leaky")
conv_case("x3t_64x64_pd2", (15, 13), 288, 40, act="sigmoid")
conv_case("x3t_64x64_pd2", (9, 9), 280, 33, act=None)
conv_case("x3t_64x64", (13, 15), 32, 40, (3, 3), act="leaky")
conv_case("x3t_64x64", (9, 12), 90, 66, (5, 3), (1, 2), (2, 2, 0, 1), act="sigmoid")
conv_case("x3t_64x64", (5, 7), 96, 40, act="relu")
conv_case("x3t_64x64", (7, 9), 32, 40, act="swish", n=1, tag="-n1")
# ---- exact f32 convs ------------------------------------------------------------------------------
conv_case("f32_s", (35, 39), 3, 40, (3, 3), (2, 2), BR, act="swish")
conv_case("f32_s", (9, 10), 3, 33, (3, 3), act="relu", prec="f32")
conv_case("f32_lds_3x3x1", (17, 19), 1, 36, (3, 3), act="leaky")
conv_case("f32_lds", (17, 19), 4, 36, (5, 3), act="sigmoid")
conv_case("f32_lds", (7, 9), 40, 33, act=None, prec="f32")
conv_case("f32", (17, 19), 12, 9, (3, 3), act="swish")
conv_case("f32", (9, 10), 32, 40, (3, 3), act="leaky", prec="f32")
conv_case("f32", (17, 19), 12, 16, (3, 3), act="sigmoid", tag="-pair")   # K = 108: gconv_f32 only
# ---- matrix-vector products on 1 x 1 maps -------------------------------------------------------------
conv_case("matvec", (1, 1), 70, 6, act="swish")
conv_case("matvec", (1, 1), 65, 5, act=None)
conv_case("matvec", (1, 1), 300, 6, act="relu")       # K % 4 == 0: the float4 loop, a second round for 11 lanes
conv_case("matvec_t", (1, 1), 6, 70, act="sigmoid")
conv_case("matvec_t", (1, 1), 64, 300, act="leaky")   # two blocks of outputs
conv_case("matvec_t", (1, 1), 20, 9, act="relu")       # a partial second round of 16 products


# ---- fusions: SE scale and residual into an MFMA conv, closed by an identity affine ---------------
def se_res_case(kernel, hw, cin, cout, k, act, squeeze, res_from_conv):
    name = f"{kernel}-se-res-{k[0]}x{k[1]}-{cin}to{cout}-{hw[0]}x{hw[1]}-{act}"

    def build():
        t = gt.Tab(_seed(name), (hw[0], hw[1], cin))
        if res_from_conv:
            r = t.conv(-1, cin, cout)                                  # 0: the residual's producer
        else:
            r = t.node("affine", -1, off=(t.put(cin), t.put(cin)))     # (C_out == C_in)
        g = t.node("gavgpool", -1)                                     # 1
        a = t.conv(g, cin, squeeze, act="swish")                       # 2
        s = t.conv(a, squeeze, cin, act="sigmoid")                     # 3: the scale [n][C_in]
        m = t.node("mul", -1, s)                                       # 4: fused away
        c = t.conv(m, cin, cout, k=k, pad=SAME[k])                     # 5: the node under test
        t.node("add", c, r, act=act, alpha=0.2 if act == "leaky" else 0.0)   # 6: fused away
        t.node("affine", 6)                                            # 7: a copy of node 5's output
        return t
    CASES.append(Case(name, build, 5, kernel, fused=("se", "res")))


se_res_case("x3t_64x64_kc2", (5, 5), 48, 48, (1, 1), "swish", 12, False)
se_res_case("x3p", (17, 19), 32, 16, (3, 3), "relu", 8, True)
se_res_case("x3t_64x64_kc2", (5, 5), 48, 46, (1, 1), "leaky", 12, True)    # gconv_x3t's scalar residual reads
se_res_case("x3p", (17, 19), 32, 14, (3, 3), "swish", 8, True)             # gconv_x3p's, with scalar stores
se_res_case("x3t_split_kc2", (5, 5), 384, 38, (1, 1), "swish", 24, True)   # gsplit_reduce's scalar path
se_res_case("x3t_split_kc2", (5, 5), 384, 40, (1, 1), "swish", 24, True)   # its float4 path


# ---- depthwise convs --------------------------------------------------------------------------------
def dw_case(kernel, c, k, s, pad, act, mode):
    name = f"{kernel}-{k[0]}x{k[1]}s{s[0]}{s[1]}-C{c}-{act or 'none'}-{mode}"

    def build():
        t = gt.Tab(_seed(name), (9, 11, c))
        d = t.dw(-1, c, k=k, s=s, pad=pad, act=None, bias=True)
        _set_act(t, d, act)
        if mode == "node":
            _close(t, d, act)
        else:
            g = t.node("gavgpool", d)
            if mode == "map_x_pool":
                t.node("mul", d, g)
            else:
                t.node("affine", g)
        return t
    CASES.append(Case(name, build, 0 if mode != "pooled" else 1, kernel, mode=mode,
                      fused=() if mode == "node" else ("gap",)))


dw_case("dw4", 12, (3, 3), (1, 1), SAME[3, 3], None, "node")        # 297 lanes: two blocks
dw_case("dw4", 8, (3, 3), (2, 2), BR, "sigmoid", "node")
dw_case("dw1", 6, (5, 3), (2, 1), SAME[5, 3], "relu", "node")
dw_case("dw1", 7, (3, 3), (1, 1), SAME[3, 3], "leaky", "node")
dw_case("dw1", 5, (3, 3), (1, 1), SAME[3, 3], "swish", "node")
for _mode in ("map_x_pool", "pooled"):
    dw_case("dwpool4_s1", 40, (3, 3), (1, 1), SAME[3, 3], "swish", _mode)
    dw_case("dwpool4_s2", 36, (3, 3), (2, 2), (1, 1, 1, 1), "sigmoid", _mode)   # clamped loads on all four sides
    dw_case("dwpool4_k3", 8, (3, 3), (1, 2), (1, 1, 0, 1), "leaky", _mode)
    dw_case("dwpool4", 8, (5, 5), (1, 1), SAME[5, 5], "relu", _mode)
    dw_case("dwpool", 70, (3, 3), (1, 1), SAME[3, 3], None, _mode)


# ---- pools and element-wise nodes, each as its own output node (more than one block of 256 elements) ---
def simple_case(name, kernel, in_shape, fn, node, positive=False):
    def build():
        t = gt.Tab(_seed(name), in_shape)
        fn(t)
        return t
    CASES.append(Case(name, build, node, kernel, positive=positive))


simple_case("pool2d-max-3x3s2-pad", "pool2d", (17, 19, 6),
            lambda t: t.node("maxpool", -1, k=(3, 3), s=(2, 2), pad=(1, 1, 1, 1), act="relu"), 0)
simple_case("pool2d-avg-3x2s21-pad", "pool2d", (17, 19, 6),
            lambda t: t.node("avgpool", -1, k=(3, 2), s=(2, 1), pad=(1, 0, 0, 1)), 0)
simple_case("pool2d-avg-2x2s2", "pool2d", (9, 11, 5), lambda t: t.node("avgpool", -1, k=(2, 2), s=(2, 2), act="swish"), 0)
for _kern, _c in (("gpool4", 72), ("gpool", 70)):
    for _op in ("gmaxpool", "gavgpool"):
        # H W < 32 (and < 16 at 3 x 3), = 32, and no multiple of the 16 / 32 stripes
        for _hw in ((3, 3), (5, 5), (4, 8), (9, 11)):
            simple_case(f"{_kern}-{_op}-{_hw[0]}x{_hw[1]}-C{_c}", _kern, (_hw[0], _hw[1], _c),
                        lambda t, _op=_op: t.node(_op, -1), 0)


def _add(t):
    a = t.node("affine", -1, off=(t.put(6), t.put(6)))
    t.node("add", a, -1, act="relu")


def _mul_same(t):
    a = t.node("affine", -1, off=(t.put(6), t.put(6)))
    t.node("mul", a, -1)


def _mul_bcast(t):
    g = t.node("gavgpool", -1)
    t.node("mul", -1, g, act="swish")


simple_case("binary-add", "binary", (9, 11, 6), _add, 1)
simple_case("binary-mul-same", "binary", (9, 11, 6), _mul_same, 1)
simple_case("binary-mul-broadcast", "binary", (9, 11, 6), _mul_bcast, 1)
simple_case("affine-scale", "affine", (9, 11, 6), lambda t: t.node("affine", -1, off=(t.put(6), -1)), 0)
simple_case("affine-shift", "affine", (9, 11, 6), lambda t: t.node("affine", -1, act="relu", off=(-1, t.put(6))), 0)
simple_case("affine-both", "affine", (9, 11, 6),
            lambda t: t.node("affine", -1, act="leaky", alpha=0.3, off=(t.put(6), t.put(6))), 0)
simple_case("affine-identity", "affine", (9, 11, 6), lambda t: t.node("affine", -1), 0)
simple_case("pow-0.75", "pow", (12, 10, 6), lambda t: t.node("pow", -1, alpha=0.75), 0, positive=True)
simple_case("dense-K90-sigmoid-out", "dense", (3, 5, 6),
            lambda t: t.node("dense", -1, filters=5, act="sigmoid", off=(t.put((90, 5), 0.1), t.put(5, 0.1))), 0)
simple_case("dense-K288", "dense", (3, 8, 12),   # float4 loop, a second round for 8 lanes
            lambda t: t.node("dense", -1, filters=7, off=(t.put((288, 7), 0.1), t.put(7, 0.1))), 0)

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---- plans, prefix graphs, the evaluation ------------------------------------------------------------
def plan_of(L, tab, prec):
    d = gt.describe(L, tab.table(), prec, images=False)
    assert d["rc"] == 0, d
    return d


def prefix(tab, p):
    """The table cut after node p, plus an identity affine: node p's output as the graph's."""
    t = gt.Tab(0, tab.in_shape)
    t.nodes = [dict(d) for d in tab.nodes[:p + 1]]
    t.chunks, t.n = list(tab.chunks), tab.n
    t.node("affine", p)
    return t


def launch_grid(p, d, n):
    """run_conv_mfma's grid of an MFMA node (plan entry p, table node d) at batch n."""
    name = GK_NAME[p["kernel"]]
    bm, bn = TILE[name]
    pointwise = d["kh"] == 1 and d["kw"] == 1 and d["sh"] == 1 and d["sw"] == 1 and d["pt"] == 0 and d["pl"] == 0
    hwo, nz = (p["H"] * p["W"] * n, 1) if pointwise else (p["H"] * p["W"], n)
    if name == "x3p":
        return (-(-p["W"] // PATCH) * -(-p["H"] // PATCH), p["cout_pad"] // p["bn"], n)
    if name.startswith("x3t_split"):
        return (-(-hwo // 64), p["cout_pad"] // 64, p["split"])
    return (-(-hwo // bm), p["cout_pad"] // bn, nz)


def evaluate(case, L, run):
    """The oracle's check of the case's node on its actual inputs, and its output:
    dict(check=..., g=[n, H, W, C] float32, plan=..., tab=..., x=..., bufs=...)."""
    tab = case.tab()
    full = plan_of(L, tab, case.prec)
    plan = full["nodes"]
    x = case.input(tab.in_shape)
    i = case.node
    tgt = 0 if case.mode == "pooled" else i   # the launch whose inputs are read
    bufs = {-1: x}
    srcs = {plan[tgt][f] for f in ("in0", "in1", "scale_src", "res_src")}
    if case.mode == "map_x_pool":
        srcs.add(1)
    for p in sorted(s for s in srcs if s >= 0):
        pt = prefix(tab, p)
        pp = plan_of(L, pt, case.prec)["nodes"]
        for f in SAME_FIELDS:
            assert pp[p][f] == plan[p][f], (case.name, "prefix", p, f, pp[p][f], plan[p][f])
        bufs[p] = run(pt, case.prec, x).reshape(case.n, plan[p]["H"], plan[p]["W"], plan[p]["C"])
    out = run(tab, case.prec, x)
    blob = tab.table()[1]
    if case.mode == "node":
        if i != len(plan) - 1:  # a copy of node i is the output
            assert len(plan) - 1 > i and go.OPS[tab.nodes[-1]["op"]] == "affine" and plan[-1]["in0"] == i and \
                tab.nodes[-1]["off"] == [-1, -1] and plan[-1]["act"] == 0, (case.name, plan[-1])
        chk = go.node_check(tab.nodes, blob, plan, i, bufs)
        shape = (plan[i]["H"], plan[i]["W"], plan[i]["C"])
    else:
        dwc = go.node_check(tab.nodes, blob, plan, 0, bufs)
        if case.mode == "map_x_pool":
            chk = go.through_mul(dwc, bufs[1])
            shape = (plan[0]["H"], plan[0]["W"], plan[0]["C"])
        else:
            chk = go.pooled_after(dwc, go.ACTS[plan[1]["act"]], plan[1]["alpha"])
            shape = (1, 1, plan[1]["C"])
    g = out.reshape((case.n,) + shape)
    return dict(check=chk, g=g, plan=plan, tab=tab, x=x, bufs=bufs, blob=blob)


def cpu_run(L):
    """A stand-in for the GPU on a machine without one, as evaluate's `run`: every
    launched node's float64 result rounded to f32
    (oracle.graph_node_oracle.cpu_buffers), the last node's as [n, L]."""
    def run(tab, prec, x):
        plan = plan_of(L, tab, prec)["nodes"]
        bufs = go.cpu_buffers(tab.nodes, tab.table()[1], plan, x)
        return bufs[len(plan) - 1].reshape(x.shape[0], -1)
    return run
