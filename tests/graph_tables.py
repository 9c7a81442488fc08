"""Node tables for the graph planner's tests (test_graph_plan.py, the CPU pin;
test_gpu_graph_pin.py, the logits pin) and what one plan of them yields.

The networks are tools/make_models.graph_arch's with its seeded weight
generator (_graph_weights) and no BatchNormalization calibration: make_graph's
calibration runs float64 torch convolutions, whose sums are not the same bits
on every host, and the golden file pins SHA-256 hashes of the weight images
(BatchNormalization is folded into them by aa_amd.graph.graph_table, in numpy).
"""
import ctypes as C
import hashlib
import json

import numpy as np

from aa_amd import _lib
from aa_amd.graph import graph_table
from tools.make_models import _graph_weights, graph_arch

PRECS = {"f32": _lib.AA_PREC_F32, "bf16x3": _lib.AA_PREC_BF16X3}
G, ACT = _lib.AA_G, _lib.AA_GACT
N_LABELS = 7
CASES = ["effnet_c1", "effnet_c3", "effnetv2_c3", "hand_built", "resnet_c3", "wide_cout16"]  # tables()


def wide_kernel_arch(kernels, n_labels=N_LABELS):
    """tests/test_gpu_graph.py's C_out-16 wide-kernel network."""
    L = [{"type": "conv2d", "name": "stem", "filters": 32, "kernel": [3, 3], "strides": [1, 1],
          "padding": "same", "use_bias": True, "activation": "swish", "inputs": ["input"]}]
    x = "stem"
    for i, (kh, kw) in enumerate(kernels):
        L.append({"type": "conv2d", "name": f"k{i}", "filters": 16, "kernel": [kh, kw], "strides": [1, 1],
                  "padding": "same", "use_bias": True, "activation": "swish", "inputs": [x]})
        L.append({"type": "conv2d", "name": f"w{i}", "filters": 32, "kernel": [1, 1], "strides": [1, 1],
                  "padding": "same", "use_bias": True, "activation": "swish", "inputs": [f"k{i}"]})
        x = f"w{i}"
    L.append({"type": "globalavgpool2d", "name": "gap", "inputs": [x]})
    L.append({"type": "dense", "name": "fc", "units": n_labels, "use_bias": True, "activation": "sigmoid",
              "inputs": ["gap"]})
    return L


def arch_table(arch, in_shape, seed):
    tensors = _graph_weights(arch, in_shape[2], np.random.default_rng(seed))
    nodes, blob, _ = graph_table(arch, tensors, in_shape)
    return nodes, blob, tuple(in_shape)


class Tab:
    """A hand-built node table and its blob, from a seeded generator."""

    def __init__(self, seed, in_shape):
        self.rng = np.random.default_rng(seed)
        self.in_shape = tuple(in_shape)
        self.nodes, self.chunks, self.n = [], [], 0

    def put(self, shape, scale=1.0):
        a = (self.rng.standard_normal(shape) * scale).astype(np.float32).ravel()
        off, self.n = self.n, self.n + a.size
        self.chunks.append(a)
        return off

    def node(self, op, in0, in1=-1, k=(1, 1), s=(1, 1), pad=(0, 0, 0, 0), filters=0, act=None, alpha=0.0,
             off=(-1, -1)):
        self.nodes.append(dict(op=G[op], in0=in0, in1=in1, kh=k[0], kw=k[1], sh=s[0], sw=s[1], pt=pad[0], pb=pad[1],
                               pl=pad[2], pr=pad[3], filters=filters, act=ACT[act], alpha=alpha, off=list(off)))
        return len(self.nodes) - 1

    def conv(self, in0, cin, cout, k=(1, 1), s=(1, 1), pad=(0, 0, 0, 0), act=None, bias=True):
        off = [self.put((k[0], k[1], cin, cout), np.sqrt(2.0 / (k[0] * k[1] * cin))), self.put(cout, 0.1) if bias else -1]
        return self.node("conv", in0, k=k, s=s, pad=pad, filters=cout, act=act, off=off)

    def dw(self, in0, c, k=(3, 3), s=(1, 1), pad=(1, 1, 1, 1), act="swish", bias=False):
        off = [self.put((k[0], k[1], c), np.sqrt(2.0 / (k[0] * k[1]))), self.put(c, 0.1) if bias else -1]
        return self.node("dwconv", in0, k=k, s=s, pad=pad, act=act, off=off)

    def table(self):
        arr = (_lib.Node * len(self.nodes))()
        for a, d in zip(arr, self.nodes):
            for f in ("op", "in0", "in1", "kh", "kw", "sh", "sw", "pt", "pb", "pl", "pr", "filters", "act"):
                setattr(a, f, int(d[f]))
            a.alpha = float(d["alpha"])
            a.off[0], a.off[1] = int(d["off"][0]), int(d["off"][1])
        return arr, np.concatenate(self.chunks) if self.chunks else np.zeros(1, np.float32), self.in_shape


def hand_built(seed=41):
    """What the networks miss: affine nodes with a scale only / a shift only,
    pow, a max and an average pool, a dangling branch, a Dense on an H x W > 1
    map, depthwise convs with C % 4 != 0 (alone, and with the global average
    pool that reads them), depthwise + pool shapes outside the chunked 3x3
    kernels, a global max pool, 1x1 convs on 1x1 maps with K <= 64 and K > 64,
    and a 9-chunk pointwise conv (two K steps in flight)."""
    t = Tab(seed, (12, 10, 6))
    p = t.node("pow", -1, alpha=0.75)
    a = t.node("affine", p, off=(t.put(6), -1))                       # scale only
    a = t.node("affine", a, act="relu", off=(-1, t.put(6)))           # shift only
    t.node("maxpool", a, k=(5, 5), s=(3, 3), act="relu")              # dangling: nobody reads it
    d = t.dw(a, 6, bias=True)                                         # C % 4 != 0
    m = t.node("maxpool", d, k=(3, 3), s=(1, 1), pad=(1, 1, 1, 1))
    v = t.node("avgpool", m, k=(2, 2), s=(2, 2))                      # 6 x 5 x 6
    d = t.dw(v, 6, k=(3, 2), pad=(1, 1, 0, 1))                        # scalar depthwise + pool
    g = t.node("gavgpool", d)
    r = t.conv(g, 6, 70, act="swish")                                 # 1x1 map, K = 6: gmatvec_t
    e = t.conv(r, 70, 6, act="sigmoid")                               # 1x1 map, K = 70: gmatvec
    x = t.node("mul", d, e)
    x = t.conv(x, 6, 288, k=(3, 3), pad=(1, 1, 1, 1), act="swish")    # 6 x 5 x 288
    y = t.dw(x, 288, s=(1, 2))                                        # 3x3 with unequal strides + pool
    g = t.node("gavgpool", y)
    x = t.node("mul", y, g)                                           # 6 x 3 x 288
    q = t.node("gmaxpool", v)                                         # C % 4 != 0: ggpool
    x = t.conv(x, 288, 40, bias=False)                                # 9 chunks: PD = 2 (or its SE-fused form)
    x = t.node("add", x, x)
    x = t.node("mul", x, t.conv(q, 6, 40))                            # broadcast of a [1][1][40] product
    t.node("dense", x, filters=5, act="sigmoid", off=(t.put((6 * 3 * 40, 5), 0.05), t.put(5, 0.1)))
    return t.table()


def smallest_split_k_T(limit=64):
    """The smallest T at which some node of the effnetv2 network still plans as
    split-K (a pointwise conv with C_in >= 384 on a map of <= 128 pixels)."""
    L = _lib.lib()
    for T in range(1, limit):
        got = describe(L, arch_table(graph_arch("effnetv2", N_LABELS), (160, T, 3), 5), "bf16x3", images=False)
        if any(n["split"] > 1 and n["kernel"] in (_lib.AA_GK["x3t_split_kc2"], _lib.AA_GK["x3t_split_kc1"])
               for n in got["nodes"]):
            return T
    raise AssertionError("no split-K node")


EFFNETV2_T = 1  # == smallest_split_k_T() (asserted by test_graph_plan.py)


def tables():
    """name -> (aa_node array, blob, input shape)"""
    out = {
        "effnet_c1": arch_table(graph_arch("effnet", N_LABELS), (160, 113, 1), 1),
        "effnet_c3": arch_table(graph_arch("effnet", N_LABELS), (160, 113, 3), 2),
        "resnet_c3": arch_table(graph_arch("resnet", N_LABELS), (160, 113, 3), 3),
        "effnetv2_c3": arch_table(graph_arch("effnetv2", N_LABELS), (160, EFFNETV2_T, 3), 5),
        "wide_cout16": arch_table(wide_kernel_arch([(5, 5), (3, 3), (4, 6), (5, 3), (3, 7), (1, 10)]), (40, 70, 1), 11),
        "hand_built": hand_built(),
    }
    return out


def rejections():
    """name -> (table, precision): every refusal of aa_graph_create a node table reaches."""
    out = {}

    def base():
        t = Tab(50, (9, 8, 4))
        t.conv(-1, 4, 8, k=(3, 3), pad=(1, 1, 1, 1), act="relu")
        return t

    def edit(name, fn, prec="f32", t=None):
        t = t or base()
        fn(t)
        out[name] = (t.table(), prec)

    edit("reads_later_node", lambda t: t.node("affine", 1))
    edit("reads_later_node_in1", lambda t: t.node("add", 0, 5))
    edit("reads_before_input", lambda t: t.node("affine", -2))
    edit("activation", lambda t: t.nodes[0].update(act=5))
    edit("activation_negative", lambda t: t.nodes[0].update(act=-1))
    edit("window_zero", lambda t: t.node("maxpool", 0, k=(0, 2)))
    edit("stride_zero", lambda t: t.nodes[0].update(sw=0))
    edit("pad_negative", lambda t: t.nodes[0].update(pb=-1))
    edit("input_smaller_than_window", lambda t: t.node("avgpool", 0, k=(10, 2)))
    edit("filters_zero", lambda t: t.nodes[0].update(filters=0))
    edit("conv_kernel_past", lambda t: t.nodes[0]["off"].__setitem__(0, t.n - 5))
    edit("conv_kernel_neg", lambda t: t.nodes[0]["off"].__setitem__(0, -3))
    edit("conv_bias_past", lambda t: t.nodes[0]["off"].__setitem__(1, t.n - 2))
    edit("dw_kernel_past", lambda t: t.nodes[t.dw(0, 8)]["off"].__setitem__(0, t.n - 1))
    edit("dw_bias_past", lambda t: t.nodes[t.dw(0, 8, bias=True)]["off"].__setitem__(1, t.n - 1))
    edit("add_shapes", lambda t: t.node("add", 0, -1))
    edit("mul_broadcast_channels", lambda t: t.node("mul", 0, t.conv(t.node("gavgpool", 0), 8, 9)))
    edit("affine_scale_past", lambda t: t.node("affine", 0, off=(t.n - 3, -1)))
    edit("affine_shift_past", lambda t: t.node("affine", 0, off=(-1, t.n - 3)))
    edit("dense_units_zero", lambda t: t.node("dense", 0, filters=0, off=(0, -1)))
    edit("dense_kernel_past", lambda t: t.node("dense", 0, filters=3, off=(t.n - 10, -1)))
    edit("dense_bias_past", lambda t: t.node("dense", 0, filters=1, off=(t.put((9 * 8 * 8, 1)), t.n - 0)))
    edit("op_unknown", lambda t: t.nodes.append(dict(t.nodes[0], op=12)))
    edit("op_zero", lambda t: t.nodes[0].update(op=0), prec="bf16x3")
    return out


def image(L, h, node, which):
    n = C.c_size_t()
    assert L.aa_graph_node_image(h, node, which, None, 0, C.byref(n)) == 0
    buf = np.zeros(n.value, np.uint8)
    assert L.aa_graph_node_image(h, node, which, buf.ctypes.data, buf.size, C.byref(n)) == 0
    return buf


def pin_input(case, table, n=3):
    """n seeded windows for `table`: dB-like values for the networks, positive
    ones for the hand-built table (its first node is a pow)."""
    H, W, Cin = table[2]
    rng = np.random.default_rng(sum(map(ord, case)))
    lo, hi = (0.1, 2.0) if case == "hand_built" else (-80.0, 0.0)
    return rng.uniform(lo, hi, (n, H, W, Cin)).astype(np.float32)


def forward3(L, table, prec, x):
    """aa_graph_forward's logits from three calls with identical buffers on one
    stream: direct launches, then the capture, then its replay."""
    import torch
    nodes, blob, (H, W, Cin) = table
    h = C.c_void_p()
    _lib.check(L.aa_graph_create(nodes, len(nodes), blob.ctypes.data, blob.size, H, W, Cin, PRECS[prec], C.byref(h)),
               "aa_graph_create")
    n, nl = x.shape[0], L.aa_graph_n_outputs(h)
    out = []
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        xt = torch.from_numpy(x).cuda()
        ws = torch.empty(L.aa_graph_workspace_bytes(h, n), dtype=torch.uint8, device=xt.device)
        lg = torch.empty((n, nl), dtype=torch.float32, device=xt.device)
        for _ in range(3):
            lg.fill_(float("nan"))
            _lib.check(L.aa_graph_forward(h, _lib.dptr(xt), n, _lib.dptr(lg), None, _lib.dptr(ws), ws.numel(),
                                          _lib.stream_ptr(s)), "aa_graph_forward")
            out.append(lg.cpu().numpy().copy())
    torch.cuda.synchronize()
    L.aa_graph_destroy(h)
    return out


GUARD = 256  # floats of NaN before and after the input (a multiple of 64: the kernels load float4s)


def guarded_input(x, device="cuda"):
    """x on the device inside a larger NaN-filled allocation: (the view of x, the
    allocation).  A kernel that reads outside the batch reads NaN."""
    import torch
    buf = torch.full((GUARD + x.size + GUARD,), float("nan"), dtype=torch.float32, device=device)
    xt = buf[GUARD:GUARD + x.size].view(x.shape)
    xt.copy_(torch.from_numpy(x))
    assert xt.is_contiguous() and xt.data_ptr() % 256 == 0
    return xt, buf


def forward3_guarded(L, table, prec, x):
    """forward3 with traps: the input between NaN guard bands (guarded_input), the
    workspace filled with NaN bytes before each of the three calls (an element no
    block writes, or a split-K slice nobody wrote, stays NaN), logits and probs
    NaN-filled too.  Returns ([logits] * 3, [probs] * 3, sigmoid_out)."""
    import torch
    nodes, blob, (H, W, Cin) = table
    h = C.c_void_p()
    _lib.check(L.aa_graph_create(nodes, len(nodes), blob.ctypes.data, blob.size, H, W, Cin, PRECS[prec], C.byref(h)),
               "aa_graph_create")
    lay = _lib.GraphLayout()
    assert L.aa_graph_plan_layout(h, C.byref(lay)) == 0
    n, nl = x.shape[0], L.aa_graph_n_outputs(h)
    logits, probs = [], []
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        xt, keep = guarded_input(x)
        ws = torch.empty(L.aa_graph_workspace_bytes(h, n), dtype=torch.uint8, device=xt.device)
        lg = torch.empty((n, nl), dtype=torch.float32, device=xt.device)
        pr = torch.empty((n, nl), dtype=torch.float32, device=xt.device)
        for _ in range(3):
            ws.fill_(0xFF)
            lg.fill_(float("nan"))
            pr.fill_(float("nan"))
            _lib.check(L.aa_graph_forward(h, _lib.dptr(xt), n, _lib.dptr(lg), _lib.dptr(pr), _lib.dptr(ws), ws.numel(),
                                          _lib.stream_ptr(s)), "aa_graph_forward")
            logits.append(lg.cpu().numpy().copy())
            probs.append(pr.cpu().numpy().copy())
    torch.cuda.synchronize()
    L.aa_graph_destroy(h)
    del keep
    return logits, probs, bool(lay.sigmoid_out)


def node_digest(node):
    """One node of describe() as the golden file keeps it: [name, launch
    variant, the first 16 hex digits of the SHA-256 over every field (name,
    flops, bytes, the aa_node_plan fields, length and SHA-256 of each image)]."""
    text = json.dumps(node, sort_keys=True, separators=(",", ":"))
    return [node["name"], node["kernel"], hashlib.sha256(text.encode()).hexdigest()[:16]]


PLAN_FIELDS = [f for f, _ in _lib.NodePlan._fields_]


def describe(L, table, prec, images=True):
    """What one plan of `table` yields, as plain JSON values."""
    nodes, blob, (H, W, Cin) = table
    h = C.c_void_p()
    rc = L.aa_graph_plan(nodes, len(nodes), blob.ctypes.data, blob.size, H, W, Cin, PRECS[prec], C.byref(h))
    if rc != 0:
        return {"rc": rc, "error": L.aa_last_error().decode()}
    lay = _lib.GraphLayout()
    assert L.aa_graph_plan_layout(h, C.byref(lay)) == 0
    assert L.aa_graph_n_outputs(h) == lay.n_outputs
    out = {"rc": 0, "per_win": lay.per_win, "part_off": lay.part_off, "L": lay.n_outputs,
           "sigmoid_out": lay.sigmoid_out, "workspace_1": L.aa_graph_workspace_bytes(h, 1),
           "workspace_7": L.aa_graph_workspace_bytes(h, 7), "nodes": []}
    for i in range(L.aa_graph_n_stages(h)):
        name = C.create_string_buffer(128)
        fl, by = C.c_double(), C.c_double()
        assert L.aa_graph_stage_info(h, i, name, 128, C.byref(fl), C.byref(by)) == 0
        p = _lib.NodePlan()
        assert L.aa_graph_node_plan(h, i, C.byref(p)) == 0
        d = {"name": name.value.decode(), "flops": fl.value, "bytes": by.value}
        d.update({f: getattr(p, f) for f in PLAN_FIELDS})
        if images:
            d["images"] = [[int(b.size), hashlib.sha256(b.tobytes()).hexdigest() if b.size else ""]
                           for b in (image(L, h, i, w) for w in range(4))]
        out["nodes"].append(d)
    L.aa_graph_destroy(h)
    return out
