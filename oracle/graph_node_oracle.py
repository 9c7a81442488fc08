"""One node of a graph model in float64, its derived bound and the interval rule
(DESIGN.md 5b "Per-node checks of the graph kernels").

A node is what one launch of aa_graph_forward computes (aa_graph_plan.h
choose_kernel): a conv with whatever graph_fuse put into it (a
squeeze-and-excite scale on its input, a residual added before the
activation), a depthwise conv, a pool, an element-wise node, a Dense.  The
reference reads the node's ACTUAL inputs -- float32 arrays the caller read
from the GPU with prefix graphs -- so errors do not accumulate and a failure
names one kernel (the rule of 5a).

Bound B on the value before the activation, A = |W| (*) |x| + |bias| (+ |res|
where a residual is fused), K the length of the sum, U24 = 2^-24:

  split-bf16 MFMA convs  (SPLIT_C + (K + 8) U24) A   (5a's row for gconv_x3)
    + a fused SE scale   + U24 A: the staged input is fl(x s) = x s (1 + d),
                         |d| <= U24, and the reference multiplies exactly, so
                         every product moves by at most U24 |w x s|
    + split K            + (split - 1) U24 A: the slices are summed in order
                         by gsplit_reduce, split - 1 f32 additions of partial
                         sums that are each at most A (conservative: the
                         (K + 8) term already covers any summation tree)
  exact f32 sums         (K + 8) U24 A: gconv_f32*, gmatvec*, Dense (K the
                         sum's length), depthwise (K = kh kw), average pools
                         (K = the window's taps, or H W)
  max pools              0: a selection, no rounding
  add, mul               1 U24 |r|: one rounding of the exact sum / product
  affine                 1 U24 |r|: gaffine is one fmaf (with a scale: a single
                         rounding of x s + shift, however much the two cancel),
                         one add (shift only) or a copy (neither: B = 0)
  pow                    no accuracy statement for the device library's powf
                         is available to this project, so 4 x the largest
                         relative error of the float32 CPU pow on the same
                         inputs (POW_MARGIN; both numbers are reported)
Every B also gets TINY = 2^-126 (results below the smallest normal f32).

Activations put the interval's ends through the activation (act_interval):
none, relu, leaky with a slope in [0, 1] are monotone and rounded as the
kernels round them (f32); sigmoid is monotone; swish is not -- its minimum is
at v = SWISH_MIN_V, so the image of [lo, hi] is [min over both ends and the
minimum where lo <= SWISH_MIN_V <= hi, max over both ends].

Slack of the kernels' fast logistic (aa_gconv.h glogistic):
s^ = rcp(fl(1 + exp2(fl(v c)))), c = fl(-log2 e), exp2 and rcp within 1 ulp
(relative 2 U24), the product and the add correctly rounded (U24).
  t = fl(v c) = -v log2 e (1 + d1), |d1| <= 2 U24 (rounding of c and of the
  product); 2^t = e^-v e^(-v d1): relative |v| 2 U24.  With exp2's own ulp
  E^ = e^-v (1 + eE), |eE| <= (2 |v| + 2) U24.  1 + E^ = (1 + E)(1 + (1 - s) eE)
  with s = 1 / (1 + E); the add and rcp contribute U24 + 2 U24.  So
      |s^ - s| <= s U24 (3 + (1 - s)(2 |v| + 2))            (logistic_slack)
  and for swish, fl(v s^): |v| times that plus U24 |v s|.
Floor TINY: for large -v 2^t overflows to inf and rcp returns 0 (the exact
value is below the smallest normal), and rcp may flush a denormal result.

The output node's own sigmoid is not one of these: gfinal applies it with
expf and a division to the logits (final_probs_bound).
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.cnn_oracle import SPLIT_C, U24, _absconv, interval_violations  # noqa: F401 (re-exported)

TINY = 2.0 ** -126
SWISH_MIN_V = -1.2784645427610738  # root of 1 + e^-v (1 + v) = 0
POW_MARGIN = 4.0
OPS = {1: "conv", 2: "dwconv", 3: "maxpool", 4: "avgpool", 5: "gmaxpool", 6: "gavgpool", 7: "add", 8: "mul",
       9: "affine", 10: "dense", 11: "pow"}
ACTS = {0: None, 1: "relu", 2: "leaky", 3: "sigmoid", 4: "swish"}
MFMA_KERNELS = set(range(1, 10))   # aa_gkernel x3p .. x3t_64x64
SPLIT_KERNELS = {5, 6}


# ---- activations ------------------------------------------------------------------
def logistic64(v):
    v = np.asarray(v, np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-v))


def logistic_slack(v):
    """|glogistic(v) - logistic(v)| for an f32 v, from its four roundings (module docstring)."""
    v = np.asarray(v, np.float64)
    s = logistic64(v)
    return s * U24 * (3.0 + (1.0 - s) * (2.0 * np.abs(v) + 2.0)) + TINY


def act_slack(v, act):
    """Absolute slack of gact at pre-activation v for sigmoid / swish; 0 otherwise."""
    v = np.asarray(v, np.float64)
    if act == "sigmoid":
        return logistic_slack(v)
    if act == "swish":
        return np.abs(v) * logistic_slack(v) + U24 * np.abs(v * logistic64(v)) + TINY
    return np.zeros_like(v)


def act64(v, act, alpha=0.0):
    v = np.asarray(v, np.float64)
    if act is None:
        return v
    if act == "relu":
        return np.maximum(v, 0.0)
    if act == "leaky":
        return np.where(v >= 0, v, v * float(np.float32(alpha)))
    if act == "sigmoid":
        return logistic64(v)
    if act == "swish":
        return v * logistic64(v)
    raise ValueError(act)


def _act32_monotone(v, act, alpha):
    """none / relu / leaky as the kernels apply them: on the f32 value, in f32."""
    v32 = np.asarray(v, np.float64).astype(np.float32)
    if act == "relu":
        v32 = np.maximum(v32, np.float32(0))
    elif act == "leaky":
        v32 = np.where(v32 >= 0, v32, v32 * np.float32(alpha))
    return v32.astype(np.float64)


def act_interval(lo, hi, act, alpha=0.0):
    """The interval the activation's output lies in when its f32 argument lies in [lo, hi]."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    if act in (None, "relu", "leaky"):
        assert act != "leaky" or 0.0 <= alpha <= 1.0, "leaky slopes outside [0, 1] are not monotone non-decreasing"
        return _act32_monotone(lo, act, alpha), _act32_monotone(hi, act, alpha)
    a, b = act64(lo, act), act64(hi, act)
    out_lo, out_hi = np.minimum(a, b), np.maximum(a, b)
    if act == "swish":
        inside = (lo <= SWISH_MIN_V) & (SWISH_MIN_V <= hi)
        out_lo = np.where(inside, act64(SWISH_MIN_V, "swish"), out_lo)
    mid = (lo + hi) / 2
    slack = np.maximum(np.maximum(act_slack(lo, act), act_slack(hi, act)), act_slack(mid, act))
    return out_lo - slack, out_hi + slack


def gact_f32(v32, act, alpha=0.0):
    """gact in f32 with the fast logistic's four roundings, exp2 and rcp correctly
    rounded (a correct kernel may differ from this by their ulp)."""
    v32 = np.asarray(v32, np.float32)
    if act in (None, "relu", "leaky"):
        return _act32_monotone(v32, act, alpha).astype(np.float32)
    t = v32 * np.float32(-1.44269504088896341)
    with np.errstate(over="ignore"):
        e = np.exp2(t.astype(np.float64)).astype(np.float32)
        d = np.float32(1) + e
        s = (1.0 / d.astype(np.float64)).astype(np.float32)
    return s if act == "sigmoid" else v32 * s


def final_probs_bound(logits):
    """gfinal's 1 / (1 + expf(-v)): expf within 1 ulp (relative 2 U24 on e^-v), the
    add and the division correctly rounded: s U24 (2 + 2 (1 - s)) + TINY."""
    s = logistic64(logits)
    return s * U24 * (2.0 + 2.0 * (1.0 - s)) + TINY


# ---- the node -----------------------------------------------------------------------
def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double().permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def conv_weights(d, blob, cin):
    """(w [O, I, kh, kw], bias [O]) float64 of a conv / depthwise node (depthwise as a
    block-diagonal full conv: the same sums, and _absconv serves both)."""
    kh, kw = d["kh"], d["kw"]
    if OPS[d["op"]] == "conv":
        co = d["filters"]
        w = torch.from_numpy(blob[d["off"][0]:d["off"][0] + kh * kw * cin * co].reshape(kh, kw, cin, co).copy())
        w = w.double().permute(3, 2, 0, 1).contiguous()
    else:
        co = cin
        k = torch.from_numpy(blob[d["off"][0]:d["off"][0] + kh * kw * cin].reshape(kh, kw, cin).copy()).double()
        w = torch.zeros((cin, cin, kh, kw), dtype=torch.float64)
        idx = torch.arange(cin)
        w[idx, idx] = k.permute(2, 0, 1)
    b = (torch.from_numpy(blob[d["off"][1]:d["off"][1] + co].copy()).double() if d["off"][1] >= 0
         else torch.zeros(co, dtype=torch.float64))
    return w, b


def pad_input(x, d, value=0.0):
    return F.pad(x, (d["pl"], d["pr"], d["pt"], d["pb"]), value=value)


def _conv(xp, w, b, d):
    """(y, A) of a conv on the padded input xp: the strided conv and the abs-conv
    (cnn_oracle._absconv is stride 1: taken at the strided positions)."""
    y = F.conv2d(xp, w, stride=(d["sh"], d["sw"])) + b[None, :, None, None]
    A = _absconv(xp, w, b)[:, :, ::d["sh"], ::d["sw"]]
    return y, A


@torch.no_grad()
def node_pre(nodes, blob, plan, i, bufs):
    """Node i before its activation: dict of y (float64 centre), B (bound), A, K, all
    [n, H, W, C] float64 numpy (K an int), and the activation the launch applies.
    nodes: graph_tables.Tab.nodes; plan: graph_tables.describe(...)["nodes"];
    bufs[k]: the float32 output of node k ([n, H, W, C]; -1: the graph's input)."""
    d, p = nodes[i], plan[i]
    op = OPS[d["op"]]
    assert not p["skip"], "a fused-away node launches nothing"
    last = i == len(plan) - 1
    act, alpha = ACTS[p["act"]], float(p["alpha"])
    if last and act == "sigmoid":
        act = None  # gfinal applies it: the logits are the values before it
    a = np.asarray(bufs[p["in0"]], np.float32)
    n = a.shape[0]
    x = _nchw(a)
    extra = ""
    if op in ("conv", "dwconv"):
        cin = a.shape[3]
        w, b = conv_weights(d, blob, cin)
        K = d["kh"] * d["kw"] * (cin if op == "conv" else 1)
        c_rel = (K + 8) * U24
        if p["scale_src"] >= 0:
            s = _nchw(np.asarray(bufs[p["scale_src"]], np.float32).reshape(n, 1, 1, cin))
            x = x * s
            c_rel += U24
            extra += "+se"
        y, A = _conv(pad_input(x, d), w, b, d)
        if p["res_src"] >= 0:
            res = _nchw(np.asarray(bufs[p["res_src"]], np.float32))
            y, A = y + res, A + res.abs()
            extra += "+res"
        if p["kernel"] in MFMA_KERNELS:
            c_rel += SPLIT_C
            if p["kernel"] in SPLIT_KERNELS:
                c_rel += (p["split"] - 1) * U24
        B = c_rel * A
    elif op == "dense":
        K = a.shape[1] * a.shape[2] * a.shape[3]
        units = d["filters"]
        w = torch.from_numpy(blob[d["off"][0]:d["off"][0] + K * units].reshape(K, units).copy()).double()
        b = (torch.from_numpy(blob[d["off"][1]:d["off"][1] + units].copy()).double() if d["off"][1] >= 0
             else torch.zeros(units, dtype=torch.float64))
        flat = torch.from_numpy(a.reshape(n, K)).double()
        y = (flat @ w + b)[:, :, None, None]
        A = (flat.abs() @ w.abs() + b.abs())[:, :, None, None]
        B = (K + 8) * U24 * A
    elif op in ("maxpool", "avgpool"):
        K = d["kh"] * d["kw"]
        k, s = (d["kh"], d["kw"]), (d["sh"], d["sw"])
        if op == "maxpool":
            y = F.max_pool2d(pad_input(x, d, -float("inf")), k, s)
            A, B = y.abs(), torch.zeros_like(y)
        else:
            cnt = F.avg_pool2d(pad_input(torch.ones_like(x), d), k, s, divisor_override=1)
            y = F.avg_pool2d(pad_input(x, d), k, s, divisor_override=1) / cnt
            A = F.avg_pool2d(pad_input(x.abs(), d), k, s, divisor_override=1) / cnt
            B = (K + 8) * U24 * A
    elif op in ("gmaxpool", "gavgpool"):
        K = a.shape[1] * a.shape[2]
        if op == "gmaxpool":
            y = x.amax(dim=(2, 3), keepdim=True)
            A, B = y.abs(), torch.zeros_like(y)
        else:
            y, A = x.mean(dim=(2, 3), keepdim=True), x.abs().mean(dim=(2, 3), keepdim=True)
            B = (K + 8) * U24 * A
    elif op in ("add", "mul"):
        K = 1
        bb = np.asarray(bufs[p["in1"]], np.float32)
        z = _nchw(bb.reshape(n, 1, 1, -1) if bb.ndim == 2 else bb)
        y = x + z if op == "add" else x * z
        A = x.abs() + z.abs() if op == "add" else y.abs()
        B = U24 * y.abs()
    elif op == "affine":
        K = 1
        C = a.shape[3]
        col = lambda off: torch.from_numpy(blob[off:off + C].copy()).double()[None, :, None, None]
        sc = col(d["off"][0]) if d["off"][0] >= 0 else None
        sh = col(d["off"][1]) if d["off"][1] >= 0 else None
        y = x if sc is None else x * sc
        A = y.abs()
        if sh is not None:
            y, A = y + sh, A + sh.abs()
        B = U24 * y.abs() if (sc is not None or sh is not None) else torch.zeros_like(A)
    elif op == "pow":
        K = 1
        e = float(np.float32(d["alpha"]))
        y = x ** e
        cpu32 = torch.from_numpy(a).permute(0, 3, 1, 2) ** np.float32(e)
        rel = float(((cpu32.double() - y).abs() / y.abs().clamp(min=TINY)).max())
        A = y.abs()
        B = POW_MARGIN * rel * A
        extra += f" pow: f32 CPU max rel {rel:.3e} x {POW_MARGIN:g}"
    else:
        raise ValueError(op)
    return dict(y=_nhwc(y), B=_nhwc(B) + TINY, A=_nhwc(A), K=K, act=act, alpha=alpha, op=op, extra=extra)


def node_check(nodes, blob, plan, i, bufs):
    """node_pre plus the interval rule's ends: r = act(y), lo / hi = the activation's
    image of [y - B, y + B] (act_interval).  An output element g is correct iff
    lo <= g <= hi (interval_violations)."""
    d = node_pre(nodes, blob, plan, i, bufs)
    d["lo"], d["hi"] = act_interval(d["y"] - d["B"], d["y"] + d["B"], d["act"], d["alpha"])
    d["r"] = act64(d["y"], d["act"], d["alpha"])
    return d


def through_mul(d, q):
    """The check d of a map taken through an exact-input Multiply by q (float32,
    [n, 1, 1, C] or the map's shape): fl(g q) is monotone in g for a fixed q, so the
    interval's ends go through the f32 product (sorted: q may be negative)."""
    q = np.asarray(q, np.float32).astype(np.float64)
    q = q.reshape(q.shape[0], 1, 1, -1) if q.ndim == 2 else q
    a = (d["lo"] * q).astype(np.float32).astype(np.float64)
    b = (d["hi"] * q).astype(np.float32).astype(np.float64)
    out = dict(d)
    out["lo"], out["hi"] = np.minimum(a, b), np.maximum(a, b)
    out["r"], out["B"], out["A"] = d["r"] * q, d["B"] * np.abs(q) + TINY, d["A"] * np.abs(q)
    return out


def pooled_after(d, pool_act=None, pool_alpha=0.0):
    """The check of the pooled vector a depthwise conv + global average pool launch
    writes, from the check d of the depthwise map (both in one launch: the map's
    interval goes through the mean, plus the mean's own (H W + 8) U24 term)."""
    n, H, W, C = d["lo"].shape
    mag = np.maximum(np.abs(d["lo"]), np.abs(d["hi"])).mean(axis=(1, 2), keepdims=True)
    Bp = (H * W + 8) * U24 * mag + TINY
    lo, hi = d["lo"].mean(axis=(1, 2), keepdims=True) - Bp, d["hi"].mean(axis=(1, 2), keepdims=True) + Bp
    y = d["r"].mean(axis=(1, 2), keepdims=True)
    out = dict(y=y, A=mag, B=(hi - lo) / 2, K=H * W, act=pool_act, alpha=pool_alpha, op="gavgpool", extra="+dw")
    out["lo"], out["hi"] = act_interval(lo, hi, pool_act, pool_alpha)
    out["r"] = act64(y, pool_act, pool_alpha)
    return out


# ---- the split-bf16 emulation and its planted defects ---------------------------------
def _split(t32):
    hi = t32.to(torch.bfloat16).float()
    return hi, (t32 - hi).to(torch.bfloat16).float()


@torch.no_grad()
def mfma_emulation(nodes, blob, plan, i, bufs, defect=None):
    """The MFMA convs' arithmetic on the CPU: x (times the SE scale, in f32) and W
    split into bf16 hi + lo, hi.hi + lo.hi + hi.lo accumulated in float32, bias,
    residual and the activation in f32 (gact_f32).  Returns the output [n, H, W, C]
    float32.  defect: one of DEFECTS, planted into this arithmetic."""
    d, p = nodes[i], plan[i]
    assert p["kernel"] in MFMA_KERNELS
    last = i == len(plan) - 1
    act, alpha = ACTS[p["act"]], float(p["alpha"])
    if last and act == "sigmoid":
        act = None
    a = np.asarray(bufs[p["in0"]], np.float32)
    n, cin = a.shape[0], a.shape[3]
    x = torch.from_numpy(a).permute(0, 3, 1, 2).contiguous()
    w64, b64 = conv_weights(d, blob, cin)
    w, b = w64.float(), b64.float()
    if p["scale_src"] >= 0:
        s = torch.from_numpy(np.asarray(bufs[p["scale_src"]], np.float32).reshape(n, cin, 1, 1).copy())
        if defect == "se_window":
            s = torch.roll(s, 1, 0)
        x = x * s
    elif defect == "se_window":
        return None
    if defect == "quad":  # the last 8-channel quad of a partial 32-chunk
        if cin % 32 == 0:
            return None
        x = x.clone()
        x[:, (cin - 1) // 8 * 8:] = 0
    if defect == "slice":  # one split-K slice (the last) left out
        if p["kernel"] not in SPLIT_KERNELS:
            return None
        x = x.clone()
        x[:, (p["split"] - 1) * p["cslice"] * 32:] = 0
    xp = pad_input(x, d)
    if defect == "clamp":  # the padding column next to the image reads the clamped pixel
        if d["pl"] == 0:
            return None
        xp[:, :, d["pt"]:d["pt"] + x.shape[2], d["pl"] - 1] = x[:, :, :, 0]
    xh, xl = _split(xp)
    wh, wl = _split(w)
    st = (d["sh"], d["sw"])
    acc = F.conv2d(xh, wh, stride=st) + F.conv2d(xl, wh, stride=st)
    if defect != "lohi":
        acc = acc + F.conv2d(xh, wl, stride=st)
    if defect == "bias":  # another channel's bias on top of the last real channel's
        if d["off"][1] < 0:
            return None
        b = b.clone()
        b[-1] += b[0] if b.numel() > 1 else b[-1]
    v = acc + b[None, :, None, None]
    if p["res_src"] >= 0:
        v = v + torch.from_numpy(np.asarray(bufs[p["res_src"]], np.float32)).permute(0, 3, 1, 2)
    v = v.permute(0, 2, 3, 1).contiguous().numpy()
    out = gact_f32(v, act, alpha)
    if defect == "swish_relu":
        if act != "swish":
            return None
        idx = np.unravel_index(int(np.argmin(np.abs(np.abs(v) - 1.0))), v.shape)  # |v| nearest 1
        out = out.copy()
        out[idx] = max(v[idx], np.float32(0))
    return out


# (a) .. (g) of the issue
DEFECTS = ["lohi", "clamp", "quad", "se_window", "bias", "slice", "swish_relu"]
RMS_MARGIN = 4.0  # the project's margin over an emulation (5a)


def rms_ratio(g, d, emu):
    """rms((g - r) / A) / rms((emu - r) / A): the rms gate is ratio <= RMS_MARGIN."""
    A = np.maximum(d["A"], TINY)
    with np.errstate(invalid="ignore"):
        num = np.sqrt(np.mean(((np.asarray(g, np.float64) - d["r"]) / A) ** 2))
        den = np.sqrt(np.mean(((np.asarray(emu, np.float64) - d["r"]) / A) ** 2))
    return float(num / max(den, TINY))


def cpu_buffers(nodes, blob, plan, x):
    """Stand-ins for the GPU's buffers on a machine without one: every launched
    node's float64 result rounded to f32 (fused-away nodes have none)."""
    bufs = {-1: np.asarray(x, np.float32)}
    for i, p in enumerate(plan):
        if p["skip"]:
            continue
        d = node_pre(nodes, blob, plan, i, bufs)
        bufs[i] = act64(d["y"], d["act"], d["alpha"]).astype(np.float32)
    return bufs
