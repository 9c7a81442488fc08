"""CPU fp32 oracle for the window classifier CNN.  TEST INFRASTRUCTURE ONLY.

Reference call site: ``model.predict(np.array(d))`` at
src/identify_tracks.py:544 (Keras / TF 2.19 on CPU), input ``[W, n_mels, T, C]``
(NHWC, produced by ``get_spect`` :267), output ``[W, n_labels]``.  The real
Cacophony weights/architecture are a Docker-time download (Dockerfile:33-37)
and TF is not installed, so the model family is defined by this build
 and stored as ``audioModel.safetensors`` whose
``__metadata__["arch"]`` is a Keras-style layer list.  This oracle evaluates
that layer list literally, un-fused, in torch-CPU float32 (or float64):

* ``magtransform``  -> ``x ** sigmoid(a)``   src/magtransform.py:17-19,
  src/magtransformv2.py:19-21
* ``conv2d``        -> Keras Conv2D, padding="valid", stride 1, HWIO kernel
* ``batchnorm``     -> inference BN with moving statistics (not folded)
* ``leakyrelu``     -> max(x, alpha*x)
* ``maxpool2d``     -> Keras MaxPooling2D(pool), strides = pool, valid (floor)
* ``globalmaxpool2d`` -> max over H, W
* ``relu``          -> max(x, 0)
* ``dense``         -> Keras Dense after the global pooling (x @ kernel + bias)
* ``activation``    -> sigmoid

``logits`` are the GlobalMaxPool outputs before the final sigmoid.
"""
from __future__ import annotations

import json

import numpy as np
import torch
import torch.nn.functional as F
from safetensors.numpy import load_file
from safetensors import safe_open


def load_arch(path):
    with safe_open(str(path), framework="np") as f:
        meta = f.metadata()
    return json.loads(meta["arch"]), load_file(str(path))


_GRAPH_TYPES = {"depthwise_conv2d", "add", "multiply", "globalavgpool2d", "avgpool2d", "zeropad2d", "rescaling",
                "normalization", "reshape", "flatten", "dropout"}


def _is_graph(arch):
    for ly in arch:
        if "inputs" in ly or ly["type"] in _GRAPH_TYPES or ly.get("padding", "valid") != "valid":
            return True
        if ly["type"] == "conv2d" and (list(ly.get("strides", [1, 1])) != [1, 1] or
                                       ly.get("activation") not in (None, "linear")):
            return True
        if ly["type"] == "maxpool2d" and list(ly.get("strides") or ly["pool"]) != list(ly["pool"]):
            return True
        if ly["type"] == "activation" and ly.get("fn") != "sigmoid":
            return True
    return False


def _tf_same(n, k, s):
    """TF "same" padding: (before, after), the odd pixel after."""
    out = -(-n // s)
    total = max((out - 1) * s + k - n, 0)
    return total // 2, total - total // 2


def _act(x, fn, alpha=0.2):
    fn = None if fn is None else str(fn).lower()
    if fn in (None, "linear"):
        return x
    if fn == "relu":
        return F.relu(x)
    if fn == "sigmoid":
        return torch.sigmoid(x)
    if fn in ("swish", "silu"):
        return x * torch.sigmoid(x)
    if fn in ("leaky_relu", "leaky"):
        return F.leaky_relu(x, alpha)
    raise ValueError(f"activation {fn}")


@torch.no_grad()
def _forward_graph(arch, tensors, x, dtype, capture=None):
    """Keras Functional semantics, literally (NCHW torch, un-fused): each entry
    reads the layers named in "inputs" (default: the previous entry; "input":
    the model input).  logits: the last layer's input to a final sigmoid."""
    t = lambda k: torch.from_numpy(np.asarray(tensors[k])).to(dtype)
    outs = {"input": x}
    prev = "input"
    logits = None
    for i, ly in enumerate(arch):
        kind = ly["type"]
        name = ly.get("name") or f"_l{i}"
        ins = [outs[s] for s in (ly.get("inputs") or [prev])]
        h = ins[0]
        if kind in ("conv2d", "depthwise_conv2d", "maxpool2d", "avgpool2d"):
            k = list(ly["kernel"] if kind != "maxpool2d" and kind != "avgpool2d" else ly["pool"])
            s = list(ly.get("strides") or ([1, 1] if kind.endswith("conv2d") else k))
            if ly.get("padding", "valid") == "same":
                pt, pb = _tf_same(h.shape[2], k[0], s[0])
                pl, pr = _tf_same(h.shape[3], k[1], s[1])
            else:
                pt = pb = pl = pr = 0
            if kind == "conv2d":
                w = t(name + ".kernel").reshape(k[0], k[1], h.shape[1], -1).permute(3, 2, 0, 1)
                b = t(name + ".bias") if ly.get("use_bias", True) else None
                y = F.conv2d(F.pad(h, (pl, pr, pt, pb)), w, b, stride=s)
                y = _act(y, ly.get("activation"))
            elif kind == "depthwise_conv2d":
                C = h.shape[1]
                w = t(name + ".kernel").reshape(k[0], k[1], C).permute(2, 0, 1)[:, None]
                b = t(name + ".bias") if ly.get("use_bias", True) else None
                y = F.conv2d(F.pad(h, (pl, pr, pt, pb)), w, b, stride=s, groups=C)
                y = _act(y, ly.get("activation"))
            elif kind == "maxpool2d":
                y = F.max_pool2d(F.pad(h, (pl, pr, pt, pb), value=-float("inf")), k, s)
            else:  # TF AvgPool: the mean over the taps inside the image
                ones = torch.ones_like(h[:, :1])
                num = F.avg_pool2d(F.pad(h, (pl, pr, pt, pb)), k, s, divisor_override=1)
                den = F.avg_pool2d(F.pad(ones, (pl, pr, pt, pb)), k, s, divisor_override=1)
                y = num / den
        elif kind == "zeropad2d":
            (a, b_), (l_, r_) = ly["pad"]
            y = F.pad(h, (l_, r_, a, b_))
        elif kind == "batchnorm":
            g, be = t(name + ".gamma"), t(name + ".beta")
            mu, var = t(name + ".moving_mean"), t(name + ".moving_variance")
            y = (h - mu[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + float(ly.get("eps", 1e-3)))
            y = y * g[None, :, None, None] + be[None, :, None, None]
        elif kind == "activation":
            if ly["fn"] == "sigmoid" and i == len(arch) - 1:
                logits = h
            y = _act(h, ly["fn"])
        elif kind == "relu":
            y = F.relu(h)
        elif kind == "leakyrelu":
            y = F.leaky_relu(h, float(ly.get("alpha", 0.3)))
        elif kind in ("globalavgpool2d", "globalmaxpool2d"):
            y = (h.mean(dim=(2, 3)) if kind == "globalavgpool2d" else torch.amax(h, dim=(2, 3)))[:, :, None, None]
        elif kind == "add":
            y = ins[0] + ins[1]
        elif kind == "multiply":
            y = ins[0] * ins[1]
        elif kind == "rescaling":
            y = h * float(ly.get("scale", 1.0)) + float(ly.get("offset", 0.0))
        elif kind == "normalization":
            mean = t(name + ".mean").reshape(1, -1, 1, 1)
            var = t(name + ".variance").reshape(1, -1, 1, 1)
            y = (h - mean) / torch.clamp(torch.sqrt(var), min=1e-7)
        elif kind in ("reshape", "flatten", "dropout"):
            y = h
        elif kind == "magtransform":
            y = torch.pow(h, torch.sigmoid(t(name + ".a").reshape(-1)[0]))
        elif kind == "dense":
            flat = h.permute(0, 2, 3, 1).reshape(h.shape[0], -1)  # Keras Flatten of NHWC
            y = flat @ t(name + ".kernel").reshape(flat.shape[1], -1)
            if ly.get("use_bias", True):
                y = y + t(name + ".bias")
            if ly.get("activation") == "sigmoid" and i == len(arch) - 1:
                logits = y
            y = _act(y, ly.get("activation"))
            y = y[:, :, None, None]
        else:
            raise ValueError(f"unknown layer type {kind}")
        outs[name] = y
        prev = name
    if capture is not None:
        capture.update(outs)
    out = outs[prev].reshape(x.shape[0], -1) if outs[prev].dim() == 4 and outs[prev].shape[2:] == (1, 1) else \
        outs[prev].permute(0, 2, 3, 1).reshape(x.shape[0], -1)
    lg = out if logits is None else (logits.reshape(x.shape[0], -1) if logits.dim() == 2 else
                                     logits.permute(0, 2, 3, 1).reshape(x.shape[0], -1))
    return lg.cpu().numpy(), out.cpu().numpy()


@torch.no_grad()
def forward(path_or_arch, x_nhwc: np.ndarray, dtype=torch.float32, tensors=None):
    """Run the CNN on ``x_nhwc`` [W, H, T, C]; returns (logits, probs) numpy."""
    if tensors is None:
        arch, tensors = load_arch(path_or_arch)
    else:
        arch = path_or_arch
    if _is_graph(arch):
        x = torch.from_numpy(np.ascontiguousarray(x_nhwc)).to(dtype).permute(0, 3, 1, 2)
        return _forward_graph(arch, tensors, x, dtype)
    t = lambda k: torch.from_numpy(np.asarray(tensors[k])).to(dtype)
    x = torch.from_numpy(np.ascontiguousarray(x_nhwc)).to(dtype).permute(0, 3, 1, 2)
    logits = None
    for layer in arch:
        kind = layer["type"]
        name = layer.get("name")
        if kind == "magtransform":
            a = t(name + ".a").reshape(-1)[0]
            x = torch.pow(x, torch.sigmoid(a))
        elif kind == "conv2d":
            w = t(name + ".kernel").permute(3, 2, 0, 1)  # HWIO -> OIHW
            b = t(name + ".bias") if layer.get("use_bias", False) else None
            x = F.conv2d(x, w, b)
        elif kind == "batchnorm":
            g, be = t(name + ".gamma"), t(name + ".beta")
            mu, var = t(name + ".moving_mean"), t(name + ".moving_variance")
            eps = float(layer.get("eps", 1e-3))
            x = (x - mu[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + eps)
            x = x * g[None, :, None, None] + be[None, :, None, None]
        elif kind == "leakyrelu":
            x = F.leaky_relu(x, float(layer.get("alpha", 0.3)))
        elif kind == "relu":
            x = F.relu(x)
        elif kind == "dense":  # Keras Dense after the global pooling: x @ kernel + bias
            x = x @ t(name + ".kernel")
            if layer.get("use_bias", True):
                x = x + t(name + ".bias")
            logits = x
        elif kind == "maxpool2d":
            ph, pw = layer["pool"]
            x = F.max_pool2d(x, (ph, pw), (ph, pw))
        elif kind == "globalmaxpool2d":
            x = torch.amax(x, dim=(2, 3))
            logits = x
        elif kind == "activation":
            assert layer["fn"] == "sigmoid"
            x = torch.sigmoid(x)
        else:
            raise ValueError(f"unknown layer type {kind}")
    if logits is None:
        logits = x
    return logits.cpu().numpy(), x.cpu().numpy()


def _fp8(x):
    """Round to OCP e4m3fn (nearest even, saturated to +-448), back to f32."""
    return x.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).to(torch.float32)


# fp8 MFMA accumulation (gfx950, measured by tools/mfma_fp8_precision.hip,
# profiles/r03/fp8_mfma_precision.txt): v_mfma_f32_16x16x32_fp8_fp8 and the
# K = 128 f8f6f4 form sum each group of 8 products (one lane's 8 bytes of a
# 32-deep chunk: 8 consecutive input channels of one tap) after truncating
# every product toward zero to a multiple of 2^(E - 13), E the largest sum of
# operand exponents (ea + eb) in the group; one instruction adds its groups to
# the f32 accumulator and rounds.
MFMA_FP8_WIN = 13


def _fp8_mfma_conv(x: torch.Tensor, wq: torch.Tensor, k128: bool, lchunk: int = 256) -> torch.Tensor:
    """Valid conv of e4m3 activations x [N, C, H, W] with e4m3 weights wq
    [O, C, kh, kw] (scaled), summed the way conv_mfma / conv_head do on the
    fp8 MFMAs: chunk k = tap * C/32 + channel chunk, one instruction per chunk
    (C = 32) or per four chunks (C >= 64, K = 128; the last padded), groups of
    8 channels truncated as above, f32 rounding after every instruction.
    Returns the f32 accumulator [N, O, Ho, Wo]."""
    N, C, H, W = x.shape
    O, _, kh, kw = wq.shape
    assert C % 32 == 0
    taps, cpc = kh * kw, C // 32
    nch = taps * cpc
    per = 4 if k128 else 1
    nst = -(-nch // per)
    Ho, Wo = H - kh + 1, W - kw + 1
    L = Ho * Wo
    # e4m3 x e4m3 products, their truncation to a power-of-two grid and a
    # group's sum of 8 are exact in f32; chunks and steps are summed in f64
    cols = F.unfold(x.float(), (kh, kw)).view(N, C, taps, L).permute(0, 3, 2, 1)  # [N, L, taps, C]
    xc = cols.reshape(N, L, nch, 4, 8)  # chunk k = t * cpc + cc, group g = channels 8g..8g+7
    wc = wq.float().view(O, C, taps).permute(0, 2, 1).reshape(O, nch, 4, 8).contiguous()
    def e4m3_exp(v):  # unbiased exponent field of e4m3 values (subnormal / zero: -6)
        return torch.clamp(torch.frexp(v).exponent - 1, min=-6).to(torch.int32)

    ex, ew = e4m3_exp(xc), e4m3_exp(wc)
    out = torch.empty(N, L, O, dtype=torch.float32)
    for n in range(N):
        for l0 in range(0, L, lchunk):
            p = xc[n, l0:l0 + lchunk, None] * wc[None]  # [l, O, nch, 4, 8]
            # grid 2^(max over the group of (ea + eb) - WIN): the operands' e4m3
            # exponents (subnormals and zero at the minimum, -6), not the
            # product's own (1.5 x 1.5 = 2.25 keeps the finer grid)
            es = (ex[n, l0:l0 + lchunk, None] + ew[None]).amax(-1, keepdim=True)
            inv = torch.ldexp(torch.ones_like(p[..., :1]), MFMA_FP8_WIN - es)
            p.mul_(inv).trunc_().div_(inv)
            cs = p.sum(-1).double().sum(-1)  # [l, O, nch]: one chunk's groups
            if per > 1:
                cs = F.pad(cs, (0, nst * per - nch)).view(cs.shape[0], O, nst, per).sum(-1)
            acc = torch.zeros(cs.shape[:2], dtype=torch.float32)
            for st in range(nst):
                acc = (acc.double() + cs[..., st]).float()
            out[n, l0:l0 + lchunk] = acc
    return out.permute(0, 2, 1).reshape(N, O, Ho, Wo)


@torch.no_grad()
def forward_fp8_emulated(path, x_nhwc: np.ndarray, first_bf16=True, mfma=True):
    """CPU emulation of libaa's AA_PREC_FP8 numerics (the checker of that mode,
    not a reference result): BN folded into the conv (per output channel), a
    C_in = 1 first conv with bf16 weights on the f32 input (first_bf16: the
    fused first layer; False: f32 weights, the stand-alone conv_small), every
    later conv's folded weights quantised per output channel to e4m3fn with
    the largest |w| at 240 and dequantised after the f32 accumulation,
    pre-pool values rounded to bf16 (the epilogue tile), every stored
    activation rounded to e4m3fn.  mfma: the convs summed as the fp8 MFMAs
    sum (_fp8_mfma_conv: per 8-product group truncation, f32 rounding per
    instruction) with the epilogue's single-rounding fmaf; False: torch's f32
    conv.  A 1x1 conv followed by GlobalMaxPool2D is
    the head kernel (max of the f32 values); any other conv followed by it
    stores e4m3fn activations that the global max then reads.  Returns
    (logits, probs)."""
    arch, tensors = load_arch(path)
    t = lambda k: torch.from_numpy(np.asarray(tensors[k])).to(torch.float64)
    x = torch.from_numpy(np.ascontiguousarray(x_nhwc)).to(torch.float32).permute(0, 3, 1, 2)
    i, logits = 0, None
    while i < len(arch):
        layer = arch[i]
        kind, name = layer["type"], layer.get("name")
        if kind == "magtransform":
            x = torch.pow(x, torch.sigmoid(t(name + ".a").reshape(-1)[0].float()))
            i += 1
            continue
        assert kind == "conv2d", kind
        w = t(name + ".kernel").permute(3, 2, 0, 1)  # OIHW
        cout = w.shape[0]
        b = t(name + ".bias") if layer.get("use_bias", False) else torch.zeros(cout, dtype=torch.float64)
        i += 1
        if i < len(arch) and arch[i]["type"] == "batchnorm":
            bn, nm = arch[i], arch[i]["name"]
            sc = t(nm + ".gamma") / torch.sqrt(t(nm + ".moving_variance") + float(bn.get("eps", 1e-3)))
            b = (b - t(nm + ".moving_mean")) * sc + t(nm + ".beta")
            w = w * sc[:, None, None, None]
            i += 1
        w, b = w.float(), b.float()
        first = w.shape[1] == 1
        if first and first_bf16:
            # the fused first layer: bf16 weights times the input as bf16 hi + lo
            xh = x.to(torch.bfloat16).float()
            y = F.conv2d(xh + (x - xh).to(torch.bfloat16).float(), w.to(torch.bfloat16).float(), b)
        elif first:
            y = F.conv2d(x, w, b)
        else:
            amax = w.abs().amax(dim=(1, 2, 3))
            s = torch.where(amax > 0, 240.0 / amax, torch.ones_like(amax))
            wq = _fp8(w * s[:, None, None, None])
            if mfma:  # the fp8 MFMAs' own summation, then the epilogue's fmaf(acc, 1/s, bias)
                acc = _fp8_mfma_conv(x, wq, k128=w.shape[1] >= 64)
                y = (acc.double() * (1.0 / s).double()[None, :, None, None] + b.double()[None, :, None, None]).float()
            else:
                y = F.conv2d(x, wq) * (1.0 / s)[None, :, None, None] + b[None, :, None, None]
        act, pool, head = None, None, False
        while i < len(arch) and arch[i]["type"] in ("leakyrelu", "maxpool2d", "globalmaxpool2d", "activation"):
            k = arch[i]["type"]
            if k == "leakyrelu":
                act = float(arch[i].get("alpha", 0.3))
            elif k == "maxpool2d":
                pool = tuple(arch[i]["pool"])
            elif k == "globalmaxpool2d":
                head = True
            i += 1
        if head and w.shape[2:] == (1, 1):
            logits = torch.amax(y, dim=(2, 3))
            if act is not None:
                logits = F.leaky_relu(logits, act)
            x = torch.sigmoid(logits)
            break
        if not first:
            y = y.to(torch.bfloat16).float()
        if pool is not None:
            y = F.max_pool2d(y, pool, pool)
        if act is not None:
            y = F.leaky_relu(y, act)
        x = _fp8(y)
        if head:  # GlobalMaxPool2D over the stored e4m3fn activations
            logits = torch.amax(x, dim=(2, 3))
            if i < len(arch) and arch[i]["type"] == "activation":
                i += 1
            x = torch.sigmoid(logits)
            break
    return logits.numpy(), x.numpy()


def ensemble_track_mean(probs_per_model):
    """np.mean over models then over windows (src/identify_tracks.py:548-551)."""
    p = np.mean(probs_per_model, axis=0)
    return np.mean(p, axis=0)


# ---------------------------------------------------------------------------
# One stage at a time: float64 reference + derived bound + interval rule
# (DESIGN.md "Per-stage checks").  A stage is what one kernel launch of
# aa_model_forward computes: one conv block (conv [BN] [act] [pool]), or the
# fused first pair (two blocks), read from the stage's ACTUAL input (the GPU's
# decoded output of the previous stored stage), so errors do not accumulate
# and a failure names one kernel.
# ---------------------------------------------------------------------------
U24 = 2.0 ** -24        # f32 unit roundoff
SPLIT_C = 2.0 ** -15    # split-bf16 direct kernels: 3 * 2^-18 per product (dropped lo.lo, bf16 rounding of lo), margin 2


def conv_blocks(arch):
    """The arch as conv blocks, one per libaa stage, in stage order:
    ([[conv, bn?, act?, pool?] layer dicts, ...], the layers after the last
    block).  Block k is stage k of aa_model_create's plan."""
    blocks, i = [], 0
    while i < len(arch) and arch[i]["type"] != "conv2d":
        if arch[i]["type"] == "magtransform":
            raise NotImplementedError("stage reference: MagTransform models")
        i += 1
    while i < len(arch) and arch[i]["type"] == "conv2d":
        blk = [arch[i]]
        i += 1
        for kind in ("batchnorm", ("leakyrelu", "relu"), "maxpool2d"):
            if i < len(arch) and arch[i]["type"] in (kind if isinstance(kind, tuple) else (kind,)):
                blk.append(arch[i])
                i += 1
        blocks.append(blk)
    return blocks, arch[i:]


def _fold_block(tensors, blk):
    """(w64 [O, I, kh, kw] with the BN scale folded in, shift64 [O], slope or
    None, pool or None) of one conv block, as aa_model_create folds it."""
    t = lambda k: torch.from_numpy(np.asarray(tensors[k])).double()
    conv = blk[0]
    w = t(conv["name"] + ".kernel").permute(3, 2, 0, 1)
    shift = t(conv["name"] + ".bias") if conv.get("use_bias", False) else torch.zeros(w.shape[0], dtype=torch.float64)
    slope, pool = None, None
    for ly in blk[1:]:
        if ly["type"] == "batchnorm":
            nm = ly["name"]
            sc = t(nm + ".gamma") / torch.sqrt(t(nm + ".moving_variance") + float(np.float32(ly.get("eps", 1e-3))))
            shift = (shift - t(nm + ".moving_mean")) * sc + t(nm + ".beta")
            w = w * sc[:, None, None, None]
        elif ly["type"] == "leakyrelu":
            slope = float(np.float32(ly.get("alpha", 0.3)))
        elif ly["type"] == "relu":
            slope = 0.0
        elif ly["type"] == "maxpool2d":
            pool = tuple(ly["pool"])
    return w, shift, slope, pool


def _bf16r(x):
    return x.float().to(torch.bfloat16).double()


def _split16(x):
    """hi + lo of an f32 value as the kernels form it (bf16 hi, bf16 lo of the
    exact remainder): what an OUT_SPLIT store keeps and a fused first layer reads."""
    x = x.float()
    hi = x.to(torch.bfloat16).float()
    return (hi + (x - hi).to(torch.bfloat16).float()).double()


def _fp8_quant(w32):
    """aa_model_create's e4m3fn weights: per output channel s = 240 / amax in
    f32, q = e4m3fn(w * s); (q, 1 / s) as f32 tensors."""
    amax = w32.abs().amax(dim=(1, 2, 3))
    s = torch.where(amax > 0, 240.0 / amax, torch.ones_like(amax))
    return _fp8(w32 * s[:, None, None, None]), 1.0 / s


def _act32(v, slope):
    if slope is None:
        return v
    return torch.where(v >= 0, v, v * np.float32(slope))


def stage_store(v64, slope, pool, storage, ebf16=False):
    """The kernels' epilogue after the accumulator, applied as they apply it
    (f32 arithmetic): [bf16 epilogue tile] -> max pool -> activation ->
    rounding to the storage type ("f32", "split": the grouped-split hi + lo,
    "bf16", "fp8").  Every step is monotone non-decreasing, so the chain maps
    an interval of pre-activation values to the interval of stored values.
    v64: [N, C, H, W] float64; returns float64."""
    v = v64.float()
    if ebf16:
        v = v.to(torch.bfloat16).float()
    if pool is not None and tuple(pool) != (1, 1):
        v = F.max_pool2d(v, pool, pool)
    v = _act32(v, slope)
    if storage == "split":
        return _split16(v)
    if storage == "bf16":
        v = v.to(torch.bfloat16).float()
    elif storage == "fp8":
        v = _fp8(v)
    else:
        assert storage == "f32", storage
    return v.double()


def _absconv(x, w, shift):
    return F.conv2d(x.abs(), w.abs()) + shift.abs()[None, :, None, None]


def _trunc_slack(xmag, wq, inv_s):
    """fp8 MFMA truncation: every product of a group of 8 loses < 2^(E - 13),
    2^E <= the group's largest max(|a|, 2^-6) * max(|b|, 2^-6), so a group
    loses < 2^-10 of the sum of those.  Upper bound of that loss per output."""
    lo = 2.0 ** -6
    return 2.0 ** -10 * F.conv2d(xmag.clamp(min=lo), wq.double().abs().clamp(min=lo)) * inv_s.double()[None, :, None, None]


def _stage_pre(tensors, stage_layers, x_in, precision, kernel="direct", c_wg=None):
    """(centre y, bound B) of the last block's accumulator + shift, float64
    [N, C, Hc, Wc], plus that block's (slope, pool)."""
    blocks, rest = conv_blocks(list(stage_layers))
    assert blocks and not rest and len(blocks) in (1, 2), "a stage is one conv block or the fused first pair"
    x = torch.from_numpy(np.ascontiguousarray(x_in)).double().permute(0, 3, 1, 2)
    col = lambda v: v[None, :, None, None]
    w, shift, slope, pool = _fold_block(tensors, blocks[-1])
    K = w.shape[1] * w.shape[2] * w.shape[3]
    if len(blocks) == 2:
        # fused first pair: a C_in = 1 3x3 conv and its activation, then the block above
        w1, s1, slope1, pool1 = _fold_block(tensors, blocks[0])
        assert w1.shape[1] == 1 and pool1 is None and (slope1 is None or 0.0 <= slope1 <= 1.0)
        K1 = w1.shape[2] * w1.shape[3]
        act = lambda v: v if slope1 is None else torch.where(v >= 0, v, v * slope1)
        if precision in ("f32", "bf16x3"):
            sp = SPLIT_C if precision == "bf16x3" else 0.0
            y1 = F.conv2d(x, w1) + col(s1)
            B1 = ((K1 + 8) * U24 + sp) * _absconv(x, w1, s1)
            h1 = act(y1)  # |act(a) - act(b)| <= |a - b| for a slope in [0, 1]
            y = F.conv2d(h1, w) + col(shift)
            A = _absconv(h1.abs() + B1, w, shift)
            B = F.conv2d(B1, w.abs()) + ((K + 8) * U24 + sp) * A
            return y, B, slope, pool
        # bf16 / fp8: bf16 weights on the input as bf16 hi + lo, f32 sums from
        # the bias, the activation, then bf16 / e4m3fn into the patch
        q = (lambda v: v.to(torch.bfloat16).float()) if precision == "bf16" else _fp8
        w1q, b1 = _bf16r(w1.float()), s1.float().double()
        x16 = _split16(x)
        y1 = F.conv2d(x16, w1q) + col(b1)
        B1 = (K1 + 8) * U24 * _absconv(x16, w1q, b1)
        h = [q(_act32(v.float(), slope1)).double() for v in (y1 - B1, y1, y1 + B1)]
        hmag = torch.maximum(h[0].abs(), h[2].abs())
        dh = h[2] - h[0]
        b2 = shift.float().double()
        if precision == "bf16":
            wq = _bf16r(w.float())
            y = F.conv2d(h[1], wq) + col(b2)
            B = F.conv2d(dh, wq.abs()) + (K + 8) * U24 * _absconv(hmag, wq, b2)
        else:
            wq, inv_s = _fp8_quant(w.float())
            acc = _fp8_mfma_conv(h[1].float(), wq, k128=False, lchunk=64)
            y = acc.double() * col(inv_s.double()) + col(b2)
            weff = wq.double() * inv_s.double()[:, None, None, None]
            # beyond the issue's |W2| (*) interval term: the centre is the TRUNCATING emulation on h[1],
            # and an intermediate one e4m3fn step away changes which product bits its groups truncate;
            # both runs lose < _trunc_slack, hence 2 x, and only where some intermediate is two-valued
            touched = (F.conv2d((dh != 0).double(), (wq != 0).double()) > 0).double()
            B = (F.conv2d(dh, weff.abs()) + 2.0 * _trunc_slack(hmag, wq, inv_s) * touched +
                 (K + 8) * U24 * _absconv(hmag, weff, b2))
        return y, B, slope, pool
    if w.shape[1] == 1 or precision == "f32" or precision == "bf16x3":
        # f32 arithmetic (conv_small in every mode), the f32 MFMA chain, or split-bf16
        y = F.conv2d(x, w) + col(shift)
        A = _absconv(x, w, shift)
        c = (K + 8) * U24
        if precision == "bf16x3" and w.shape[1] > 1:
            if kernel == "wg":
                assert c_wg is not None, "the Winograd constant comes from the emulation (winograd_constant)"
                c += c_wg
            else:
                c += SPLIT_C
        return y, c * A, slope, pool
    b = shift.float().double()
    if precision == "bf16":
        wq = _bf16r(w.float())
        y = F.conv2d(x, wq) + col(b)
        return y, (K + 8) * U24 * _absconv(x, wq, b), slope, pool
    assert precision == "fp8", precision
    wq, inv_s = _fp8_quant(w.float())
    acc = _fp8_mfma_conv(x.float(), wq, k128=w.shape[1] >= 64, lchunk=64)
    y = acc.double() * col(inv_s.double()) + col(b)
    weff = wq.double() * inv_s.double()[:, None, None, None]
    return y, (K + 8) * U24 * _absconv(x, weff, b), slope, pool


def _storage(precision, out_split):
    return "split" if out_split else {"f32": "f32", "bf16x3": "f32", "bf16": "bf16", "fp8": "fp8"}[precision]


def _pooled(y, B, slope, pool):
    if pool is not None and tuple(pool) != (1, 1):
        y, B = F.max_pool2d(y, pool, pool), F.max_pool2d(B, pool, pool)
    if slope is not None:
        y = torch.where(y >= 0, y, y * slope)
        B = B * max(1.0, slope)
    return y.permute(0, 2, 3, 1).numpy(), B.permute(0, 2, 3, 1).numpy()


@torch.no_grad()
def stage_reference(arch, tensors, stage_layers, x_in, precision, kernel="direct", c_wg=None):
    """(r, B), float64 NHWC at the stage's output shape.  r: the stage's
    layers in float64 on x_in (bf16 / fp8: with the weights as
    aa_model_create stores them; fp8: summed as the MFMAs sum, the project's
    emulation).  B: how far correct arithmetic of that precision may sit from
    r, per element: the pre-activation bound (see _stage_pre / DESIGN.md)
    taken through the max pool (the largest of the window) and the
    activation (slope <= 1 keeps it).  ``arch`` is not needed (the stage's
    layers carry their names); kept for call sites that pass it."""
    return _pooled(*_stage_pre(tensors, stage_layers, x_in, precision, kernel, c_wg))


@torch.no_grad()
def stage_check(tensors, stage_layers, x_in, precision, kernel="direct", c_wg=None, ebf16=False, out_split=False):
    """One evaluation of the stage for the interval rule: dict of float64 NHWC
    arrays r, B (stage_reference), lo = store(y - B), hi = store(y + B) and
    mid = store(y), `store` being the stage's own epilogue chain
    (stage_store).  A stored element g is correct iff lo <= g <= hi."""
    y, B, slope, pool = _stage_pre(tensors, stage_layers, x_in, precision, kernel, c_wg)
    # (conv_small, a stand-alone C_in = 1 first conv, has no epilogue tile)
    small = np.asarray(x_in).shape[-1] == 1 and len(conv_blocks(list(stage_layers))[0]) == 1
    st = _storage(precision, out_split)
    e = bool(ebf16) and precision in ("bf16", "fp8") and not small
    out = {k: stage_store(v, slope, pool, st, e).permute(0, 2, 3, 1).numpy()
           for k, v in (("lo", y - B), ("hi", y + B), ("mid", y))}
    out["r"], out["B"] = _pooled(y, B, slope, pool)
    return out


def stage_interval(arch, tensors, stage_layers, x_in, precision, kernel="direct", c_wg=None, ebf16=False,
                   out_split=False):
    """(lo, hi) of stage_check."""
    d = stage_check(tensors, stage_layers, x_in, precision, kernel, c_wg, ebf16, out_split)
    return d["lo"], d["hi"]


@torch.no_grad()
def head_interval(tensors, stage_layers, x_in, precision):
    """(lo, hi, r) of the logits [N, L] of a 1x1 head + global max, float64:
    stage_layers = [the head conv] (conv_head + head_final on the stored
    activations x_in), or [conv block, head conv] for split-bf16's fused tail
    (aa_conv_tail.h: the conv, bias, activation, hi / lo split and the head in
    one launch).  The bound goes through the 1x1 head like any conv and
    through the maximum over pixels, which is monotone."""
    blocks, rest = conv_blocks(list(stage_layers))
    assert not rest and len(blocks) in (1, 2)
    x = torch.from_numpy(np.ascontiguousarray(x_in)).double().permute(0, 3, 1, 2)
    col = lambda v: v[None, :, None, None]
    w, shift, slope, pool = _fold_block(tensors, blocks[-1])
    assert tuple(w.shape[2:]) == (1, 1) and pool is None
    K = w.shape[1]
    if len(blocks) == 2:
        assert precision == "bf16x3"
        y6, B6, s6, p6 = _stage_pre(tensors, blocks[0], x_in, "bf16x3")
        assert p6 is None
        h6 = y6 if s6 is None else torch.where(y6 >= 0, y6, y6 * s6)
        B6 = B6 * max(1.0, s6 or 0.0)
        y = F.conv2d(h6, w) + col(shift)
        B = F.conv2d(B6, w.abs()) + (SPLIT_C + (K + 8) * U24) * _absconv(h6.abs() + B6, w, shift)
    elif precision in ("f32", "bf16x3"):  # the exact-f32 MFMA on f32 activations
        y = F.conv2d(x, w) + col(shift)
        B = (K + 8) * U24 * _absconv(x, w, shift)
    elif precision == "bf16":
        wq, b = _bf16r(w.float()), shift.float().double()
        y = F.conv2d(x, wq) + col(b)
        B = (K + 8) * U24 * _absconv(x, wq, b)
    else:
        wq, inv_s = _fp8_quant(w.float())
        b = shift.float().double()
        y = _fp8_mfma_conv(x.float(), wq, k128=K >= 64).double() * col(inv_s.double()) + col(b)
        B = (K + 8) * U24 * _absconv(x, wq.double() * inv_s.double()[:, None, None, None], b)
    fin = lambda v: _act32(torch.amax(v, dim=(2, 3)).float(), slope).double().numpy()
    return fin(y - B), fin(y + B), fin(y)


def winograd_constant(tensors, stage_layers, x_in, wo, tables):
    """c_wg of a Winograd F(wo, 3) stage on these inputs: 4 x the largest
    |emulation - r| / A, the emulation being tools/wino_study.conv_wino (f32
    transforms, split-bf16 products) with the kernel's tables (A^T, G, B^T)."""
    from tools.wino_study import conv_wino
    blocks, _ = conv_blocks(list(stage_layers))
    w, shift, _, _ = _fold_block(tensors, blocks[-1])
    x = torch.from_numpy(np.ascontiguousarray(x_in)).double().permute(0, 3, 1, 2)
    r = F.conv2d(x, w) + shift[None, :, None, None]
    A = _absconv(x, w, shift)
    e = conv_wino(x, w, shift, wo, None, tables=tables)
    return 4.0 * float(((e - r).abs() / A).max())


def interval_violations(g, lo, hi):
    """Elements of g outside [lo, hi] (NaN and Inf outside any interval):
    (count, index of the worst one or None, its excess over the interval's
    half width, in half widths -- inf for a non-finite g)."""
    g, lo, hi = np.asarray(g, np.float64), np.asarray(lo), np.asarray(hi)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        ok = np.isfinite(g) & (g >= lo) & (g <= hi)
        out = np.maximum(lo - g, g - hi) / np.maximum((hi - lo) / 2, np.finfo(np.float64).tiny)
    out = np.where(np.isfinite(g), out, np.inf)
    out = np.where(ok, 0.0, out)
    n = int((~ok).sum())
    if not n:
        return 0, None, 0.0
    idx = np.unravel_index(int(np.argmax(out)), g.shape)
    return n, tuple(int(i) for i in idx), float(out[idx])
