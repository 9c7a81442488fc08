"""The CNN planner on the CPU (aa_model_plan / aa_model_stage_image, no GPU).

* Every field of the plan -- stage names, flops, bytes, shapes or refusal
  codes, workspace sizes, and byte length + SHA-256 of every weight, bias and
  tail image -- equals what the commit named in tests/golden/cnn_plan_parent.json
  computed for the same layer tables and blobs (recorded there from its
  aa_model_create, with the upload writing its bytes to files instead of the
  device); every rejection returns that commit's code and aa_last_error text.
* Two layouts are stated independently in numpy, from their descriptions in
  aa_conv_x3.h / DESIGN.md (split-bf16 steps) and aa_cnn.hip (fp8 K = 128
  super-steps), not from the packers.
"""
import ctypes as C
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from aa_amd import _lib

GOLDEN = Path(__file__).resolve().parent / "golden" / "cnn_plan_parent.json"
PRECS = {"f32": _lib.AA_PREC_F32, "bf16": _lib.AA_PREC_BF16, "fp8": _lib.AA_PREC_FP8, "bf16x3": _lib.AA_PREC_BF16X3}
OP = _lib.AA_OP


class Net:
    """A layer table and its weight blob, from a seeded generator."""

    def __init__(self, seed, in_shape, cin=None):
        self.rng = np.random.default_rng(seed)
        self.in_shape = in_shape
        self.c = in_shape[2] if cin is None else cin
        self.layers, self.chunks, self.n = [], [], 0

    def put(self, a):
        a = np.ascontiguousarray(a, np.float32).ravel()
        off, self.n = self.n, self.n + a.size
        self.chunks.append(a)
        return off

    def layer(self, op, kh=0, kw=0, filters=0, alpha=0.0, eps=0.0, off=()):
        self.layers.append(dict(op=OP[op], kh=kh, kw=kw, filters=filters, alpha=alpha, eps=eps,
                                off=list(off) + [-1] * (4 - len(off))))
        return self.layers[-1]

    def conv(self, cout, kh, kw, bias=False, bn=True, act=0.3, pool=None, edit=None):
        k = (self.rng.standard_normal((kh, kw, self.c, cout)) * np.sqrt(2.0 / (kh * kw * self.c))).astype(np.float32)
        if edit:
            edit(k)
        off = [self.put(k)]
        if bias:
            off.append(self.put(self.rng.normal(0, 0.2, cout)))
        self.layer("conv2d", kh, kw, cout, off=off)
        if bn:
            self.layer("batchnorm", eps=1e-3,
                       off=[self.put(self.rng.uniform(0.7, 1.3, cout)), self.put(self.rng.normal(0, 0.2, cout)),
                            self.put(self.rng.normal(0, 0.1, cout)), self.put(self.rng.uniform(0.5, 1.5, cout))])
        if act is not None:
            self.layer("leakyrelu", alpha=act)
        if pool:
            self.layer("maxpool2d", pool[0], pool[1])
        self.c = cout
        return k

    def dense(self, units, bias=True):
        off = [self.put(self.rng.standard_normal((self.c, units)) / np.sqrt(self.c))]
        if bias:
            off.append(self.put(self.rng.normal(0, 0.2, units)))
        self.layer("dense", filters=units, off=off)
        self.c = units

    def blob(self):
        return np.concatenate(self.chunks) if self.chunks else np.zeros(1, np.float32)


def plant_edges(k):
    """Head kernel [1][1][256][labels] (no BatchNorm: folded weight = the value
    itself).  Label 0 all zero (fp8 scale 1).  Label 1: amax 240, so the fp8
    scale is 1 and the values meet f2fp8 as they are -- e4m3 ties 1.0625 (->
    1.0, even) and 1.1875 (-> 1.25), 2^-10 + 2^-11 in the subnormal range (a
    tie between 1 and 2 steps of 2^-9), 2^-11 (a tie with zero); bf16 ties
    1 + 2^-8 (-> 1.0) and 1 + 3 * 2^-8 (-> 1 + 2^-6), and 1 + 2^-8 + 2^-20 just
    above one.  Label 2: 1000.0, above 448, sets the scale (0.24), under which
    the channel's ordinary weights fall into the e4m3 subnormal range."""
    k[0, 0, :, 0] = 0.0
    k[0, 0, :, 1] *= 0.5
    k[0, 0, :9, 1] = [240.0, 1.0625, 1.1875, 2.0 ** -10 + 2.0 ** -11, 2.0 ** -11, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8,
                      1 + 2.0 ** -8 + 2.0 ** -20, -(1 + 2.0 ** -8)]
    k[0, 0, 17, 2] = 1000.0


def chain(seed, labels=24, last=256, mag=False):
    """The model1 architecture (tools/make_models.py) at 160 x 226."""
    n = Net(seed, (160, 226, 1))
    if mag:
        n.layer("magtransform", off=[n.put([0.3])])
    n.conv(32, 3, 3)
    n.conv(32, 3, 3, pool=(3, 3))
    n.conv(64, 3, 3)
    n.conv(64, 3, 3)
    n.conv(128, 9, 3, pool=(3, 3))
    n.conv(last, 1, 3)
    n.conv(labels, 1, 1, bias=True, bn=False, act=None, edit=plant_edges if last == 256 else None)
    n.layer("globalmaxpool2d")
    n.layer("sigmoid")
    return n


def chain_5x5(seed):
    """A 5x5 conv at C_in 32 with a 2x2 pool: no tuned tile (ST_GCONV with a
    pooled scratch in bf16x3, ST_GENERIC in f32 / bf16, refused in fp8)."""
    n = Net(seed, (40, 50, 1))
    n.conv(32, 3, 3)
    n.conv(48, 5, 5, pool=(2, 2))
    n.conv(10, 1, 1, bias=True, bn=False, act=None)
    n.layer("globalmaxpool2d")
    n.layer("sigmoid")
    return n


def pooldense(seed, dense):
    n = Net(seed, (30, 40, 1))
    n.layer("magtransform", off=[n.put([-0.7])])
    n.conv(32, 3, 3, bias=True, act=None)
    n.layer("relu")
    n.layer("globalmaxpool2d")
    if dense:
        n.dense(7)
    n.layer("sigmoid")
    return n


def cases():
    # labels37_last250: the odd width makes the 1x3 conv's cout_pad round up and
    # leaves the 1x1 conv (C_in 250) to the generic / runtime-shaped kernels;
    # labels37: the conv_head path with cout_pad rounding, no tail (> 32 labels)
    return {"model1": chain(11), "labels37_last250": chain(12, labels=37, last=250),
            "labels37": chain(16, labels=37, mag=True), "conv5x5_pool2": chain_5x5(13),
            "mag_pool_dense": pooldense(14, True), "mag_pool_nodense": pooldense(15, False)}


def rejections():
    """name -> (Net, precision): every way aa_model_create refuses a model."""
    out = {}

    def small(seed=20, shape=(20, 24, 1)):
        n = Net(seed, shape)
        n.conv(32, 3, 3, bias=True)
        return n

    def head(n):
        n.conv(5, 1, 1, bias=True, bn=False, act=None)
        n.layer("globalmaxpool2d")
        n.layer("sigmoid")
        return n

    # offsets outside the blob, one operand at a time (conv kernel, conv bias,
    # the four BatchNorm vectors, dense kernel, dense bias, MagTransform's a)
    for name, li, oi in [("off_conv_kernel", 0, 0), ("off_conv_bias", 0, 1), ("off_bn_gamma", 1, 0), ("off_bn_beta", 1, 1),
                         ("off_bn_mean", 1, 2), ("off_bn_var", 1, 3)]:
        for how in ("past", "neg"):
            if how == "neg" and (li, oi) == (0, 1):
                continue  # a negative bias offset means "no bias"
            n = head(small())
            n.layers[li]["off"][oi] = n.n - 3 if how == "past" else -5
            out[f"{name}_{how}"] = (n, "bf16x3")
    for name, oi in [("off_dense_kernel", 0), ("off_dense_bias", 1)]:
        n = small()
        n.layer("globalmaxpool2d")
        n.dense(6)
        n.layers[-1]["off"][oi] = n.n - 2
        out[name] = (n, "f32")
    n = Net(21, (20, 24, 1))
    n.layer("magtransform", off=[10 ** 6])
    n.conv(32, 3, 3)
    out["off_mag"] = (head(n), "f32")
    n = small()
    n.layer("magtransform", off=[n.put([0.1])])
    out["mag_after_conv"] = (head(n), "bf16")
    n = Net(22, (20, 24, 1))
    n.conv(32, 3, 3, act=-0.1)
    out["negative_slope"] = (head(n), "bf16x3")
    n = head(small())
    n.layer("sigmoid")
    out["layers_after_head"] = (n, "bf16x3")
    n = small()
    n.layer("globalmaxpool2d")
    n.dense(6)
    n.layer("sigmoid")
    n.layer("relu")
    out["layers_after_dense"] = (n, "f32")
    out["fp8_untuned"] = (chain_5x5(13), "fp8")
    n = small()
    n.conv(32, 3, 3)
    out["no_global_pool"] = (n, "bf16")
    out["input_smaller_than_kernel"] = (head(small(shape=(2, 24, 1))), "f32")
    n = Net(23, (8, 9, 1))
    n.conv(32, 3, 3, pool=(7, 2))
    out["pool_larger_than_output"] = (head(n), "bf16x3")
    n = Net(24, (8, 9, 1))
    n.conv(32, 3, 3, pool=(0, 2))
    out["pool_window_zero"] = (head(n), "f32")
    n = Net(25, (20, 24, 1))
    n.layer("batchnorm", eps=1e-3, off=[0, 0, 0, 0])
    n.put(np.ones(4))
    out["expected_conv"] = (n, "f32")
    n = Net(26, (20, 24, 1))
    n.layer("globalmaxpool2d")
    n.put(np.ones(4))
    out["global_pool_first"] = (n, "f32")
    return out


def layer_table(net):
    arr = (_lib.Layer * len(net.layers))()
    for a, d in zip(arr, net.layers):
        a.op, a.kh, a.kw, a.filters, a.alpha, a.eps = d["op"], d["kh"], d["kw"], d["filters"], d["alpha"], d["eps"]
        for i in range(4):
            a.off[i] = d["off"][i]
    return arr


def image(L, h, stage, which):
    n = C.c_size_t()
    assert L.aa_model_stage_image(h, stage, which, None, 0, C.byref(n)) == 0
    buf = np.zeros(n.value, np.uint8)
    assert L.aa_model_stage_image(h, stage, which, buf.ctypes.data, buf.size, C.byref(n)) == 0
    return buf


def describe(L, create, net, prec, images):
    """What one plan (or creation) of `net` yields, as plain JSON values.
    images(handle, stage) -> three byte arrays."""
    blob = net.blob()
    h = C.c_void_p()
    H, W, Cin = net.in_shape
    rc = create(layer_table(net), len(net.layers), blob.ctypes.data, blob.size, H, W, Cin, PRECS[prec], C.byref(h))
    if rc != 0:
        return {"rc": rc, "error": L.aa_last_error().decode()}
    out = {"rc": 0, "n_outputs": L.aa_model_n_outputs(h), "workspace_1": L.aa_model_workspace_bytes(h, 1),
           "workspace_3": L.aa_model_workspace_bytes(h, 3), "stages": []}
    for s in range(L.aa_model_n_stages(h)):
        name = C.create_string_buffer(128)
        fl, by = C.c_double(), C.c_double()
        assert L.aa_model_stage_info(h, s, name, 128, C.byref(fl), C.byref(by)) == 0
        sh = [C.c_int32(), C.c_int32(), C.c_int32()]
        src = L.aa_model_stage_shape(h, s, *map(C.byref, sh))
        out["stages"].append({"name": name.value.decode(), "flops": fl.value, "bytes": by.value,
                              "shape": [v.value for v in sh] if src == 0 else {"rc": src},
                              "images": [[int(b.size), hashlib.sha256(b.tobytes()).hexdigest()] for b in images(h, s)]})
    L.aa_model_destroy(h)
    return out


def plan(net, prec):
    L = _lib.lib()
    return describe(L, L.aa_model_plan, net, prec, lambda h, s: [image(L, h, s, w) for w in range(3)])


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


@pytest.mark.parametrize("prec", sorted(PRECS))
@pytest.mark.parametrize("case", sorted(cases()))
def test_plan_equals_parent(golden, case, prec):
    want = golden["cases"][case][prec]
    got = plan(cases()[case], prec)
    if want["rc"] == 0:
        assert got["rc"] == 0, got
        for k in ("n_outputs", "workspace_1", "workspace_3"):
            assert got[k] == want[k], k
        assert [s["name"] for s in got["stages"]] == [s["name"] for s in want["stages"]]
        for g, w in zip(got["stages"], want["stages"]):
            assert g == w, g["name"]
    assert got == want


def test_cases_cover_every_kernel_family(golden):
    """The fixture exercises what it is meant to (read from the parent's record)."""
    names = lambda c, p: [s["name"] for s in golden["cases"][c][p]["stages"]]
    m = names("model1", "bf16x3")
    assert m[1].startswith("conv_small_3x3_1_32+conv_3x3_32_32_pool3") and m[-1].startswith("conv_1x3_128_256+head_1x1_256_24")
    assert golden["cases"]["model1"]["bf16x3"]["stages"][-1]["images"][2][0] == 8 * 2 * 2 * 64 * 8 * 2  # the tail image
    assert "conv_1x3_128_250" in names("labels37_last250", "bf16x3")
    assert names("labels37", "bf16x3")[-2:] == ["conv_1x3_128_256", "head_1x1_256_37"]
    assert any(n.startswith("conv_gx3_5x5_32_48_pool2") for n in names("conv5x5_pool2", "bf16x3"))
    assert any(n.startswith("conv_generic_5x5_32_48_pool2") for n in names("conv5x5_pool2", "f32"))
    assert golden["cases"]["conv5x5_pool2"]["fp8"]["rc"] == _lib.AA_ERR_UNSUPPORTED
    assert names("mag_pool_dense", "f32")[-1] == "globalmax_dense_32_7"
    assert golden["cases"]["mag_pool_nodense"]["f32"]["stages"][-1]["images"][0][0] == 0  # null weight image
    assert len(golden["rejections"]) == len(rejections()) + 2


@pytest.mark.parametrize("name", sorted(rejections()))
def test_rejection_equals_parent(golden, name):
    net, prec = rejections()[name]
    want = golden["rejections"][name]
    assert want["rc"] != 0
    assert plan(net, prec) == want


def test_null_and_precision_rejections(golden):
    L = _lib.lib()
    h = C.c_void_p()
    assert L.aa_model_plan(None, 0, None, 0, 1, 1, 1, 0, C.byref(h)) == golden["rejections"]["null_argument"]["rc"]
    assert L.aa_last_error().decode() == golden["rejections"]["null_argument"]["error"]
    net = pooldense(14, True)
    blob = net.blob()
    rc = L.aa_model_plan(layer_table(net), len(net.layers), blob.ctypes.data, blob.size, 30, 40, 1, 9, C.byref(h))
    assert {"rc": rc, "error": L.aa_last_error().decode()} == golden["rejections"]["bad_precision"]


def test_planned_model_refuses_to_run():
    L = _lib.lib()
    net = pooldense(14, True)
    blob = net.blob()
    h = C.c_void_p()
    assert L.aa_model_plan(layer_table(net), len(net.layers), blob.ctypes.data, blob.size, 30, 40, 1, 0, C.byref(h)) == 0
    x = np.zeros(4, np.float32)
    assert L.aa_model_forward(h, x.ctypes.data, 1, x.ctypes.data, None, x.ctypes.data, 1 << 30, None) == _lib.AA_ERR_INVALID
    assert b"aa_model_plan" in L.aa_last_error()
    assert L.aa_model_forward_prefix(h, x.ctypes.data, 1, 0, x.ctypes.data, x.ctypes.data, 1 << 30, None) == _lib.AA_ERR_INVALID
    assert L.aa_model_set_input_f16(h, 0) == _lib.AA_ERR_INVALID
    n = C.c_size_t()
    small = np.zeros(8, np.uint8)
    assert L.aa_model_stage_image(h, 0, 0, small.ctypes.data, 8, C.byref(n)) == _lib.AA_ERR_INVALID and n.value == 32 * 9 * 4
    assert L.aa_model_stage_image(h, 0, 3, None, 0, C.byref(n)) == _lib.AA_ERR_INVALID
    assert L.aa_model_stage_image(h, 9, 0, None, 0, C.byref(n)) == _lib.AA_ERR_INVALID
    assert L.aa_model_destroy(h) == 0


# ---- layouts stated independently --------------------------------------------
def layout_net():
    """conv 3x3 1->32, conv 3x3 32->64 pool 3, then a 3x3 conv at C_in 64 with 3
    output channels and no BatchNorm (folded weight = the kernel value)."""
    n = Net(31, (30, 40, 1))
    n.conv(32, 3, 3)
    n.conv(64, 3, 3, pool=(3, 3))
    k = n.conv(3, 3, 3, bn=False)
    n.layer("globalmaxpool2d")
    return n, k


def plan_images(net, prec, stage):
    L = _lib.lib()
    blob = net.blob()
    h = C.c_void_p()
    H, W, Cin = net.in_shape
    assert L.aa_model_plan(layer_table(net), len(net.layers), blob.ctypes.data, blob.size, H, W, Cin, PRECS[prec],
                           C.byref(h)) == 0
    out = [image(L, h, stage, w) for w in range(3)]
    L.aa_model_destroy(h)
    return out


def rn_bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).float().numpy()


def test_x3_layout_from_its_description():
    """aa_conv_x3.h: steps (32-channel group g, tap t) in order g * ntap + t,
    each [cout_pad] rows of 8 units of 8 bf16; units 0-3 hi = rn_bf16(w) of
    channels 32 g + 8 u .. + 7, units 4-7 lo = rn_bf16(w - hi); unit u of row o
    in slot (u + o) & 7.  (The tuned C_in 64 shape has 9 taps, not 2.)"""
    net, k = layout_net()
    w_img = plan_images(net, "bf16x3", 2)[0].view(np.uint16)
    ntap, cin, cout, cout_pad = 9, 64, 3, 64
    assert w_img.size == 2 * ntap * cout_pad * cin + 1024
    rows = w_img[:2 * ntap * cout_pad * cin].reshape(cin // 32 * ntap * cout_pad, 8, 8)
    as_f32 = lambda u16: (u16.astype(np.uint32) << 16).view(np.float32)
    kt = k.reshape(ntap, cin, cout)
    used = np.zeros(rows.shape, bool)
    for g in range(cin // 32):
        for t in range(ntap):
            for o in range(cout):
                r = (g * ntap + t) * cout_pad + o
                for u in range(4):
                    w = kt[t, 32 * g + 8 * u:32 * g + 8 * u + 8, o]
                    hi = rn_bf16(w)
                    assert (as_f32(rows[r, (u + o) & 7]) == hi).all()
                    assert (as_f32(rows[r, (u + 4 + o) & 7]) == rn_bf16(w - hi)).all()
                    used[r, (u + o) & 7] = used[r, (u + 4 + o) & 7] = True
    assert not rows[~used].any() and not w_img[2 * ntap * cout_pad * cin:].any()  # padding rows and slack are zero


def test_fp8_k128_layout_from_its_description():
    """aa_cnn.hip (conv_mfma, fp8 at C_in >= 64): chunk k = tap * C_in/32 +
    channel chunk lies at byte 32 (k % 4) of row (k / 4) * cout_pad + o, rows of
    4 x 32 B + 16 B pad; values quantised at 240 / amax per output channel, the
    inverse scale after the cout_pad biases."""
    net, k = layout_net()
    w_img, b_img, _ = plan_images(net, "fp8", 2)
    ntap, cin, cout, cout_pad, bstr = 9, 64, 3, 64, 144
    nch = ntap * cin // 32
    nss = (nch + 3) // 4
    assert w_img.size == nss * cout_pad * bstr + 1024
    rows = w_img[:nss * cout_pad * bstr].reshape(nss * cout_pad, bstr)
    kt = k.reshape(ntap, cin, cout)
    scales = b_img.view(np.float32)[cout_pad:]
    used = np.zeros(rows.shape, bool)
    for o in range(cout):
        amax = np.abs(kt[:, :, o]).max()
        sc = np.float32(240.0) / amax
        assert scales[o] == np.float32(1.0) / sc
        for kk in range(nch):
            t, cc = divmod(kk, cin // 32)
            q = torch.from_numpy(kt[t, 32 * cc:32 * cc + 32, o] * sc).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
            r = (kk // 4) * cout_pad + o
            assert (rows[r, 32 * (kk % 4):32 * (kk % 4) + 32] == q).all()
            used[r, 32 * (kk % 4):32 * (kk % 4) + 32] = True
    assert (scales[cout:] == 1.0).all()
    assert not rows[~used].any() and not w_img[nss * cout_pad * bstr:].any()
