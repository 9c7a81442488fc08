"""The split-bf16 fused first conv's per-lane image (aa_model_first_lane_image,
no GPU): what pack_first_lanes uploads equals the kernel's lane formulas,
restated here in numpy from their description in aa_conv_x3.h, for all 64
lanes.

A lane of a wave computes the first layer (3x3, 1 -> 32) with two
v_mfma_f32_32x32x16_bf16.  MFMA row m = lane & 31 is first-layer channel
16 ((m >> 2) & 1) + 4 (m >> 3) + (m & 3); kg = lane >> 5 is the k-group.
MFMA 1's operand holds bf16 hi of taps 0..7 in both k-groups; MFMA 2's holds
bf16 lo of taps 0..7 (kg 0) or hi(w8), hi(w8), lo(w8), 0 x 5 (kg 1); the 16
accumulator start values are the biases of channels 16 kg .. 16 kg + 15.
hi rounds to nearest even, lo is the bf16 of the exact f32 remainder.
Two weight sets: seeded weights under a folded BatchNorm, and planted values
whose hi rounding carries (1 + 2^-8 + 2^-9), ties, and a zero.
"""
import ctypes as C

import numpy as np
import pytest

from aa_amd import _lib
from test_cnn_plan import Net, PRECS, image, layer_table


def bf16_bits(x):
    """f32 array -> bf16 bit patterns (uint16), round to nearest even."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_val(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def split(x):
    hi = bf16_bits(x)
    return hi, bf16_bits(np.asarray(x, np.float32) - bf16_val(hi))


def restated(w, b):
    """w [32][9], b [32] (folded, f32) -> the image's bytes."""
    hi, lo = split(w)
    img = np.zeros((6, 64, 16), np.uint8)
    for lane in range(64):
        m, kg = lane & 31, lane >> 5
        ch = 16 * ((m >> 2) & 1) + 4 * (m >> 3) + (m & 3)
        wa = hi[ch, :8]
        wal = lo[ch, :8] if kg == 0 else np.array([hi[ch, 8], hi[ch, 8], lo[ch, 8], 0, 0, 0, 0, 0], np.uint16)
        img[0, lane] = wa.view(np.uint8)
        img[1, lane] = wal.view(np.uint8)
        img[2:6, lane] = np.ascontiguousarray(b[16 * kg:16 * kg + 16], np.float32).view(np.uint8).reshape(4, 16)
    return img.reshape(-1)


def plant(k):
    """[3][3][1][32]: channel 5's taps, tap 8 included (the k-group 1 slots)."""
    c = 2.0 ** -8 + 2.0 ** -9
    k[:, :, 0, 5] = np.array([1 + c, -(1 + c), 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 0.0, 2.0 ** -20, 255.0 + 0.75,
                              1 + 2.0 ** -8 + 2.0 ** -20, 3 * (1 + c)], np.float32).reshape(3, 3)
    k[2, 2, 0, 17] = 1 + c


def nets():
    a = Net(11, (160, 226, 1))
    a.conv(32, 3, 3)
    b = Net(12, (31, 50, 1))
    b.conv(32, 3, 3, bias=True, bn=False, act=0.1, edit=plant)
    for n in (a, b):
        n.conv(32, 3, 3, pool=(3, 3))
        n.conv(7, 1, 1, bias=True, bn=False, act=None)
        n.layer("globalmaxpool2d")
        n.layer("sigmoid")
    return {"seeded_bn": a, "planted": b}


def lane_image(L, h):
    n = C.c_size_t()
    assert L.aa_model_first_lane_image(h, None, 0, C.byref(n)) == 0
    buf = np.zeros(n.value, np.uint8)
    if n.value:
        assert L.aa_model_first_lane_image(h, buf.ctypes.data, buf.size, C.byref(n)) == 0
    return buf


def planned(net, prec):
    L = _lib.lib()
    h = C.c_void_p()
    blob = net.blob()
    H, W, Cin = net.in_shape
    assert L.aa_model_plan(layer_table(net), len(net.layers), blob.ctypes.data, blob.size, H, W, Cin, PRECS[prec],
                           C.byref(h)) == 0, L.aa_last_error()
    return L, h


@pytest.mark.parametrize("name", sorted(nets()))
def test_lane_image_equals_the_lane_formulas(name):
    net = nets()[name]
    L, h = planned(net, "bf16x3")
    w = image(L, h, 0, 0).view(np.float32).reshape(32, 9)  # the folded first conv, [channel][tap]
    b = image(L, h, 0, 1).view(np.float32)[:32]
    if name == "planted":  # no BatchNorm: the folded weights are the planted values
        k = net.chunks[0].reshape(3, 3, 1, 32)
        assert np.array_equal(w, k.reshape(9, 32).T)
        hi, lo = split(w[5])
        assert hi[0] == 0x3F81 and bf16_val(lo[:1])[0] < 0  # 1 + 2^-8 + 2^-9 carries to 1 + 2^-7
        assert hi[2] == 0x3F80 and hi[3] == 0x3F82  # ties to even
    got = lane_image(L, h)
    assert got.size == 6 * 64 * 16
    want = restated(w, b)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} bytes differ, first at part {bad[0] // 1024}, lane {bad[0] % 1024 // 16}, byte {bad[0] % 16}"
    small = np.zeros(8, np.uint8)
    n = C.c_size_t()
    assert L.aa_model_first_lane_image(h, small.ctypes.data, 8, C.byref(n)) == _lib.AA_ERR_INVALID and n.value == 6144
    assert L.aa_model_destroy(h) == 0


@pytest.mark.parametrize("prec", ["f32", "bf16", "fp8"])
def test_no_lane_image_outside_split_bf16(prec):
    L, h = planned(nets()["seeded_bn"], prec)
    assert lane_image(L, h).size == 0
    assert L.aa_model_destroy(h) == 0
