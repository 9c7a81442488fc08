"""The 9x3 Winograd conv with its A fragments sliding in registers (conv_wg
SLIDE, aa_conv_wg.h), at the small shapes where the sliding can go wrong.

A wave's three fragments interleave the tile's 39 group-pixels (lane r of
fragment i: pixel 3 r + i) and move down the plane one lane per kernel row;
the lanes a shift leaves empty, and the plane rows clamped at the first read,
may reach padding pixels (p >= 39) only.  A wrong lane, a row entering late or
garbage reaching a stored pixel shows in single pixels, so the 9x3 stage's
activations are compared per pixel with a float64 reference under the
per-stage bound (test_gpu_cnn_stages.walk: every stored stage, the 9x3 one
among them, with oracle.cnn_oracle.stage_check's derived bound), and the
split-bf16 logits with the f32-precision model of the same weights at the
project's 1e-3 gate.

Network: conv 3x3 1 -> 32, conv 3x3 32 -> 64 (the cheap 64-channel producer),
conv 9x3 64 -> 128 with pool 3; 2 windows.  Shapes, as the 9x3 conv's output
before pooling against its 39 x 6 tile:
  one_tile        39 x 6   exactly one full tile
  short_bottom    43 x 6   a second tile row with 3 valid rows, one row cut by
                           the pool's floor (H_out * 3 = 42, not a multiple of 39)
  partial_group   39 x 11  a second tile column whose only column group has 3
                           valid columns (W_out * 3 = 9), the rest clamped
  both            82 x 15  2 full tile rows + 3 rows, 2 full columns + half a group
"""
import numpy as np
import pytest
import torch

from test_gpu_cnn_stages import walk
from test_stage_bounds import TILES
from tools.make_models import calibration_input, make_chain

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-3
BLOCKS = [(32, (3, 3), None), (64, (3, 3), None), (128, (9, 3), (3, 3))]
SHAPES = {"one_tile": (39, 6), "short_bottom": (43, 6), "partial_group": (39, 11), "both": (82, 15)}
NAMES = ["conv_small_3x3_1_32", "conv_3x3_32_64", "conv_9x3_64_128_pool3", "globalmax_128_128"]


def test_shapes_meet_the_tile():
    t = TILES[("bf16x3", 9, 3, 64, 3)]
    assert (t["TH"], t["TW"], t["WO"]) == (39, 6, 6)
    rel = {k: ((hc // 3 * 3) % t["TH"], (wc // 3 * 3) % t["TW"]) for k, (hc, wc) in SHAPES.items()}
    assert rel == {"one_tile": (0, 0), "short_bottom": (3, 0), "partial_group": (0, 3), "both": (3, 3)}
    assert SHAPES["one_tile"] == (t["TH"], t["TW"])


@pytest.mark.parametrize("shape", list(SHAPES))
def test_sliding_9x3_stage_and_logits(gpu, tmp_path, shape):
    from aa_amd.model import Model
    hc, wc = SHAPES[shape]
    H, W = hc + sum(k[0] - 1 for _, k, _ in BLOCKS), wc + sum(k[1] - 1 for _, k, _ in BLOCKS)
    path = make_chain(tmp_path / "m", BLOCKS, seed=23, n_mels=H, T=W)
    x = calibration_input(2, H, W, True, np.random.default_rng(H * 131 + W))
    tag = f"9x3 slide {shape} {H}x{W}"
    fails, ratios, lg = walk(path, x, "bf16x3", tag, NAMES)
    for k, v in ratios.items():
        print(f"bf16x3  {k}: {v:.3e}")
    assert any("conv_9x3_64_128_pool3 max |g - r| / B" in k for k in ratios), list(ratios)
    assert not fails, "\n".join(fails)
    ref = Model(path, x.shape[1:], precision="f32").forward(torch.from_numpy(x).cuda())[0].cpu().numpy()
    d = float(np.abs(lg - ref).max())
    print(f"bf16x3  {tag}: max |logit - f32 logit| = {d:.3e}")
    assert lg.shape == (2, 128) and d <= LOGIT_TOL
