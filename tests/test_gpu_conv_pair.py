"""The 3x3 32 -> 64 and 3x3 64 -> 64 split-bf16 convs in one launch
(conv_x3_pair, aa_conv_pair.h) against the two conv_x3 launches it replaces.

The pair recomputes the first layer on each 12 x 8 tile's halo and hands it to
the second through LDS; every accumulator sums the same products in the same
order as the two kernels do, so stage k + 1's stored activations and the
logits must equal the unfused path's (AA_X3_PAIR=0 at create time) bit for
bit.  A wrong halo pixel, swizzle slot or clamped edge shows in single words.

Network: conv 3x3 1 -> 32, conv 3x3 32 -> 64 (stage 1), conv 3x3 64 -> 64
(stage 2), GlobalMaxPool; 3 windows.  Shapes, as stage 2's output against the
12 x 8 tile:
  one_tile       12 x 8    exactly one tile
  two_tiles_rem  25 x 17   two tiles and a remainder of 1 each way
  odd            13 x 11   a second tile row of 1 row, a second column of 3
  single         1 x 1     one pixel: every other intermediate pixel is clamped
Which path ran is read from the stage timers: the pair is timed under stage 2
and stage 1 then reports no launch.
"""
import numpy as np
import pytest
import torch

from tools.make_models import calibration_input, make_chain

pytestmark = pytest.mark.gpu

SHAPES = {"one_tile": (12, 8), "two_tiles_rem": (25, 17), "odd": (13, 11), "single": (1, 1)}
NAMES = ["conv_small_3x3_1_32", "conv_3x3_32_64", "conv_3x3_64_64", "globalmax_64_64"]


def _blocks(C):
    return [(32, (3, 3), None), (C, (3, 3), None), (C, (3, 3), None)]


def _run(path, x, monkeypatch, pair):
    """(stage 2 read-out, logits, launches of stages 1 and 2 in one forward)"""
    from aa_amd.model import Model
    if pair:
        monkeypatch.delenv("AA_X3_PAIR", raising=False)
    else:
        monkeypatch.setenv("AA_X3_PAIR", "0")
    m = Model(path, x.shape[1:], precision="bf16x3")
    xt = torch.from_numpy(x).cuda()
    m.set_timing(True)
    lg = m.forward(xt)[0]
    torch.cuda.synchronize()
    m.set_timing(False)
    counts = (m.stage_time(1)[1], m.stage_time(2)[1])
    act = m.forward_prefix(xt, 2)
    first = m.forward_prefix(xt, 1)  # a prefix ending at stage 1 runs its own kernel either way
    names = [m.stage_info(i)[0] for i in range(m.n_stages())]
    return act.cpu().numpy(), lg.cpu().numpy(), counts, first.cpu().numpy(), names


@pytest.mark.parametrize("shape", list(SHAPES))
def test_pair_equals_the_two_launches(gpu, tmp_path, monkeypatch, shape):
    hb, wb = SHAPES[shape]
    H, W = hb + 6, wb + 6
    path = make_chain(tmp_path / "m", _blocks(64), seed=31, n_mels=H, T=W)
    x = calibration_input(3, H, W, True, np.random.default_rng(H * 131 + W))
    act0, lg0, cnt0, first0, names0 = _run(path, x, monkeypatch, pair=False)
    act1, lg1, cnt1, first1, names1 = _run(path, x, monkeypatch, pair=True)
    assert names0 == NAMES and names1 == NAMES
    assert cnt0 == (1, 1), f"AA_X3_PAIR=0 must keep both launches: {cnt0}"
    assert cnt1 == (0, 1), f"the pair runs under stage 2 and stage 1 reports no launch: {cnt1}"
    assert act0.shape == (3, hb, wb, 64) and np.isfinite(act0).all()
    nd = int((act0.view(np.uint32) != act1.view(np.uint32)).sum())
    print(f"{shape}: {nd} of {act0.size} stage-2 words differ, "
          f"{int((lg0.view(np.uint32) != lg1.view(np.uint32)).sum())} of {lg0.size} logit words")
    assert nd == 0
    assert np.array_equal(lg0.view(np.uint32), lg1.view(np.uint32))
    assert np.array_equal(first0.view(np.uint32), first1.view(np.uint32))


def test_other_widths_plan_unfused(gpu, tmp_path, monkeypatch):
    H, W = 12 + 6, 8 + 6
    path = make_chain(tmp_path / "m", _blocks(72), seed=31, n_mels=H, T=W)
    x = calibration_input(3, H, W, True, np.random.default_rng(7))
    _, lg0, cnt0, _, names0 = _run(path, x, monkeypatch, pair=False)
    _, lg1, cnt1, _, names1 = _run(path, x, monkeypatch, pair=True)
    assert names0 == names1
    assert cnt0 == (1, 1) and cnt1 == (1, 1)
    assert np.array_equal(lg0.view(np.uint32), lg1.view(np.uint32))
