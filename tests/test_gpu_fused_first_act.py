"""The fused first conv (split-bf16) over its activation and log-mel forms.

model1's first two layers (3x3 1 -> 32, 3x3 32 -> 32, 3x3 max pool) on 2
windows of 31 x 50: conv2's output is 27 x 46 and the pooled output 9 x 15
against the kernel's 12 x 21 tile -- three tile rows and three tile columns,
the last with a 3-row and a 4-column remainder.  The stage read-out is held to
the float64 stage reference with the bound of the per-stage tests
(test_gpu_cnn_stages.check_stage), for

* the first layer's activation as the kernel folds it to a slope: LeakyReLU
  alpha 0, 0.1 and 1, and ReLU (leaky_split2's max(x, a x));
* the log-mel stored as float32 and as float16 (two instantiations of the
  kernel: conv_x3's LM parameter);
* one model with MagTransform in front (the instantiations that carry powf).

MagTransform: the stage reference does not model it, so that case restates
the fused pair's bound of oracle.cnn_oracle._stage_pre on the float64 input
x ** e (e: sigmoid(a) rounded to f32, as aa_model_create computes it) with
one more term for the kernel's f32 powf, 4 ulp = 2^-21 relative on every
input element, carried through |w1| into the first layer's bound: the HIP math
API documents powf to 1 ulp (2 taken); the kernel's exponent is e itself, so
it adds nothing; the f32 rounding of the result is within the first ulp; and
the remaining 2 ulp are margin.  (The term is small beside the split's 2^-15.)
"""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cnn_oracle as co
from test_gpu_cnn_stages import Plan, check_stage
from tools import make_models as mm

pytestmark = pytest.mark.gpu

H, W, N = 31, 50, 2
ACTS = {"leaky0": {"type": "leakyrelu", "alpha": 0.0}, "leaky0.1": {"type": "leakyrelu", "alpha": 0.1},
        "leaky1": {"type": "leakyrelu", "alpha": 1.0}, "relu": {"type": "relu"}}


def _two_layers(out_dir, act, mag, seed):
    """conv 3x3 -> 32, BN, act, conv 3x3 -> 32, BN, act, max pool 3x3, global
    max: seeded weights, BN statistics calibrated on this geometry's inputs."""
    from safetensors.numpy import save_file
    arch = [{"type": "magtransform", "name": "mag", "version": 1}] if mag else []
    for i in (1, 2):
        arch += [{"type": "conv2d", "name": f"conv{i}", "filters": 32, "kernel": [3, 3], "use_bias": i == 2},
                 {"type": "batchnorm", "name": f"bn{i}", "eps": 1e-3}, dict(act)]
    arch += [{"type": "maxpool2d", "pool": [3, 3]}, {"type": "globalmaxpool2d"}]
    rng = np.random.default_rng(seed)
    tensors = mm._init_weights(arch, 1, rng)
    tensors = mm._calibrate(arch, tensors, mm.calibration_input(4, H, W, not mag, rng), rng)
    out_dir.mkdir(parents=True, exist_ok=True)
    save_file({k: np.ascontiguousarray(v) for k, v in tensors.items()}, str(out_dir / "audioModel.safetensors"),
              metadata={"arch": json.dumps(arch)})
    meta = dict(mm.DEFAULT_META)
    meta.update({"name": "two_layers", "labels": [f"c{i}" for i in range(32)], "db_scale": not mag})
    (out_dir / "metadata.txt").write_text(json.dumps(meta, indent=2))
    return out_dir / "audioModel.safetensors"


@pytest.mark.parametrize("logmel", ["f32", "f16"])
@pytest.mark.parametrize("act", list(ACTS))
def test_fused_first_activation_forms(gpu, tmp_path, act, logmel):
    from aa_amd.model import Model
    path = _two_layers(tmp_path / "m", ACTS[act], False, seed=31)
    arch, tensors = co.load_arch(path)
    plan = Plan(arch, "bf16x3")
    assert plan.fused and plan.stored == [1]
    x = mm.calibration_input(N, H, W, True, np.random.default_rng(3150))
    if logmel == "f16":
        x = x.astype(np.float16).astype(np.float32)  # the values the kernel reads
    m = Model(path, (H, W, 1), precision="bf16x3")
    assert [m.stage_info(i)[0] for i in range(m.n_stages())] == plan.names()
    xt = torch.from_numpy(x).cuda()
    g = m.forward_prefix(xt.half() if logmel == "f16" else xt, 1).cpu().numpy()
    assert g.shape == (N, 9, 15, 32)
    ratios = {}
    msg = check_stage(plan, tensors, 1, x, g.astype(np.float64), f"{act} {logmel}-logmel {H}x{W}", ratios)
    for k, v in ratios.items():
        print(f"{k}: {v:.3e}")
    assert msg is None, msg
    # both signs reach the first layer's activation (else the slope is untested)
    w1, s1, _, _ = co._fold_block(tensors, plan.blocks[0])
    y1 = F.conv2d(torch.from_numpy(x).double().permute(0, 3, 1, 2), w1) + s1[None, :, None, None]
    assert 0.1 < float((y1 < 0).double().mean()) < 0.9


def test_fused_first_magtransform(gpu, tmp_path):
    from aa_amd.model import Model
    path = _two_layers(tmp_path / "m", ACTS["leaky0.1"], True, seed=37)
    arch, tensors = co.load_arch(path)
    assert arch[0]["type"] == "magtransform"
    blocks, _ = co.conv_blocks(arch[1:])
    x = mm.calibration_input(N, H, W, False, np.random.default_rng(3151))
    assert x.min() >= 9.9e-5 and x.max() <= 1.0
    m = Model(path, (H, W, 1), precision="bf16x3")
    names = [m.stage_info(i)[0] for i in range(m.n_stages())]
    assert names[1] == "conv_small_3x3_1_32+conv_3x3_32_32_pool3", names
    g = m.forward_prefix(torch.from_numpy(x).cuda(), 1).cpu().numpy().astype(np.float64)
    assert g.shape == (N, 9, 15, 32)

    a = np.float32(np.asarray(tensors["mag.a"]).reshape(-1)[0])
    e = np.float32(1.0) / (np.float32(1.0) + np.exp(-a, dtype=np.float32))  # aa_model_create: sigmoid in f32
    xm = torch.from_numpy(x.astype(np.float64) ** float(e)).permute(0, 3, 1, 2)
    col = lambda v: v[None, :, None, None]
    w1, s1, slope1, _ = co._fold_block(tensors, blocks[0])
    w2, s2, slope2, pool = co._fold_block(tensors, blocks[1])
    assert 0.0 <= slope1 <= 1.0 and pool == (3, 3)
    K1, K2 = 9, 9 * 32
    # oracle.cnn_oracle._stage_pre's fused pair (bf16x3), plus the powf term
    y1 = F.conv2d(xm, w1) + col(s1)
    B1 = ((K1 + 8) * co.U24 + co.SPLIT_C) * co._absconv(xm, w1, s1) + F.conv2d(2.0 ** -21 * xm, w1.abs())
    h1 = torch.where(y1 >= 0, y1, y1 * slope1)
    y = F.conv2d(h1, w2) + col(s2)
    B = F.conv2d(B1, w2.abs()) + ((K2 + 8) * co.U24 + co.SPLIT_C) * co._absconv(h1.abs() + B1, w2, s2)
    lo = co.stage_store(y - B, slope2, pool, "f32").permute(0, 2, 3, 1).numpy()
    hi = co.stage_store(y + B, slope2, pool, "f32").permute(0, 2, 3, 1).numpy()
    r, Bp = co._pooled(y, B, slope2, pool)
    print(f"magtransform e={float(e):.6f}: max |g - r| / B = {float(np.max(np.abs(g - r) / Bp)):.3e}")
    n, idx, ex = co.interval_violations(g, lo, hi)
    assert not n, f"{n} of {g.size} elements outside, worst {idx}: g={g[idx]!r} r={r[idx]!r} B={Bp[idx]:.3e} ({ex:.3g} half widths out)"
    assert 0.1 < float((y1 < 0).double().mean()) < 0.9
