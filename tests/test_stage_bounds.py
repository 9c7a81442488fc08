"""The per-stage checker checked on the CPU (oracle.cnn_oracle.stage_reference /
stage_interval, DESIGN.md "Per-stage checks"): the tests of
test_gpu_cnn_stages.py are only fair if correct arithmetic of each precision
passes the interval rule, and only useful if the rule catches the defects the
conv kernels can have.  Both are asserted here, not assumed:

* torch's f32 conv, the split-bf16 emulation (tools.wino_study.conv_split),
  the Winograd emulation (conv_wino on the tables parsed from aa_conv_wg.h),
  a bf16-input f32-accumulate conv and the fp8 MFMA-sum emulation with the
  other instruction grouping, each followed by the kernels' epilogue chain,
  satisfy their interval on every tuned layer shape;
* planted defects (a moved element, a shifted tile column, swapped channel
  groups, a dropped tap, a repeated Winograd group, NaN / Inf) fail it, and
  the report names the element;
* TILES, the tile table that sets the GPU test's geometries, equals the
  tables in the kernel sources.
"""
import re
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cnn_oracle as co
from test_winograd_tables import FORMS, _table
from tools.wino_study import conv_split, conv_wino

CSRC = Path(__file__).resolve().parents[1] / "audio-analysis_amd" / "csrc"

# (precision, kh, kw, C_in, pool) -> output tile TH x TW (before pooling),
# output channels per block BN, Winograd outputs per group WO (0: a direct
# kernel), bf16 epilogue tile EB.  bf16x3 rows are conv_x3's, except where a
# conv_wg row exists (aa_model_create prefers it).
TILES = {
    ("f32", 3, 3, 32, 3): dict(TH=6, TW=48, BN=32, WO=0, EB=False),
    ("f32", 3, 3, 32, 1): dict(TH=6, TW=24, BN=64, WO=0, EB=False),
    ("f32", 3, 3, 64, 1): dict(TH=6, TW=24, BN=64, WO=0, EB=False),
    ("f32", 9, 3, 64, 3): dict(TH=3, TW=33, BN=64, WO=0, EB=False),
    ("f32", 1, 3, 128, 1): dict(TH=6, TW=24, BN=32, WO=0, EB=False),
    ("bf16", 3, 3, 32, 3): dict(TH=18, TW=21, BN=32, WO=0, EB=True),
    ("bf16", 3, 3, 32, 1): dict(TH=8, TW=16, BN=64, WO=0, EB=True),
    ("bf16", 3, 3, 64, 1): dict(TH=8, TW=16, BN=64, WO=0, EB=True),
    ("bf16", 9, 3, 64, 3): dict(TH=39, TW=9, BN=128, WO=0, EB=True),
    ("bf16", 1, 3, 128, 1): dict(TH=7, TW=20, BN=128, WO=0, EB=False),
    ("fp8", 3, 3, 32, 3): dict(TH=12, TW=30, BN=32, WO=0, EB=True),
    ("fp8", 3, 3, 32, 1): dict(TH=8, TW=16, BN=64, WO=0, EB=True),
    ("fp8", 3, 3, 64, 1): dict(TH=12, TW=16, BN=64, WO=0, EB=True),
    ("fp8", 9, 3, 64, 3): dict(TH=21, TW=18, BN=128, WO=0, EB=True),
    ("fp8", 1, 3, 128, 1): dict(TH=7, TW=20, BN=128, WO=0, EB=True),
    ("bf16x3", 3, 3, 32, 3): dict(TH=12, TW=21, BN=32, WO=0, EB=False),
    ("bf16x3", 3, 3, 32, 1): dict(TH=10, TW=18, BN=64, WO=0, EB=False),
    ("bf16x3", 3, 3, 64, 1): dict(TH=12, TW=8, BN=64, WO=0, EB=False),
    ("bf16x3", 9, 3, 64, 3): dict(TH=39, TW=6, BN=64, WO=6, EB=False),
    ("bf16x3", 1, 3, 128, 1): dict(TH=7, TW=12, BN=64, WO=0, EB=False),
}
# the fused tail (split-bf16: the 1x3/128 -> 256 conv and the head in one launch)
TAIL_TILE = dict(TH=13, TW=5)


def _rows(macro, text):
    """Argument lists of the X(...) rows of the #define of `macro` that carries
    rows (not the A/B alias `#define M(X) M_ALT(X)`)."""
    m = re.search(rf"#define {macro}\(X\)((?:\s*\\\n)?\s*X\([^\n]*\n(?:\s*X\([^\n]*\n)*)", text)
    assert m, macro
    return [[a.strip() for a in r.split(",")] for r in re.findall(r"X\(([^)]*)\)", m.group(1))]


def tiles_from_sources():
    text = (CSRC / "aa_cnn_tiles.h").read_text()
    out = {}
    for r in _rows("AA_X3_CFGS", text):  # KH, KW, CIN, POOL, WM, WN, MF, NF, TH, TW, RING, AJIT, OCC
        kh, kw, cin, pool, wm, wn, mf, nf, th, tw = (int(v) for v in r[:10])
        out[("bf16x3", kh, kw, cin, pool)] = dict(TH=th, TW=tw, BN=wn * nf * 16, WO=0, EB=False)
    for r in _rows("AA_WG_CFGS", text):  # KH, CIN, POOL, WM, WN, MF, NF, TH, TW, OCC, WO, NPASS, BD
        kh, cin, pool, wm, wn, mf, nf, th, tw, occ, wo = (int(v) for v in r[:11])
        out[("bf16x3", kh, 3, cin, pool)] = dict(TH=th, TW=tw, BN=wn * nf * 16, WO=wo, EB=False)
    for r in _rows("AA_CONV_CFGS", text):  # T, KH, KW, CIN, POOL, WM, WN, MF, NF, TH, TW, EB, OCC
        prec = {"float": "f32", "bf16": "bf16", "fp8": "fp8"}[r[0]]
        kh, kw, cin, pool, wm, wn, mf, nf, th, tw = (int(v) for v in r[1:11])
        out[(prec, kh, kw, cin, pool)] = dict(TH=th, TW=tw, BN=wn * nf * 16, WO=0, EB={"true": True, "false": False}[r[11]])
    th = re.search(r"constexpr int TAIL_TH = (\d+), TAIL_TW = AA_TAIL_TW;", text)
    tw = re.search(r"#define AA_TAIL_TW (\d+)", text)
    assert th and tw
    return out, dict(TH=int(th.group(1)), TW=int(tw.group(1)))


def test_tile_table_matches_sources():
    tiles, tail = tiles_from_sources()
    assert len(tiles) == 20
    assert tiles == TILES
    assert tail == TAIL_TILE


def wg_tables(wo):
    bn, an, gn = FORMS[wo]
    a = wo + 2
    f = lambda t: np.array([[float(v) for v in row] for row in t])
    return f(_table(an, wo, a)), f(_table(gn, a, 3)), f(_table(bn, a, a))


# ---- one conv block on a stage input, as the GPU test meets it -------------
# (C_in, kh, kw, C_out, pool, input H x W): the tuned shapes, maps large enough
# for more than one Winograd group / tile column and a remainder
SHAPES = {
    "3x3_32": (32, 3, 3, 64, None, 9, 22),
    "3x3_32_pool": (32, 3, 3, 40, (3, 3), 13, 17),
    "3x3_64": (64, 3, 3, 64, None, 8, 22),
    "9x3_64_pool": (64, 9, 3, 72, (3, 3), 19, 19),
    "1x3_128": (128, 1, 3, 40, None, 5, 16),
}


def make_layer(cin, kh, kw, cout, pool, H, W, seed=0, n=2, storage="f32"):
    """(stage_layers, tensors, x_in NHWC float32) of one conv + BN + LeakyReLU
    [+ pool] block with He weights, on activations as a LeakyReLU leaves them,
    representable in `storage`."""
    rng = np.random.default_rng(seed)
    layers = [{"type": "conv2d", "name": "c", "filters": cout, "kernel": [kh, kw], "use_bias": False},
              {"type": "batchnorm", "name": "b", "eps": 1e-3}, {"type": "leakyrelu", "alpha": 0.3}]
    if pool:
        layers.append({"type": "maxpool2d", "pool": list(pool)})
    tensors = {"c.kernel": (rng.standard_normal((kh, kw, cin, cout)) * np.sqrt(2.0 / (kh * kw * cin))).astype(np.float32),
               "b.gamma": rng.uniform(0.7, 1.3, cout).astype(np.float32), "b.beta": rng.normal(0, 0.2, cout).astype(np.float32),
               "b.moving_mean": rng.normal(0, 0.1, cout).astype(np.float32),
               "b.moving_variance": rng.uniform(0.5, 1.5, cout).astype(np.float32)}
    x = rng.standard_normal((n, H, W, cin)).astype(np.float32)
    x = np.where(x >= 0, x, np.float32(0.3) * x)
    xt = torch.from_numpy(x)
    if storage == "bf16":
        xt = xt.to(torch.bfloat16).float()
    elif storage == "fp8":
        xt = co._fp8(xt)
    return layers, tensors, xt.numpy()


def _folded(tensors, layers):
    w, shift, slope, pool = co._fold_block(tensors, layers)
    return w.float(), shift.float(), slope, pool


def _nchw(x):
    return torch.from_numpy(x).permute(0, 3, 1, 2)


def _nhwc(v):
    return v.permute(0, 2, 3, 1).numpy()


def _assert_inside(g, lo, hi, what):
    n, idx, ex = co.interval_violations(g, lo, hi)
    assert n == 0, f"{what}: {n} elements outside, worst {idx} g={g[idx]!r} interval [{lo[idx]!r}, {hi[idx]!r}] excess {ex:.3g}"


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_f32_conv_passes_f32_rule(shape):
    layers, tensors, x = make_layer(*SHAPES[shape], seed=1)
    w, b, slope, pool = _folded(tensors, layers)
    g = _nhwc(co.stage_store((F.conv2d(_nchw(x), w) + b[None, :, None, None]).double(), slope, pool, "f32"))
    lo, hi = co.stage_interval(None, tensors, layers, x, "f32")
    _assert_inside(g, lo, hi, shape)
    r, B = co.stage_reference(None, tensors, layers, x, "f32")
    assert r.shape == g.shape and (np.abs(g - r) <= B).all()  # the rule reduces to |g - r| <= B
    print(f"{shape}: f32 max |g - r| / B = {(np.abs(g - r) / B).max():.3g}")


@pytest.mark.parametrize("out_split", [False, True])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_split_conv_passes_bf16x3_rule(shape, out_split):
    layers, tensors, x = make_layer(*SHAPES[shape], seed=2)
    w, b, slope, pool = _folded(tensors, layers)
    y = conv_split(_nchw(x), w, b)
    g = _nhwc(co.stage_store(y, slope, pool, "split" if out_split else "f32"))
    lo, hi = co.stage_interval(None, tensors, layers, x, "bf16x3", out_split=out_split)
    _assert_inside(g, lo, hi, shape)
    r, B = co.stage_reference(None, tensors, layers, x, "bf16x3")
    print(f"{shape}: split max |g - r| / B = {(np.abs(g - r) / B).max():.3g}")
    if not out_split:
        assert (np.abs(g - r) <= B).all()


def test_winograd_emulation_passes_wg_rule():
    """c_wg taken on one input holds for the emulation on another (the GPU
    test takes it on the very input it checks)."""
    wo = TILES[("bf16x3", 9, 3, 64, 3)]["WO"]
    tables = wg_tables(wo)
    layers, tensors, x0 = make_layer(*SHAPES["9x3_64_pool"], seed=3)
    c_wg = co.winograd_constant(tensors, layers, x0, wo, tables)
    print(f"F({wo},3) c_wg = {c_wg:.3e} (direct split-bf16: {co.SPLIT_C:.3e})")
    assert 0 < c_wg < 2.0 ** -10  # one dropped tap is worth ~ A / K = 2^-10.75 A at K = 1728
    _, _, x = make_layer(*SHAPES["9x3_64_pool"], seed=4)
    w, b, slope, pool = _folded(tensors, layers)
    y = conv_wino(_nchw(x).double(), w.double(), b.double(), wo, None, tables=tables)
    g = _nhwc(co.stage_store(y, slope, pool, "f32"))
    lo, hi = co.stage_interval(None, tensors, layers, x, "bf16x3", kernel="wg", c_wg=c_wg)
    _assert_inside(g, lo, hi, "9x3 F(6,3)")


@pytest.mark.parametrize("ebf16", [False, True])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_bf16_conv_passes_bf16_rule(shape, ebf16):
    layers, tensors, x = make_layer(*SHAPES[shape], seed=5, storage="bf16")
    w, b, slope, pool = _folded(tensors, layers)
    wq = w.to(torch.bfloat16).float()
    g = _nhwc(co.stage_store((F.conv2d(_nchw(x), wq) + b[None, :, None, None]).double(), slope, pool, "bf16", ebf16))
    lo, hi = co.stage_interval(None, tensors, layers, x, "bf16", ebf16=ebf16)
    _assert_inside(g, lo, hi, shape)
    # (where B is small against a bf16 step -- K (K + 8) 2^-24 A against 2^-8 |r| -- the interval holds
    # rn(r) alone, or rn(r) and its neighbour next to a rounding boundary)
    r = _nhwc(co.stage_store(co._stage_pre(tensors, layers, x, "bf16")[0], slope, pool, "bf16", ebf16))
    print(f"{shape}: bf16 elements differing from store(r): {(g != r).mean():.2e}, two-valued intervals {(lo != hi).mean():.2e}")


@pytest.mark.parametrize("shape", ["3x3_32", "3x3_64", "1x3_128"])
def test_fp8_emulation_passes_fp8_rule(shape):
    """The fp8 MFMA-sum emulation with the other instruction grouping (K = 32
    <-> K = 128: another f32 rounding order of the same truncated products)."""
    layers, tensors, x = make_layer(*SHAPES[shape], seed=6, storage="fp8", n=1)
    w, b, slope, pool = _folded(tensors, layers)
    wq, inv_s = co._fp8_quant(w)
    acc = co._fp8_mfma_conv(_nchw(x), wq, k128=not (w.shape[1] >= 64))
    y = acc.double() * inv_s.double()[None, :, None, None] + b.double()[None, :, None, None]
    g = _nhwc(co.stage_store(y, slope, pool, "fp8", True))
    lo, hi = co.stage_interval(None, tensors, layers, x, "fp8", ebf16=True)
    _assert_inside(g, lo, hi, shape)


# ---- the fused first pair ---------------------------------------------------
def make_fused(cout=40, H=17, W=19, seed=7, n=2):
    rng = np.random.default_rng(seed)
    l1, t1, _ = make_layer(1, 3, 3, 32, None, H, W, seed=seed)
    l2, t2, _ = make_layer(32, 3, 3, cout, (3, 3), H - 2, W - 2, seed=seed + 1)
    layers, tensors = [], {}
    for i, (ls, ts) in enumerate(((l1, t1), (l2, t2)), 1):
        for ly in ls:
            ly = dict(ly)
            if "name" in ly:
                ly["name"] += str(i)
            layers.append(ly)
        tensors.update({k.replace(".", f"{i}.", 1): v for k, v in ts.items()})
    # dB-like log-mel input; the first BN then sees inputs far from zero mean
    x = np.clip(rng.normal(-45, 12, (n, H, W, 1)), -80, 0).astype(np.float32)
    tensors["c1.kernel"] = (tensors["c1.kernel"] / 12).astype(np.float32)
    return layers, tensors, x


@pytest.mark.parametrize("precision", ["f32", "bf16x3", "bf16", "fp8"])
def test_fused_first_pair_passes_its_rule(precision):
    layers, tensors, x = make_fused()
    blocks, _ = co.conv_blocks(layers)
    w1, b1, s1, _ = _folded(tensors, blocks[0])
    w2, b2, s2, pool = _folded(tensors, blocks[1])
    col = lambda v: v[None, :, None, None]
    xt = _nchw(x)
    if precision == "f32":
        h1 = co._act32(F.conv2d(xt, w1) + col(b1), s1)
        y = (F.conv2d(h1, w2) + col(b2)).double()
    elif precision == "bf16x3":
        h1 = co._act32(conv_split(xt, w1, b1).float(), s1)
        y = conv_split(h1, w2, b2)
    else:
        q = (lambda v: v.to(torch.bfloat16).float()) if precision == "bf16" else co._fp8
        y1 = F.conv2d(co._split16(xt).float(), w1.to(torch.bfloat16).float()) + col(b1)
        h1 = q(co._act32(y1, s1))
        if precision == "bf16":
            y = (F.conv2d(h1, w2.to(torch.bfloat16).float()) + col(b2)).double()
        else:
            wq, inv_s = co._fp8_quant(w2)
            y = co._fp8_mfma_conv(h1, wq, k128=True).double() * col(inv_s.double()) + col(b2.double())
    eb = precision in ("bf16", "fp8")
    g = _nhwc(co.stage_store(y, s2, pool, co._storage(precision, False), eb))
    lo, hi = co.stage_interval(None, tensors, layers, x, precision, ebf16=eb)
    _assert_inside(g, lo, hi, f"fused {precision}")
    assert g.shape == (2, 4, 5, 40)


# ---- the rule bites ---------------------------------------------------------
@pytest.fixture(scope="module")
def passing():
    """A passing f32 array of the 3x3/64 layer and a passing Winograd array of
    the 9x3/64 layer (unpooled, so columns map to Winograd groups)."""
    layers, tensors, x = make_layer(*SHAPES["3x3_64"], seed=8)
    w, b, slope, pool = _folded(tensors, layers)
    g = _nhwc(co.stage_store((F.conv2d(_nchw(x), w) + b[None, :, None, None]).double(), slope, pool, "f32"))
    lo, hi = co.stage_interval(None, tensors, layers, x, "f32")
    r, B = co.stage_reference(None, tensors, layers, x, "f32")
    assert co.interval_violations(g, lo, hi)[0] == 0
    return dict(layers=layers, tensors=tensors, x=x, g=g, lo=lo, hi=hi, r=r, B=B, w=w, b=b, slope=slope)


def test_rule_catches_one_moved_element(passing):
    g = passing["g"].copy()
    at = (1, 3, 17, 41)
    g[at] += 4 * passing["B"][at]
    n, idx, _ = co.interval_violations(g, passing["lo"], passing["hi"])
    assert n == 1 and idx == at


def test_rule_catches_a_shifted_tile_column(passing):
    g = passing["g"].copy()
    g[:, :, 7, :] = passing["g"][:, :, 8, :]  # column 7, the last of an 8-wide tile, one pixel off
    n, idx, _ = co.interval_violations(g, passing["lo"], passing["hi"])
    assert n > 0.9 * g[:, :, 7, :].size and idx[2] == 7
    bad = ~((g >= passing["lo"]) & (g <= passing["hi"]))
    assert not np.delete(bad, 7, axis=2).any()


def test_rule_catches_swapped_channel_groups(passing):
    g = passing["g"].copy()
    g[0, 2, 5, :32], g[0, 2, 5, 32:64] = passing["g"][0, 2, 5, 32:64], passing["g"][0, 2, 5, :32]
    n, idx, _ = co.interval_violations(g, passing["lo"], passing["hi"])
    assert n > 50 and idx[:3] == (0, 2, 5)


def test_rule_catches_a_dropped_tap(passing):
    w = passing["w"].clone()
    w[13, :, 2, 0] = 0  # tap (kh 2, kw 0) of output channel 13
    g = _nhwc(co.stage_store((F.conv2d(_nchw(passing["x"]), w) + passing["b"][None, :, None, None]).double(),
                             passing["slope"], None, "f32"))
    n, idx, _ = co.interval_violations(g, passing["lo"], passing["hi"])
    assert n > 0.9 * g[..., 13].size and idx[3] == 13
    # even one input channel of one tap (one product of K = 576) is caught
    w = passing["w"].clone()
    w[13, 5, 2, 0] = 0
    g = _nhwc(co.stage_store((F.conv2d(_nchw(passing["x"]), w) + passing["b"][None, :, None, None]).double(),
                             passing["slope"], None, "f32"))
    n, idx, _ = co.interval_violations(g, passing["lo"], passing["hi"])
    assert n > 0.9 * g[..., 13].size and idx[3] == 13


def test_rule_catches_a_repeated_winograd_group():
    """The last 6-column group of a row holding its neighbour's values."""
    wo = 6
    tables = wg_tables(wo)
    cin, kh, kw, cout, _, H, W = SHAPES["9x3_64_pool"]
    layers, tensors, x = make_layer(cin, kh, kw, cout, None, H, W + 1, seed=9)  # Wc = 18: three groups
    c_wg = co.winograd_constant(tensors, layers, x, wo, tables)
    w, b, slope, _ = _folded(tensors, layers)
    y = conv_wino(_nchw(x).double(), w.double(), b.double(), wo, None, tables=tables)
    g = _nhwc(co.stage_store(y, slope, None, "f32"))
    lo, hi = co.stage_interval(None, tensors, layers, x, "bf16x3", kernel="wg", c_wg=c_wg)
    assert co.interval_violations(g, lo, hi)[0] == 0
    g[1, 4, 12:18, :] = g[1, 4, 6:12, :]
    n, idx, _ = co.interval_violations(g, lo, hi)
    assert n > 0.9 * 6 * cout and idx[:2] == (1, 4) and 12 <= idx[2] < 18


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_rule_fails_non_finite(passing, bad):
    g = passing["g"].copy()
    g[0, 0, 0, 0] = bad
    n, idx, ex = co.interval_violations(g, passing["lo"], passing["hi"])
    assert n == 1 and idx == (0, 0, 0, 0) and ex == np.inf


def test_smallest_defect_stays_above_every_bound():
    """A dropped tap is worth ~ A / K; the widest bound here is (2^-15 +
    (K + 8) 2^-24) A at K = 1728 (9x3/64)."""
    for cin, kh, kw in [(32, 3, 3), (64, 3, 3), (64, 9, 3), (128, 1, 3)]:
        K = cin * kh * kw
        assert (co.SPLIT_C + (K + 8) * co.U24) * K < 0.25
