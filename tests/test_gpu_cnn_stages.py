"""Every CNN stage's activations, per pixel, against a float64 reference of that
one stage (DESIGN.md "Per-stage checks").

The other CNN tests see the chain through its logits alone: a global maximum
over all pixels after the last stage.  Here Model.forward_prefix(x, k) reads
stage k's stored output g_k (decoded exactly to f32 NHWC), the reference
computes the stage's layers in float64 on the stage's actual input g_{k-1}
with a derived per-element bound B (oracle.cnn_oracle.stage_check), and an
element passes iff store(r - B) <= g <= store(r + B), `store` being the
kernel's own monotone epilogue chain.  A failure names the stage, the
precision, the element and its position in its tile.

Geometries come from the kernels' tile tables (test_stage_bounds.TILES,
asserted there against the sources): one tile, two tiles and a remainder, a
remainder the pool's floor cuts, less than a tile; C_out off the block width
(padded output channels); n = 3 windows (blockIdx.z > 0).
"""
import hashlib
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import cnn_oracle as co
from test_stage_bounds import TAIL_TILE, TILES, wg_tables
from tools.make_models import calibration_input, make_chain

pytestmark = pytest.mark.gpu

PRECISIONS = ["f32", "bf16x3", "bf16", "fp8"]
GOLDEN = Path(__file__).parent / "golden" / "model1_logits_t226.npz"

# the kernel under test is the last conv of its chain; the prefix supplies its C_in
P3 = (3, 3)
CASES = {
    "fused_first": (lambda C: [(32, (3, 3), None), (C, (3, 3), P3)], (32, 40)),
    "3x3_32": (lambda C: [(32, (3, 3), None), (C, (3, 3), None)], (64, 72)),
    "3x3_64": (lambda C: [(32, (3, 3), None), (64, (3, 3), None), (C, (3, 3), None)], (64, 72)),
    "9x3_64": (lambda C: [(32, (3, 3), None), (64, (3, 3), None), (C, (9, 3), P3)], (128, 72)),
    "1x3_128": (lambda C: [(32, (3, 3), None), (128, (3, 3), None), (C, (1, 3), None)], (256, 40)),
}
GEOMETRIES = ["one_tile", "two_tiles_rem", "pool_cut_rem", "sub_tile"]

# (case, C, precision) -> the reason aa_model_create gives (aa_last_error) for
# refusing it.  fp8 has no generic kernel, so a refusal there would be
# legitimate; every case above is served by a tuned kernel in all four modes.
REFUSED = {}


def _ids():
    out = []
    for case, (_, cs) in CASES.items():
        for C in cs:
            for prec in PRECISIONS:
                why = REFUSED.get((case, C, prec))
                out.append(pytest.param(case, C, prec, id=f"{case}-C{C}-{prec}" + (f"-refused[{why}]" if why else "")))
    return out


def conv_geometry(blocks, precision, geometry):
    """Input H x W such that the last conv's output (before pooling) has the
    named relation to that precision's tile."""
    f, (kh, kw), pool = blocks[-1]
    p = pool[0] if pool else 1
    t = TILES[(precision, kh, kw, blocks[-2][0], p)]
    Hc, Wc = {"one_tile": (t["TH"], t["TW"]), "two_tiles_rem": (2 * t["TH"] + p, 2 * t["TW"] + p),
              "pool_cut_rem": (t["TH"] + p + 1, t["TW"] + p + 2), "sub_tile": (p, p)}[geometry]
    if geometry == "pool_cut_rem" and t["WO"]:
        assert Wc % t["WO"] not in (0, 1)
    return Hc + sum(k[0] - 1 for _, k, _ in blocks), Wc + sum(k[1] - 1 for _, k, _ in blocks)


class Plan:
    """aa_model_create's plan of a conv chain, re-derived from the arch and
    the tile table (which stages are stored, in which layout, by which
    kernel), so that the reference applies the same epilogue; the stage names
    the library reports are asserted against it."""

    def __init__(self, arch, precision, in_c=1):
        self.blocks, self.rest = co.conv_blocks(arch)
        self.precision = precision
        nb = len(self.blocks)
        self.key, self.kind = [], []
        cin = in_c
        for i, blk in enumerate(self.blocks):
            conv = blk[0]
            kh, kw = conv["kernel"]
            pool = next((tuple(l["pool"]) for l in blk if l["type"] == "maxpool2d"), (1, 1))
            p = pool[0] if pool[0] == pool[1] and pool[0] in (1, 3) else 0
            key = (precision, kh, kw, cin, p)
            head = (i == nb - 1 and i > 0 and (kh, kw) == (1, 1) and self.rest and
                    self.rest[0]["type"] == "globalmaxpool2d" and cin % 32 == 0)
            if head:
                kind = "head"
            elif cin == 1 and (kh, kw) == (3, 3) and conv["filters"] == 32 and p == 1:
                kind = "small"
            elif i > 0 and key in TILES:
                kind = "wg" if TILES[key]["WO"] else "mfma"
            else:
                raise AssertionError(f"block {i} {key}: not a tuned shape (this test covers the tuned kernels)")
            self.key.append(key)
            self.kind.append(kind)
            cin = conv["filters"]
        cout = [b[0]["filters"] for b in self.blocks]
        self.fused = nb >= 2 and self.kind[0] == "small" and self.kind[1] == "mfma" and self.key[1][1:] == (3, 3, 32, 3)
        self.out_split = [False] * nb
        if precision == "bf16x3":
            for k in range(nb - 1):
                a_ok = self.kind[k] in ("mfma", "wg") and not (k == 0 and self.fused)
                if a_ok and self.kind[k + 1] == "mfma" and not (k + 1 == 1 and self.fused) and cout[k] % 32 == 0:
                    self.out_split[k] = True
        self.tail = (precision == "bf16x3" and nb >= 2 and self.kind[-1] == "head" and cout[-1] <= 32 and
                     self.key[-1][3] == 256 and self.kind[-2] == "mfma" and self.key[-2][1:] == (1, 3, 128, 1) and
                     nb >= 3 and self.out_split[-3] and not self.out_split[-2])
        self.stored = [k for k in range(nb) if self.kind[k] != "head" and not (k == 0 and self.fused) and
                       not (self.tail and k == nb - 2)]

    def names(self):
        out = []
        for k, blk in enumerate(self.blocks):
            conv = blk[0]
            _, kh, kw, cin, p = self.key[k]
            n = {"small": "conv_small_", "head": "head_"}.get(self.kind[k], "conv_") + f"{kh}x{kw}_{cin}_{conv['filters']}"
            n += f"_pool{p}" if p > 1 else ""
            out.append(n)
        if self.fused:
            out[1] = out[0] + "+" + out[1]
        if self.tail:
            out[-1] = out[-2] + "+" + out[-1]
        if self.kind[-1] != "head":
            c = self.blocks[-1][0]["filters"]
            out.append(f"globalmax_{c}_{c}")
        return out

    def stage_layers(self, k):
        return (self.blocks[0] + self.blocks[1]) if (k == 1 and self.fused) else self.blocks[k]


def check_stage(plan, tensors, k, x_in, g, tag, ratios):
    """The interval rule on stage k's read-out g; returns a failure message or None."""
    prec = plan.precision
    layers = plan.stage_layers(k)
    _, kh, kw, cin, p = plan.key[k]
    tile = TILES.get(plan.key[k], dict(TH=1, TW=1, WO=0, EB=False))
    kernel, c_wg = "direct", None
    if plan.kind[k] == "wg":
        kernel = "wg"
        c_wg = co.winograd_constant(tensors, layers, x_in, tile["WO"], wg_tables(tile["WO"]))
        ratios[f"{tag} c_wg"] = c_wg
    d = co.stage_check(tensors, layers, x_in, prec, kernel=kernel, c_wg=c_wg, ebf16=tile["EB"], out_split=plan.out_split[k])
    lo, hi, r, B = d["lo"], d["hi"], d["r"], d["B"]
    assert g.shape == lo.shape, (tag, g.shape, lo.shape)
    name = plan.names()[k]
    if prec in ("f32", "bf16x3"):  # the rule is |g - r| <= B (but for the f32 / split rounding of the ends)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratios[f"{tag} {name} max |g - r| / B"] = float(np.nanmax(np.abs(g - r) / B))
    else:  # stored values are bf16 / e4m3fn numbers: how many are not store(r) itself
        ratios[f"{tag} {name} share of g != store(r)"] = float((g != d["mid"]).mean())
    n, idx, ex = co.interval_violations(g, lo, hi)
    if not n:
        return None
    w_, h_, x_, c_ = idx
    pp = max(p, 1)
    return (f"{tag} stage {k} {name} [{prec}{', out_split' if plan.out_split[k] else ''}]: {n} of {g.size} elements outside, "
            f"worst (window {w_}, h {h_}, w {x_}, c {c_}) g={g[idx]!r} r={r[idx]!r} B={B[idx]:.3e} "
            f"interval [{lo[idx]!r}, {hi[idx]!r}] ({ex:.3g} half widths out); "
            f"h % TH = {h_ * pp % tile['TH']}, w % TW = {x_ * pp % tile['TW']} (tile {tile['TH']}x{tile['TW']})")


def walk(path, x, precision, tag, expect_names=None):
    """Check every stored stage and the logits of the model at `path` on x;
    returns (failure messages, {stage: max |g - r| / B})."""
    from aa_amd.model import Model
    from aa_amd._lib import AAError
    arch, tensors = co.load_arch(path)
    plan = Plan(arch, precision)
    m = Model(path, x.shape[1:], precision=precision)
    names = [m.stage_info(i)[0] for i in range(m.n_stages())]
    assert names == plan.names(), (names, plan.names())
    if expect_names is not None:
        assert names == expect_names, names
    xt = torch.from_numpy(x).cuda()
    lg0 = m.forward(xt)[0].cpu().numpy()
    fails, ratios = [], {}
    prev = x
    for k in range(m.n_stages()):
        if k not in plan.stored:
            with pytest.raises(AAError, match="never stored|writes the logits"):
                m.stage_shape(k)
            continue
        g = m.forward_prefix(xt, k).cpu().numpy()
        assert g.shape[1:] == m.stage_shape(k)
        msg = check_stage(plan, tensors, k, prev, g.astype(np.float64), tag, ratios)
        if msg:
            fails.append(msg)
        prev = g
    # a read-out leaves aa_model_forward's result alone, bit for bit
    lg1 = m.forward(xt)[0].cpu().numpy()
    if not np.array_equal(lg0, lg1):
        fails.append(f"{tag}: aa_model_forward's logits changed after forward_prefix")
    # the logits: a plain global max of the last stored stage, or the head
    if plan.kind[-1] != "head":
        if not np.array_equal(lg0, prev.max(axis=(1, 2))):
            fails.append(f"{tag} {names[-1]}: logits are not the maximum over pixels of the last stage's output")
    else:
        layers = (plan.blocks[-2] + plan.blocks[-1]) if plan.tail else plan.blocks[-1]
        lo, hi, r = co.head_interval(tensors, layers, prev, precision)
        n, idx, ex = co.interval_violations(lg0, lo, hi)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratios[f"{tag} {names[-1]}"] = float(np.nanmax(np.abs(lg0 - r) / np.maximum((hi - lo) / 2, 1e-300)))
        if n:
            fails.append(f"{tag} {names[-1]} [{precision}{', fused tail' if plan.tail else ''}]: {n} of {lg0.size} logits outside, "
                         f"worst (window {idx[0]}, label {idx[1]}) g={lg0[idx]!r} r={r[idx]!r} interval [{lo[idx]!r}, {hi[idx]!r}] "
                         f"({ex:.3g} half widths out); tail tile {TAIL_TILE['TH']}x{TAIL_TILE['TW']}")
    return fails, ratios, lg0


@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("case,C,precision", _ids())
def test_stage_activations(gpu, tmp_path, case, C, precision, geometry):
    from aa_amd._lib import AAError
    blocks = CASES[case][0](C)
    H, W = conv_geometry(blocks, precision, geometry)
    path = make_chain(tmp_path / "m", blocks, seed=11, n_mels=H, T=W)
    x = calibration_input(3, H, W, True, np.random.default_rng(H * 131 + W))
    tag = f"{case} C={C} {geometry} {H}x{W}"
    why = REFUSED.get((case, C, precision))
    if why:
        with pytest.raises(AAError, match=why):
            walk(path, x, precision, tag)
        return
    kh, kw = blocks[-1][1]
    last = f"conv_{kh}x{kw}_{blocks[-2][0]}_{C}" + ("_pool3" if blocks[-1][2] else "")
    if case == "fused_first":
        expect = ["conv_small_3x3_1_32", f"conv_small_3x3_1_32+{last}", f"globalmax_{C}_{C}"]
    else:
        expect = ["conv_small_3x3_1_32"] + [f"conv_3x3_{blocks[i - 1][0]}_{blocks[i][0]}" for i in range(1, len(blocks) - 1)] + \
                 [last, f"globalmax_{C}_{C}"]
    fails, ratios, _ = walk(path, x, precision, tag, expect)
    for k, v in ratios.items():
        print(f"{precision:7s} {k}: {v:.3e}")
    assert not fails, "\n".join(fails)


def _model1_input():
    return calibration_input(2, 160, 226, True, np.random.default_rng(226))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_model1_every_stage(gpu, model_root, precision):
    """The production network at the production geometry, with its production
    flags (fused first conv, grouped-split hand-offs, Winograd 9x3, fused
    tail): every stored stage and the logits; and aa_model_forward's logits
    are bit for bit those recorded from the commit before the read-out
    existed (tests/golden/model1_logits_t226.npz)."""
    path = model_root / "model1" / "audioModel.safetensors"
    x = _model1_input()
    fails, ratios, lg = walk(path, x, precision, "model1 160x226")
    for k, v in ratios.items():
        print(f"{precision:7s} {k}: {v:.3e}")
    assert not fails, "\n".join(fails)
    gold = np.load(GOLDEN)
    _, tensors = co.load_arch(path)
    h = hashlib.sha256()
    for k in sorted(tensors):
        h.update(k.encode())
        h.update(np.ascontiguousarray(tensors[k]).tobytes())
    assert h.hexdigest() == str(gold["weights_sha256"]), "model1's seeded weights differ from those the golden logits were recorded with"
    assert np.array_equal(lg, gold[precision]), f"{precision}: logits differ from the recorded ones, max {np.abs(lg - gold[precision]).max():.3e}"


def test_model1_bf16x3_partial_tail_tiles(gpu, model_root):
    """166 x 230: the 1x3 conv's output is 14 x 21 against the fused tail's
    13 x 5 tile, so its tiles are partial in both directions."""
    path = model_root / "model1" / "audioModel.safetensors"
    x = calibration_input(2, 166, 230, True, np.random.default_rng(166))
    fails, ratios, _ = walk(path, x, "bf16x3", "model1 166x230")
    for k, v in ratios.items():
        print(f"bf16x3  {k}: {v:.3e}")
    assert any("+head_" in k for k in ratios), list(ratios)
    assert not fails, "\n".join(fails)


def test_read_out_rejects_bad_arguments(gpu, model_root):
    from aa_amd import _lib
    from aa_amd.model import Model
    m = Model(model_root / "model1" / "audioModel.safetensors", (160, 226, 1), precision="bf16x3")
    L = _lib.lib()
    assert L.aa_model_stage_shape(m._h, -1, None, None, None) == _lib.AA_ERR_INVALID
    assert L.aa_model_stage_shape(m._h, m.n_stages(), None, None, None) == _lib.AA_ERR_INVALID
    assert L.aa_model_stage_shape(m._h, 0, None, None, None) == _lib.AA_ERR_UNSUPPORTED
    assert b"never stored" in L.aa_last_error()
    assert L.aa_model_stage_shape(m._h, m.n_stages() - 1, None, None, None) == _lib.AA_ERR_UNSUPPORTED
    x = torch.zeros((1, 160, 226, 1), device="cuda")
    act = torch.empty(m.stage_shape(1), device="cuda")
    ws = torch.empty(16, dtype=torch.uint8, device="cuda")
    rc = L.aa_model_forward_prefix(m._h, _lib.dptr(x), 1, 1, _lib.dptr(act), _lib.dptr(ws), 16, None)
    assert rc == _lib.AA_ERR_WORKSPACE
    rc = L.aa_model_forward_prefix(m._h, _lib.dptr(x), 32769, 1, _lib.dptr(act), _lib.dptr(ws), 16, None)
    assert rc == _lib.AA_ERR_INVALID and b"32768" in L.aa_last_error()


def test_read_out_follows_the_input_dtype(gpu, model_root):
    """After a float16 forward the fused first stage reads float16; a float32
    read-out then switches it back (as forward does) instead of reading the
    f32 buffer as halves, and a float16 read-out equals the f32 one of the
    same values."""
    from aa_amd.model import Model
    path = model_root / "model1" / "audioModel.safetensors"
    x = torch.from_numpy(_model1_input()).cuda().half().float()
    fresh = Model(path, (160, 226, 1), precision="bf16x3").forward_prefix(x, 1)
    m = Model(path, (160, 226, 1), precision="bf16x3")
    m.forward(x.half())
    assert torch.equal(m.forward_prefix(x, 1), fresh)
    assert torch.equal(m.forward_prefix(x.half(), 1), fresh)
    assert torch.equal(m.forward(x)[0], Model(path, (160, 226, 1), precision="bf16x3").forward(x)[0])
