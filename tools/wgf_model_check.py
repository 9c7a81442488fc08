"""Input for the conv_wgf harness (tools/wgf_check.hip, WGF_DATA): the BN-folded
weights of a calibrated two-conv chain (3x3 1->32, 3x3 32->32 + pool 3) and the
dB-like check input, as raw f32 files.  (conv_wgf lives in the tools/ harness
only: libaa.so serves the pair with conv_x3, which
tests/test_gpu_cnn_stages.py checks per element.)

    python tools/wgf_model_check.py OUT_DIR
"""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "audio-analysis_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def dump(out):
    """The chain's BN-folded pair and the check input as raw f32 for tools/wgf_check (WGF_DATA)."""
    import numpy as np
    from oracle import cnn_oracle
    from tools.make_models import calibration_input, make_chain
    out = Path(out)
    p = make_chain(out / "chain", [(32, (3, 3), None), (32, (3, 3), (3, 3))])
    arch, t = cnn_oracle.load_arch(p)
    folded = []
    for i, ly in enumerate(arch):
        if ly["type"] != "conv2d":
            continue
        w = np.asarray(t[ly["name"] + ".kernel"], np.float64)  # [kh][kw][cin][cout]
        b = np.asarray(t[ly["name"] + ".bias"], np.float64) if ly.get("use_bias") else np.zeros(w.shape[-1])
        bn = arch[i + 1]
        s = np.asarray(t[bn["name"] + ".gamma"], np.float64) / np.sqrt(np.asarray(t[bn["name"] + ".moving_variance"], np.float64) + float(bn.get("eps", 1e-3)))
        b = (b - np.asarray(t[bn["name"] + ".moving_mean"], np.float64)) * s + np.asarray(t[bn["name"] + ".beta"], np.float64)
        folded.append((w * s, b))
    (w1, b1), (w2, b2) = folded
    x = calibration_input(6, 160, 226, True, np.random.default_rng(232))
    np.ascontiguousarray(x[..., 0], np.float32).tofile(out / "x.bin")
    np.ascontiguousarray(w1.reshape(9, 32).T, np.float32).tofile(out / "w1.bin")  # [cout][tap]
    b1.astype(np.float32).tofile(out / "b1.bin")
    np.ascontiguousarray(w2.reshape(9, 32, 32), np.float32).tofile(out / "k2.bin")  # [tap][cin][cout]
    b2.astype(np.float32).tofile(out / "b2.bin")
    print("folded |w1| max", np.abs(w1).max(), "|b1| max", np.abs(b1).max(), "|w2| max", np.abs(w2).max(), "|b2| max", np.abs(b2).max())


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--dump"]
    if len(args) != 1:
        sys.exit(__doc__)
    dump(args[0])
