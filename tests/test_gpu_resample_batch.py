"""aa_resample_batch (csrc/aa_resample.hip): every recording of a batch that
shares an input rate, to 16 kHz in one launch.

The contract is bit equality with what the product did before it: for an int16
segment aa_pcm_s16_to_f32 followed by aa_resample_poly, for an f32 segment
aa_resample_poly alone, on the same device.  One table of segments per input
rate: int16 (1, 2 and 3 channels) and f32 sources in one launch, odd source
offsets, a 0.25-level run between neighbours (a read across a boundary would
show), lengths around the 256-output tile, one input shorter than the filter,
and an output buffer pre-filled with a sentinel.  The samples are also held to
tests/test_gpu_resample.py's gate against the float64 oracle.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-5            # tests/test_gpu_resample.py's gate (inputs of amplitude <= 0.3, as there)
SR_OUT = 16000
RATES = [48000, 44100, 8000, 96000]  # L/M = 1/3, 160/441, 2/1 (upsampling), 1/6
N_OUT = [0, 1, 255, 256, 257, 3 * 256 + 1]
SENTINEL = np.uint32(0x7FC5A5A5)     # a NaN no filter produces
GAP16 = 8192                         # 0.25 as int16


def _case(sr):
    """The segment table of one rate and its host-side truth."""
    from aa_amd import _lib
    from aa_amd.audio import _to_mono
    from aa_amd.resample import design, out_length
    L, M, half, taps, _ = design(sr, SR_OUT)
    rng = np.random.default_rng(sr)
    shapes = [(-(-n * M // L), n) for n in N_OUT]          # (n_in, n_out): out_length(n_in) >= n_out
    short = taps // 2                                       # shorter than the filter: both edges in one tile
    shapes.append((short, out_length(short, sr, SR_OUT)))
    assert short < taps and 0 < shapes[-1][1] <= 256
    s16_parts, f32_parts, segs, mono = [], [], [], []
    o16 = of = dst = 0
    for i, (n_in, n_out) in enumerate(shapes * 2):          # every length once as int16 and once as f32
        is16 = i < len(shapes)
        ch = 1 + i % 3
        x = np.clip(rng.standard_normal(n_in * (ch if is16 else 1)) * 0.3, -1, 1)
        dst += 1 + 2 * (i % 3)                              # a gap of sentinels in front of each output range
        if is16:
            q = np.round(x * 32767).astype(np.int16)
            gap = 1 if (o16 + 1) % 2 else 2                 # every source offset odd
            s16_parts += [np.full(gap, GAP16, np.int16), q]
            o16 += gap
            segs.append(_lib.RsSegment(src_off=o16, n_in=n_in, dst_off=dst, n_out=n_out, kind=_lib.AA_RS_S16,
                                       channels=ch))
            o16 += len(q)
            mono.append(_to_mono(q, ch))
        else:
            v = x.astype(np.float32)
            gap = 1 if (of + 1) % 2 else 2
            f32_parts += [np.full(gap, 0.25, np.float32), v]
            of += gap
            segs.append(_lib.RsSegment(src_off=of, n_in=n_in, dst_off=dst, n_out=n_out, kind=_lib.AA_RS_F32,
                                       channels=1))
            of += len(v)
            mono.append(v)
        dst += n_out
    # interleave the two kinds in the table, so that neighbours in it differ in kind
    order = [k for pair in zip(range(len(shapes)), range(len(shapes), 2 * len(shapes))) for k in pair]
    segs, mono = [segs[k] for k in order], [mono[k] for k in order]
    s16_parts.append(np.full(3, GAP16, np.int16))
    f32_parts.append(np.full(3, 0.25, np.float32))
    assert all(s.src_off % 2 for s in segs)
    assert {s.channels for s in segs if s.kind == _lib.AA_RS_S16} == {1, 2, 3}
    return {"sr": sr, "filter": (L, M, half, taps), "segs": segs, "mono": mono, "s16": np.concatenate(s16_parts),
            "f32": np.concatenate(f32_parts), "n_y": dst + 5}


def _sentinel_buffer(n, dev):
    import torch
    return torch.from_numpy(np.full(n, SENTINEL, np.uint32).view(np.float32).copy()).to(dev)


def _launch(case, segs, dev, s16, f32):
    """One aa_resample_batch over `segs` into a fresh sentinel buffer -> its words (uint32)."""
    import torch
    from aa_amd.ci_batch import resample_batch
    y = _sentinel_buffer(case["n_y"], dev)
    resample_batch(s16, f32, segs, case["sr"], y)
    torch.cuda.synchronize()
    return y.cpu().numpy().view(np.uint32)


def _two_step(case, sg, dev, s16, f32):
    """The product's earlier way on the same device: aa_pcm_s16_to_f32 then aa_resample_poly."""
    import torch
    from aa_amd import _lib
    from aa_amd.resample import _bank
    L, M, half, taps, bank = _bank(case["sr"], SR_OUT, dev)
    lib = _lib.lib()
    if sg.kind == _lib.AA_RS_S16:
        x = torch.empty(max(sg.n_in, 1), dtype=torch.float32, device=dev)
        if sg.n_in:
            _lib.check(lib.aa_pcm_s16_to_f32(_lib.dptr(s16) + 2 * sg.src_off, sg.n_in, sg.channels, _lib.dptr(x),
                                             _lib.stream_ptr()), "aa_pcm_s16_to_f32")
        xp = _lib.dptr(x)
    else:
        xp = _lib.dptr(f32) + 4 * sg.src_off
    y = _sentinel_buffer(max(sg.n_out, 1), dev)
    _lib.check(lib.aa_resample_poly(xp, sg.n_in, _lib.dptr(bank), L, M, taps, half, _lib.dptr(y), sg.n_out,
                                    _lib.stream_ptr()), "aa_resample_poly")
    torch.cuda.synchronize()
    return y.cpu().numpy().view(np.uint32)[:sg.n_out]


@pytest.mark.parametrize("sr", RATES)
def test_batch_is_bit_equal_to_the_two_step_path(gpu, sr):
    import torch
    from oracle import resample_oracle as ro
    case = _case(sr)
    segs = case["segs"]
    s16 = torch.from_numpy(case["s16"]).to(gpu)
    f32 = torch.from_numpy(case["f32"]).to(gpu)
    got = _launch(case, segs, gpu, s16, f32)
    again = _launch(case, segs, gpu, s16, f32)
    assert again.tobytes() == got.tobytes()                      # a second run: the same words
    written = np.zeros(case["n_y"], bool)
    worst = 0.0
    for sg, mono in zip(segs, case["mono"]):
        words = got[sg.dst_off:sg.dst_off + sg.n_out]
        written[sg.dst_off:sg.dst_off + sg.n_out] = True
        what = (sr, sg.kind, sg.channels, sg.n_in, sg.n_out)
        assert words.tobytes() == _two_step(case, sg, gpu, s16, f32).tobytes(), what
        alone = _launch(case, [sg], gpu, s16, f32)
        assert alone[sg.dst_off:sg.dst_off + sg.n_out].tobytes() == words.tobytes(), what
        assert (np.delete(alone, np.s_[sg.dst_off:sg.dst_off + sg.n_out]) == SENTINEL).all(), what
        if sg.n_out:
            ref = ro.resample(mono.astype(np.float64), sr, SR_OUT)
            assert len(ref) >= sg.n_out and len(mono) == sg.n_in
            err = float(np.abs(words.view(np.float32) - ref[:sg.n_out]).max())
            worst = max(worst, err)
            assert err <= TOL, (what, err)
    print(f"{sr} -> {SR_OUT}: {len(segs)} segments, taps {case['filter'][3]}, max|d| vs float64 {worst:.2e}")
    # between and after the segments nothing was written
    assert written.sum() == sum(s.n_out for s in segs) and (got[~written] == SENTINEL).all()
    assert not (got[written] == SENTINEL).any()


def test_segments_that_leave_their_buffers_are_skipped(gpu):
    """The table is device memory the call cannot check: a segment whose ranges
    leave the source or the output buffer, or whose kind or channels are
    invalid, is skipped whole, and the segments around it are computed."""
    import torch
    from aa_amd import _lib
    case = _case(48000)
    s16 = torch.from_numpy(case["s16"]).to(gpu)
    f32 = torch.from_numpy(case["f32"]).to(gpu)
    good = [s for s in case["segs"] if s.n_out == 257]
    assert len(good) == 2
    S = _lib.RsSegment
    bad = [S(src_off=len(case["s16"]) - 5, n_in=6, dst_off=0, n_out=2, kind=_lib.AA_RS_S16, channels=1),
           S(src_off=len(case["f32"]) - 5, n_in=6, dst_off=0, n_out=2, kind=_lib.AA_RS_F32, channels=1),
           S(src_off=1, n_in=6, dst_off=case["n_y"] - 1, n_out=2, kind=_lib.AA_RS_F32, channels=1),
           S(src_off=-1, n_in=6, dst_off=0, n_out=2, kind=_lib.AA_RS_F32, channels=1),
           S(src_off=1, n_in=6, dst_off=-1, n_out=2, kind=_lib.AA_RS_F32, channels=1),
           S(src_off=1, n_in=6, dst_off=0, n_out=2, kind=2, channels=1),
           S(src_off=1, n_in=2, dst_off=0, n_out=2, kind=_lib.AA_RS_S16, channels=9),
           S(src_off=1, n_in=-1, dst_off=0, n_out=2, kind=_lib.AA_RS_F32, channels=1)]
    want = _launch(case, good, gpu, s16, f32)
    got = _launch(case, [good[0]] + bad + [good[1]], gpu, s16, f32)
    assert got.tobytes() == want.tobytes()
    assert (got[:good[0].dst_off] == SENTINEL).all() and (got[-5:] == SENTINEL).all()
