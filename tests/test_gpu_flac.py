"""FLAC decode on the device (aa_flac_decode_device, csrc/aa_flac_gpu.hip):
equal to the host decoder (aa_flac_decode) and audio.decode_flac's s16 sample
for sample, per-frame statuses equal to the same core's host loop, outputs and
workspace between intact guards; flac_gpu.decode_to_device and the corpus
path's flac="gpu" mode give what the host route gives."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, str(Path(__file__).resolve().parent))

GUARD32 = np.int32(0x5A5A5A5A)
GUARD16 = np.int16(0x5A5A)
PAD = 64


def _device_decode(gpu, data, tab, n_out):
    """(i32, s16, status) of one aa_flac_decode_device call; asserts the guard
    elements around both outputs, the statuses and the workspace."""
    import torch
    from aa_amd import flac_gpu
    n_ws = max(flac_gpu.workspace_bytes(tab) // 4, 1)
    i32 = torch.full((n_out + 2 * PAD,), int(GUARD32), dtype=torch.int32, device=gpu)
    s16 = torch.full((n_out + 2 * PAD,), int(GUARD16), dtype=torch.int16, device=gpu)
    st = torch.full((len(tab) + 2 * PAD,), int(GUARD32), dtype=torch.int32, device=gpu)
    ws = torch.full((n_ws + 2 * PAD,), int(GUARD32), dtype=torch.int32, device=gpu)
    comp = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(gpu)
    flac_gpu.decode_device(comp, flac_gpu.table_to_device(tab, gpu), len(tab), st[PAD:PAD + len(tab)],
                           ws[PAD:PAD + n_ws], out_i32=i32[PAD:PAD + n_out], out_s16=s16[PAD:PAD + n_out])
    torch.cuda.synchronize()
    out = []
    for t, n, g in ((i32, n_out, GUARD32), (s16, n_out, GUARD16), (st, len(tab), GUARD32), (ws, n_ws, GUARD32)):
        h = t.cpu().numpy()
        assert (h[:PAD] == g).all() and (h[PAD + n:] == g).all()
        out.append(h[PAD:PAD + n])
    return out[0], out[1], out[2]


def _check_stream(gpu, data, name=""):
    """device == oracle (i32), == decode_flac's conversion (s16), statuses == the host core's"""
    import flac_cases as fc
    from aa_amd import flac_gpu
    q, ch, bits = fc.oracle(data)
    _, tab = flac_gpu.index(data)
    h32, h16, hst = flac_gpu.decode_frames_host(data, tab, n_out=len(q))
    d32, d16, dst = _device_decode(gpu, data, tab, len(q))
    assert dst.tolist() == hst.tolist(), name
    for f, s in zip(tab, dst):
        if s == 0:
            a, b = int(f["out_at"]), int(f["out_at"]) + int(f["keep"]) * ch
            np.testing.assert_array_equal(d32[a:b], q[a:b], err_msg=name)
            np.testing.assert_array_equal(d16[a:b], fc.to_s16(q[a:b], bits), err_msg=name)
    return dst


def test_feature_table(gpu):
    import flac_cases as fc
    from aa_amd import _lib
    for name, data, side32 in fc.table():
        st = _check_stream(gpu, data, name)
        assert set(st.tolist()) == ({_lib.AA_FLAC_FALLBACK} if side32 else {_lib.AA_FLAC_OK}), name


def test_s16_is_decode_flac(gpu):
    import flac_cases as fc
    from aa_amd import audio, flac_gpu
    rng = np.random.default_rng(3)
    for bits in (12, 24):
        data, _, _ = fc.make_stream(rng, bits, [fc.KINDS[8]], "mid_side", channels=2, block=192)
        q, _, _ = audio.decode_flac(data)
        _, tab = flac_gpu.index(data)
        _, s16, st = _device_decode(gpu, data, tab, len(q))
        assert not st.any()
        np.testing.assert_array_equal(s16.astype(np.int32), q)


def test_frames_around_a_workgroup(gpu):
    import flac_cases as fc
    from aa_amd.flac_gpu import WG
    rng = np.random.default_rng(4)
    for F in (1, WG - 1, WG, WG + 1, 2 * WG + 3):
        data, _, _ = fc.make_stream(rng, 16, [fc.KINDS[3]], block=16, n_frames=F)
        st = _check_stream(gpu, data, f"F={F}")
        assert len(st) == F and not st.any()


def test_six_streams_and_an_empty_one_in_one_call(gpu):
    import flac_cases as fc
    import flac_writer as fw
    from aa_amd import flac_gpu
    rng = np.random.default_rng(5)
    K = fc.KINDS
    streams = [fc.make_stream(rng, 16, [K[8]], block=192)[0],
               fc.make_stream(rng, 24, [K[4], K[8]], "left_side", channels=2, block=256)[0],
               fc.make_stream(rng, 8, [K[1], K[6], K[7]], channels=3, block=64, cut=9)[0],
               fw.stream([], 48000, 1, 16, 0, 16),  # no frame at all
               fc.make_stream(rng, 12, [K[5]], channels=8, block=16, n_frames=5)[0],
               fc.make_stream(rng, 20, [K[9]], "mid_side", channels=2, block=576)[0],
               fc.make_stream(rng, 16, [K[10], K[11]], channels=2, block=1000, variable=True)[0]]
    tabs, refs, byte_bases, out_bases = [], [], [], []
    nb = no = 0
    for s in streams:
        ix = flac_gpu.index(s)
        q = fc.oracle(s)
        tabs.append(ix[1])
        refs.append(q)
        byte_bases.append(nb)
        out_bases.append(no)
        nb += len(s)
        no += len(q[0])
    assert len(tabs[3]) == 0
    tab = flac_gpu.concat(tabs, byte_bases, out_bases)
    assert sorted(set(tab["stream"].tolist())) == [0, 1, 2, 4, 5, 6]
    d32, d16, st = _device_decode(gpu, b"".join(streams), tab, no)
    assert not st.any()
    np.testing.assert_array_equal(d32, np.concatenate([q[0] for q in refs]))
    np.testing.assert_array_equal(d16, np.concatenate([fc.to_s16(q[0], q[2]) for q in refs]))


def test_no_frames_is_ok(gpu):
    from aa_amd import _lib
    assert _lib.lib().aa_flac_decode_device(None, 0, None, 0, None, None, None, None, 0, None) == _lib.AA_OK


def test_damaged_streams_agree_with_the_host_core(gpu):
    """A dozen of the seeded damaged streams (tests/flac_cases.py), each run
    through the core's host loop first; the device must report the same
    statuses and, for OK frames, the same samples."""
    import flac_cases as fc
    from aa_amd import flac_gpu
    picked = [c for c in fc.fuzz() if c[0].endswith(("flip0", "trunc0", "restamp0"))]
    assert len(picked) == 12
    for name, mode, bad, good, k in picked:
        ix = flac_gpu.index(bad) if mode == "restamp" else None
        tab = ix[1] if ix is not None else flac_gpu.index(good)[1]
        n_out = len(fc.oracle(good)[0])
        h32, h16, hst = flac_gpu.decode_frames_host(bad, tab, n_out=n_out)
        if not set(hst.tolist()) <= {0, 1, 2, 3}:
            continue  # (the host core left a status undefined: not for the device)
        d32, d16, dst = _device_decode(gpu, bad, tab, n_out)
        assert dst.tolist() == hst.tolist(), name
        ch = int(tab["channels"][0])
        for f, s in zip(tab, dst):
            if s == 0:
                a, b = int(f["out_at"]), int(f["out_at"]) + int(f["keep"]) * ch
                np.testing.assert_array_equal(d32[a:b], h32[a:b], err_msg=name)
                np.testing.assert_array_equal(d16[a:b], h16[a:b], err_msg=name)


def _clip_flac(path, seed, seconds, sr=48000, bits=16, stereo=False, damage=False):
    """A synth clip as a FLAC file (LPC order 4, 4096-sample blocks: the test
    encoder is Python, a higher order only makes it slower)."""
    import flac_writer as fw
    from tools import synth
    x = synth.clip(seed, seconds=seconds, sr=sr)
    y = np.clip(np.round(x * (1 << (bits - 1))), -(1 << (bits - 1)), (1 << (bits - 1)) - 1).astype(np.int64)
    chans = [y, np.clip(y[::-1] // 2, -(1 << (bits - 1)), (1 << (bits - 1)) - 1)] if stereo else [y]
    kind = {"kind": "lpc", "order": 4, "method": 1}
    frames = [fw.frame([c[i:i + 4096] for c in chans], bits, sr, k, "mid_side" if stereo else "indep",
                       [kind] * len(chans), bs_mode="table")
              for k, i in enumerate(range(0, len(y), 4096))]
    if damage:  # frame 3 damaged, its CRC-16 made good again
        f = bytearray(frames[3])
        if damage == "reserved":  # the first subframe's type a reserved one: every decoder rejects the frame
            assert f[6] >> 1 >= 32  # (6-byte header; an LPC subframe header follows)
            f[6] = 0x04
        else:                     # one Rice bit flipped
            f[len(f) // 2] ^= 0x01
        f[-2:] = fw.crc16(bytes(f[:-2])).to_bytes(2, "big")
        frames[3] = bytes(f)
    Path(path).write_bytes(fw.stream(frames, sr, len(chans), bits, len(y), 4096))
    return str(path)


def test_decode_to_device(gpu, tmp_path):
    """The single-file entry against the host route as the corpus path runs it:
    load_recording(resample=None) and, off 48 kHz, resample_device."""
    import torch
    from aa_amd import flac_gpu
    from aa_amd import identify_tracks as it
    from aa_amd.resample import resample_device
    mono = _clip_flac(tmp_path / "mono.flac", 21, 2.0)
    pcm, sr = flac_gpu.decode_to_device(mono, gpu)
    ref, ref_sr = it.load_recording(mono, resample=None)
    assert sr == ref_sr == 48000 and pcm.dtype == torch.float32
    assert np.array_equal(pcm.cpu().numpy(), ref)
    assert np.array_equal(flac_gpu.decode_to_device(Path(mono).read_bytes(), gpu)[0].cpu().numpy(), ref)
    st = _clip_flac(tmp_path / "st.flac", 22, 2.0, sr=44100, bits=24, stereo=True)
    pcm, sr = flac_gpu.decode_to_device(st, gpu)
    ref, ref_sr = it.load_recording(st, resample=None)
    assert sr == ref_sr == 44100
    assert np.array_equal(pcm.cpu().numpy(), ref)  # bit-equal before the resampler ...
    a = resample_device(pcm, 44100, 48000)
    b = resample_device(torch.from_numpy(np.ascontiguousarray(ref, dtype=np.float32)).to(gpu), 44100, 48000)
    assert torch.equal(a, b)                        # ... and therefore after it
    # a damaged file: the host route's samples or its exception
    bad = _clip_flac(tmp_path / "bad.flac", 23, 2.0, damage=True)
    try:
        ref, _ = it.load_recording(bad, resample=None)
    except Exception as e:
        with pytest.raises(type(e)):
            flac_gpu.decode_to_device(bad, gpu)
    else:
        assert np.array_equal(flac_gpu.decode_to_device(bad, gpu)[0].cpu().numpy(), ref)


def _docs(res):
    return json.dumps({k: {kk: vv for kk, vv in v.items() if kk != "processing_time_seconds"}
                       for k, v in res.items()}, sort_keys=True)


def test_batch_gpu_mode_matches_host_mode(gpu, model_root, tmp_path):
    from aa_amd.batch import BatchAnalyser
    files = [_clip_flac(tmp_path / "a.flac", 31, 3.5),
             _clip_flac(tmp_path / "b.flac", 32, 3.5, sr=44100, bits=24, stereo=True),
             _clip_flac(tmp_path / "c.flac", 33, 3.5, damage=True),
             # 32-bit mid/side: every frame falls back, the file is redone on the host inside the batch
             _clip_flac(tmp_path / "d.flac", 34, 3.5, bits=32, stereo=True)]
    models = [str(model_root / "model1" / "audioModel.keras")]
    jobs = list(enumerate(files))
    host = BatchAnalyser(models, False, device=gpu, batch=4, lanes=1, flac="host").run(jobs)
    dev = BatchAnalyser(models, False, device=gpu, batch=4, lanes=1, flac="gpu").run(jobs)
    assert _docs(dev) == _docs(host)
    assert len(host) == 4 and sum(1 for d in host.values() if d.get("species_identify")) >= 2


def test_batch_file_failing_its_host_redo_leaves_the_others_alone(gpu, model_root, tmp_path):
    """A stereo file whose CRCs are all good but whose frame 3 no decoder
    accepts: indexed, refused by the device, then by the host redo.  It still
    holds its (stereo) place in the int16 buffer, so the mono files behind it
    must be widened each from its own place."""
    from aa_amd import corpus, flac_gpu
    from aa_amd import identify_tracks as it
    from aa_amd.batch import BatchAnalyser
    bad = _clip_flac(tmp_path / "bad.flac", 41, 3.5, stereo=True, damage="reserved")
    assert flac_gpu.index(Path(bad).read_bytes()) is not None
    with pytest.raises(Exception):
        it.load_recording(bad, resample=None)
    files = [bad, _clip_flac(tmp_path / "m1.flac", 42, 3.5), _clip_flac(tmp_path / "m2.flac", 43, 4.0)]
    models = [str(model_root / "model1" / "audioModel.keras")]
    jobs = list(enumerate(files))
    host = BatchAnalyser(models, False, device=gpu, batch=4, lanes=1, flac="host").run(jobs)
    dev = BatchAnalyser(models, False, device=gpu, batch=4, lanes=1, flac="gpu").run(jobs)
    assert corpus.FAILED in host[0] and host[0] == dev[0]
    assert host[1].get("species_identify") and host[2].get("species_identify")
    assert _docs(dev) == _docs(host)


def test_batch_host_redo_of_another_length(gpu, model_root, tmp_path, monkeypatch):
    """The host redo may decode another number of samples than the index
    counted (a crafted stream can make the two differ).  Stood in for here by
    a load_recording that lengthens one file and shortens another, in both
    modes alike: the file takes the host's length, the others are unaffected."""
    from aa_amd import identify_tracks as it
    from aa_amd.batch import BatchAnalyser
    files = [_clip_flac(tmp_path / "long.flac", 51, 3.5, bits=32, stereo=True),  # 32-bit mid/side: always redone
             _clip_flac(tmp_path / "m1.flac", 52, 3.5),
             _clip_flac(tmp_path / "short.flac", 53, 4.0, bits=32, stereo=True),
             _clip_flac(tmp_path / "m2.flac", 54, 3.5)]
    orig = it.load_recording

    def load(file, resample=48000):
        frames, sr = orig(file, resample=resample)
        name = Path(str(file)).name
        if name == "long.flac":
            frames = np.concatenate([frames, frames[:9600]])
        elif name == "short.flac":
            frames = frames[:-9600]
        return frames, sr

    monkeypatch.setattr(it, "load_recording", load)
    models = [str(model_root / "model1" / "audioModel.keras")]
    jobs = list(enumerate(files))
    host = BatchAnalyser(models, False, device=gpu, batch=4, lanes=1, flac="host").run(jobs)
    dev = BatchAnalyser(models, False, device=gpu, batch=4, lanes=1, flac="gpu").run(jobs)
    assert _docs(dev) == _docs(host)
    assert all(d.get("species_identify") for d in host.values())
