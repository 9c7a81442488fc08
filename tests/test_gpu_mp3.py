"""MP3 decode on the device (aa_mp3_decode_device, csrc/aa_mp3_gpu.hip): int16
and float outputs and the statuses equal, bit for bit, to the same core's host
loops (aa_mp3_decode_frames_host -- the host decoder, which
tests/test_mp3_core.py holds to the numpy oracle) over the writer's stream
table, the real file and damaged streams; outputs, statuses and workspace
between intact guards; one call holding every stream of the table (three
rates, mono and stereo, more than one unpack workgroup);
mp3_gpu.decode_to_device and the corpus path's mp3="gpu" mode give what the
host route gives."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, str(Path(__file__).resolve().parent))

REAL = Path(__file__).resolve().parent / "golden" / "mp3" / "invalid_keypress.mp3"
GUARD32 = np.int32(0x5A5A5A5A)
GUARD16 = np.int16(0x5A5A)
PAD = 64


def _device_decode(gpu, payload, frames, streams, n_out):
    """(f32, s16, status) of one aa_mp3_decode_device call; asserts the guard
    elements around both outputs, the statuses and the workspace."""
    import torch
    from aa_amd import mp3_gpu as mg
    n_ws = max(mg.workspace_bytes(len(frames)) // 4, 2)
    n_st = 4 * len(frames)
    f32 = torch.full((n_out + 2 * PAD,), int(GUARD32), dtype=torch.int32, device=gpu)
    s16 = torch.full((n_out + 2 * PAD,), int(GUARD16), dtype=torch.int16, device=gpu)
    st = torch.full((n_st + 2 * PAD,), int(GUARD32), dtype=torch.int32, device=gpu)
    ws = torch.full((n_ws + 4 * PAD,), int(GUARD32), dtype=torch.int32, device=gpu)
    comp = torch.from_numpy(np.ascontiguousarray(payload).copy()).to(gpu)
    mg.decode_device(comp, mg.to_device(frames, gpu), len(frames), mg.to_device(streams, gpu), len(streams),
                     st[PAD:PAD + n_st], ws[2 * PAD:2 * PAD + n_ws], out_s16=s16[PAD:PAD + n_out],
                     out_f32=f32[PAD:PAD + n_out].view(torch.float32), out_elems=n_out)
    torch.cuda.synchronize()
    out = []
    for t, n, g, pad in ((f32, n_out, GUARD32, PAD), (s16, n_out, GUARD16, PAD), (st, n_st, GUARD32, PAD),
                         (ws, n_ws, GUARD32, 2 * PAD)):
        h = t.cpu().numpy()
        assert (h[:pad] == g).all() and (h[pad + n:] == g).all()
        out.append(h[pad:pad + n])
    return out[0].view(np.float32), out[1], out[2].reshape(-1, 2, 2)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _check(gpu, ix, name=""):
    from aa_amd import mp3_gpu as mg
    n_out = int(ix.stream["frames"][0] * ix.stream["channels"][0])
    h32, h16, hst = mg.decode_frames_host(ix.payload, ix.frames, ix.stream, n_out=n_out)
    d32, d16, dst = _device_decode(gpu, ix.payload, ix.frames, ix.stream, n_out)
    assert np.array_equal(dst, hst), name
    assert _same_bits(d32, h32), name
    assert np.array_equal(d16, h16), name
    return hst


def test_stream_table(gpu):
    import mp3_cases as mc
    from aa_amd import mp3_gpu as mg
    for name in mc.NAMES:
        st = _check(gpu, mg.index(mc.case(name)["data"]), name)
        assert (st != 0).sum() == len(mc.case(name)["silent"]), name


def test_real_file(gpu):
    from aa_amd import mp3_gpu as mg
    st = _check(gpu, mg.index(REAL.read_bytes()), "real")
    assert not st.any()


def test_whole_table_in_one_call(gpu):
    import mp3_cases as mc
    from aa_amd import mp3_gpu as mg
    items = [mg.index(mc.case(n)["data"]) for n in mc.NAMES] + [mg.index(REAL.read_bytes())]
    assert {int(ix.stream["sample_rate"][0]) for ix in items} == {32000, 44100, 48000}
    assert {int(ix.stream["channels"][0]) for ix in items} == {1, 2}
    byte_bases, out_bases, at, o = [], [], 3, 5
    for k, ix in enumerate(items):  # staggered: odd gaps in front of every payload and output
        byte_bases.append(at)
        out_bases.append(o)
        at += ix.payload.size + 1 + 2 * k
        o += int(ix.stream["frames"][0] * ix.stream["channels"][0]) + 3 + k
    b = mg.concat(items, byte_bases, out_bases)
    assert 2 * len(b.frames) > mg.WG  # more than one unpack workgroup
    payload = np.full(at, 0xA5, np.uint8)
    for ix, base in zip(items, byte_bases):
        payload[base:base + ix.payload.size] = ix.payload
    d32, d16, dst = _device_decode(gpu, payload, b.frames, b.streams, o)
    covered = np.zeros(o, bool)
    first = 0
    for ix, ob in zip(items, out_bases):
        n = int(ix.stream["frames"][0] * ix.stream["channels"][0])
        h32, h16, hst = mg.decode_frames_host(ix.payload, ix.frames, ix.stream)
        assert _same_bits(d32[ob:ob + n], h32) and np.array_equal(d16[ob:ob + n], h16)
        assert np.array_equal(dst[first:first + len(ix.frames)], hst)
        first += len(ix.frames)
        covered[ob:ob + n] = True
    # between the streams' outputs nothing was written
    assert (d32.view(np.int32)[~covered] == GUARD32).all() and (d16[~covered] == GUARD16).all()


def test_damaged_streams_equal_the_host_twin(gpu):
    """24 of the seeded damaged streams (tests/mp3_cases.py) that still index."""
    import mp3_cases as mc
    from aa_amd import mp3_gpu as mg
    done = 0
    for name, bad in mc.fuzz():
        ix = mg.index(bad)
        if ix is None or not int(ix.stream["frames"][0]):
            continue
        _check(gpu, ix, name)
        done += 1
        if done == 24:
            break
    assert done == 24


def test_no_frames_is_ok(gpu):
    from aa_amd import _lib
    assert _lib.lib().aa_mp3_decode_device(None, None, 0, None, 0, None, 0, None, None, 0, None, None, 0,
                                           None) == _lib.AA_OK


def test_decode_to_device(gpu):
    import torch
    from aa_amd import audio, mp3_gpu as mg
    pcm, sr = mg.decode_to_device(str(REAL), gpu)
    ref, ref_sr = audio.decode(str(REAL))
    assert sr == ref_sr == 44100 and pcm.dtype == torch.float32 and pcm.shape == (23087,)
    assert np.array_equal(pcm.cpu().numpy(), ref)
    assert np.array_equal(mg.decode_to_device(REAL.read_bytes(), gpu)[0].cpu().numpy(), ref)


def _docs(res):
    return json.dumps({k: {kk: vv for kk, vv in v.items() if kk != "processing_time_seconds"}
                       for k, v in res.items()}, sort_keys=True)


@pytest.fixture(scope="module")
def corpus_files(tmp_path_factory):
    """The real file (stereo 44.1 kHz), a mono writer stream, and a WAV."""
    import mp3_cases as mc
    from tools import synth
    d = tmp_path_factory.mktemp("mp3_corpus")
    files = []
    p = d / "real.mp3"
    p.write_bytes(REAL.read_bytes())
    files.append(p)
    p = d / "mono.mp3"
    p.write_bytes(mc.case("mono_long")["data"])
    files.append(p)
    p = d / "a.wav"
    synth.write_wav(p, synth.clip(500, seconds=4.0))
    files.append(p)
    return [str(f) for f in files]


def test_batch_gpu_mode_matches_host_mode_and_per_file(gpu, model_root, corpus_files, monkeypatch):
    from aa_amd import corpus, mp3_gpu as mg
    from aa_amd.batch import BatchAnalyser
    calls, real = [], mg.decode_device

    def counted(*args, **kw):
        calls.append(int(args[4]))  # streams of the call
        return real(*args, **kw)

    monkeypatch.setattr(mg, "decode_device", counted)
    models = [str(model_root / "model1" / "audioModel.keras")]
    jobs = list(enumerate(corpus_files))
    host = BatchAnalyser(models, False, device=gpu, batch=4, lanes=1, mp3="host").run(jobs)
    assert not calls
    dev = BatchAnalyser(models, False, device=gpu, batch=4, lanes=1, mp3="gpu").run(jobs)
    assert sum(calls) == 2
    assert _docs(dev) == _docs(host)
    per_file = corpus.run(corpus_files, models, False, batch=0)
    assert _docs(dev) == _docs(per_file)
    assert all(corpus.FAILED not in dev[k] for k in range(3))
