"""The batched old-cacophony-index path without a device: the corpus CLI's
flag, the host-side planning of a batch's 16 kHz buffer (aa_amd/ci_batch.py)
and aa_resample_batch's argument checks, which come before any HIP call."""
import ctypes as C
from math import ceil

import numpy as np
import pytest

import ci_restated
from aa_amd import _lib, corpus
from aa_amd.ci_batch import Plan, Source, plan_segments
from aa_amd.resample import design, out_length


def test_parse_args_accepts_the_flag():
    args = corpus.parse_args(["a.wav", "b.wav", "--old-cacophony-index", "-o"])
    assert args.old_cacophony_index == 1 and args.meta_to_stdout == 1 and args.files == ["a.wav", "b.wav"]
    # --bird-model is accepted and carried, as analyse.py carries it; run() ignores it in this mode
    args = corpus.parse_args(["a.wav", "--old-cacophony-index", "--bird-model", "m.keras"])
    assert args.old_cacophony_index == 1 and args.bird_model == ["m.keras"]


def test_parse_args_defaults_are_unchanged():
    args = vars(corpus.parse_args(["a.wav"]))
    assert args.pop("old_cacophony_index") is None  # action="count", as analyse.py's
    assert args == {"files": ["a.wav"], "analyse_tracks": False, "meta_to_stdout": None, "gpus": 1, "backend": None,
                    "bird_model": ["/models/pre-model/audioModel.keras", "/models/bird-model-v2m/audioModel.keras"]}


def test_run_without_a_batch_goes_file_by_file_through_calculate(monkeypatch):
    from aa_amd import cacophony_index
    seen = []

    def fake(path):
        seen.append(path)
        if path.endswith("bad.wav"):
            raise ValueError(f"{path}: missing fmt/data chunk")
        return {"cacophony_index_old": [], "cacophony_index_old_version": cacophony_index.VERSION}

    monkeypatch.setattr(cacophony_index, "calculate", fake)
    res = corpus.run(["a.wav", "bad.wav", "c.wav"], None, batch=0, old_cacophony_index=True)
    assert seen == ["a.wav", "bad.wav", "c.wav"] and sorted(res) == [0, 1, 2]
    assert res[1] == {corpus.FAILED: "ValueError: bad.wav: missing fmt/data chunk"}
    for k in (0, 2):
        assert isinstance(res[k].pop("processing_time_seconds"), float)
        assert res[k] == {"cacophony_index_old": [], "cacophony_index_old_version": "2020-01-20_A"}


def _n_frames(n):
    return int(_lib.lib().aa_ci_n_frames(n))


def _check_plan(plan: Plan, sources):
    pos = 0
    seen = {}
    for k, s in enumerate(sources):
        n = ceil(s.n_in * 16000.0 / s.sr)
        assert n == out_length(s.n_in, s.sr, 16000)
        assert plan.offsets[k] == pos and plan.lengths[k] == n, k
        assert plan.points[k] == max(_n_frames(n) - 1, 0) == max(ci_restated.n_frames(n) - 1, 0), k
        pos += n
    assert plan.total == pos
    for sr, segs in plan.resample:
        assert 1 <= len(segs) <= 64 and sr != 16000
        for k, g in segs:
            s = sources[k]
            assert k not in seen and s.sr == sr
            seen[k] = g
            assert (g.kind, g.src_off, g.n_in) == (s.kind, s.off, s.n_in)
            assert g.channels == (s.channels if s.kind == _lib.AA_RS_S16 else 1)
            assert (g.dst_off, g.n_out) == (plan.offsets[k], plan.lengths[k])
    assert sorted(list(seen) + plan.direct) == list(range(len(sources)))
    assert all(sources[k].sr == 16000 for k in plan.direct)
    assert [k for g in plan.groups for k in g] == list(range(len(sources)))
    assert all(1 <= len(g) <= 64 for g in plan.groups)


def test_plan_of_mixed_rates_and_a_zero_length_file():
    S16, F32 = _lib.AA_RS_S16, _lib.AA_RS_F32
    src = [Source(S16, 0, 960001, 1, 48000), Source(S16, 960001, 441001, 2, 44100), Source(F32, 0, 0, 1, 48000),
           Source(S16, 1842003, 320000, 1, 16000), Source(F32, 0, 160001, 1, 8000), Source(F32, 160001, 5, 1, 16000),
           Source(S16, 2162003, 0, 3, 44100), Source(S16, 2162003, 1920000, 3, 96000)]
    plan = plan_segments(src)
    _check_plan(plan, src)
    assert plan.lengths == [320001, 160001, 0, 320000, 320002, 5, 0, 320000]
    assert [sr for sr, _ in plan.resample] == [48000, 44100, 8000, 96000]  # one launch per distinct rate
    assert plan.direct == [3, 5] and plan.groups == [list(range(8))]
    assert plan.points[2] == 0 and plan.points[3] == 308  # 309 frames of 2048 at hop 1024 from sample 1024
    assert plan_segments([]).total == 0 and plan_segments([]).groups == []


def test_plan_of_more_than_64_files():
    rng = np.random.default_rng(5)
    src, o16 = [], 0
    for k in range(150):
        sr = (48000, 44100, 16000)[k % 3]
        n = int(rng.integers(0, 3 * sr))
        src.append(Source(_lib.AA_RS_S16, o16, n, 1 + k % 2, sr))
        o16 += n * (1 + k % 2)
    plan = plan_segments(src)
    _check_plan(plan, src)
    assert [len(g) for g in plan.groups] == [64, 64, 22]
    assert sorted(len(s) for _, s in plan.resample) == [50, 50]
    many = plan_segments([Source(_lib.AA_RS_F32, 0, 3, 1, 48000)] * 130)
    assert [(sr, len(s)) for sr, s in many.resample] == [(48000, 64), (48000, 64), (48000, 2)]
    assert many.lengths == [1] * 130 and many.offsets == list(range(130))


def test_plan_refuses_bad_sources():
    for bad in (Source(2, 0, 1, 1, 48000), Source(0, 0, -1, 1, 48000), Source(0, -1, 1, 1, 48000),
                Source(0, 0, 1, 9, 48000), Source(0, 0, 1, 0, 48000), Source(1, 0, 1, 1, 0)):
        with pytest.raises(ValueError):
            plan_segments([bad])


def test_segment_binding_matches_the_header():
    import re
    from pathlib import Path
    text = (Path(__file__).resolve().parent.parent / "include" / "aa.h").read_text()
    body = re.search(r"typedef struct aa_rs_segment \{(.*?)\}", text, re.S).group(1)
    fields = [(n.strip(), {"int64_t": C.c_int64, "int32_t": C.c_int32}[decl.split()[0]])
              for decl in body.split(";") if decl.strip()
              for n in decl.strip().split(None, 1)[1].split(",")]
    assert fields == list(_lib.RsSegment._fields_) and C.sizeof(_lib.RsSegment) == 40
    assert re.search(r"#define AA_RS_S16 0\b", text) and re.search(r"#define AA_RS_F32 1\b", text)


# (any non-null address will do: the checks return before the pointers are used)
P = 0x1000


def _call(**kw):
    L, M, half, taps, _ = design(48000, 16000)
    a = dict(src_s16=P, n_s16=10, src_f32=P, n_f32=10, segs=P, n_seg=1, max_n_out=4, bank=P, L=L, M=M, taps=taps,
             half=half, y=P, n_y=8, stream=None)
    a.update(kw)
    rc = _lib.lib().aa_resample_batch(a["src_s16"], a["n_s16"], a["src_f32"], a["n_f32"], a["segs"], a["n_seg"],
                                      a["max_n_out"], a["bank"], a["L"], a["M"], a["taps"], a["half"], a["y"],
                                      a["n_y"], a["stream"])
    return rc, _lib.lib().aa_last_error().decode()


@pytest.mark.parametrize("kw, named", [
    (dict(segs=None), "segs_dev"), (dict(bank=None), "bank"), (dict(y=None), "y"),
    (dict(src_s16=None), "src_s16"), (dict(src_f32=None), "src_f32"),
    (dict(n_s16=-1), "n_s16"), (dict(n_f32=-1), "n_f32"), (dict(n_y=-1), "n_y"),
    (dict(n_seg=-1), "n_seg"), (dict(n_seg=65), "n_seg"),
    (dict(max_n_out=-1), "max_n_out"), (dict(max_n_out=9), "max_n_out"),
    (dict(L=0), "L"), (dict(M=0), "M"), (dict(taps=0), "taps"),
    (dict(half=-1), "half"), (dict(half=571), "half"), (dict(L=2, taps=100, half=200), "half"),
    (dict(taps=20000, half=5), "LDS"),
])
def test_resample_batch_refuses_bad_arguments(kw, named):
    assert _lib.AA_CI_MAX_REC == 64 and design(48000, 16000)[3] == 571
    rc, msg = _call(**kw)
    assert rc == _lib.AA_ERR_INVALID
    assert msg.startswith("aa_resample_batch: ") and named in msg, msg


def test_resample_batch_with_nothing_to_do_is_ok():
    # no segments, or none with an output: AA_OK before any launch (this machine may have no device)
    assert _call(n_seg=0)[0] == _lib.AA_OK
    assert _call(max_n_out=0)[0] == _lib.AA_OK
    assert _call(src_s16=None, n_s16=0, src_f32=None, n_f32=0, n_seg=0)[0] == _lib.AA_OK
