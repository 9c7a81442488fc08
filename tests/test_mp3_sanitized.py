"""The MP3 decoder's index and core under host ASan + UBSan:
tools/mp3_core_check.cpp (stand-alone, its own main; nothing is loaded into
Python) is built with the sanitizers and run over the stream table, the real
file and the seeded damaged streams of tests/mp3_cases.py -- each one indexed
and decoded through the core into exact-size heap blocks.  Exit status 0 and
no sanitizer report."""
import shutil
import subprocess
from pathlib import Path

import pytest

import mp3_cases as mc

ROOT = Path(__file__).resolve().parent.parent
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def _clangxx():
    from aa_amd import _build
    for c in (Path(_build.hipcc()).resolve().parent.parent / "lib" / "llvm" / "bin" / "clang++",
              Path(_build.hipcc()).resolve().parent / "clang++", shutil.which("clang++")):
        if c and Path(c).exists():
            return str(c)
    return None


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    work = tmp_path_factory.mktemp("mp3_core_check")
    cxx = _clangxx()
    if cxx is None:
        pytest.skip("no clang++ next to hipcc")
    trivial = work / "trivial.cpp"
    trivial.write_text("#include <vector>\nint main() { std::vector<int> v(4, 1); return v[3] - 1; }\n")
    r = subprocess.run([cxx, "-std=c++17", *SAN, str(trivial), "-o", str(work / "trivial")], capture_output=True)
    if r.returncode != 0 or subprocess.run([str(work / "trivial")], capture_output=True).returncode != 0:
        pytest.skip("a trivial sanitized program does not build and run here")
    exe = work / "mp3_core_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", *SAN,
                    str(ROOT / "tools" / "mp3_core_check.cpp"), "-o", str(exe)], check=True)
    return exe


def _run(exe, args):
    r = subprocess.run([str(exe), *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout.splitlines()


def test_fuzz_set_is_clean(checker, tmp_path):
    args = []
    for name, bad in mc.fuzz():
        p = tmp_path / f"{name}.mp3"
        p.write_bytes(bad)
        args.append(str(p))
    lines = _run(checker, args)
    assert len(lines) == len(mc.fuzz()) == 200
    assert sum("checksum" in ln for ln in lines) >= 150  # indexed and decoded


def test_stream_table_is_clean_and_checksums_repeat(checker, tmp_path):
    args = [str(ROOT / "tests" / "golden" / "mp3" / "invalid_keypress.mp3")]
    for name in mc.NAMES:
        p = tmp_path / f"{name}.mp3"
        p.write_bytes(mc.case(name)["data"])
        args.append(str(p))
    a = _run(checker, args)
    assert len(a) == len(args) and all("checksum" in ln for ln in a)
    assert a == _run(checker, args)
