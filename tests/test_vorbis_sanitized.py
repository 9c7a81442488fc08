"""The device Vorbis decoder's index and core under host ASan + UBSan:
tools/vorbis_core_check.cpp (stand-alone, its own main; nothing is loaded into
Python) is built with the sanitizers and run over the stream table and the
seeded damaged streams of tests/vorbis_cases.py -- each one indexed, decoded
through the core and compared with the host decoder inside the program.  Exit
status 0 and no sanitizer report."""
import shutil
import subprocess
from pathlib import Path

import pytest

import vorbis_cases as vc

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
    work = tmp_path_factory.mktemp("vorbis_core_check")
    cxx = _clangxx()
    if cxx is None:
        pytest.skip("no clang++ next to hipcc")
    trivial = work / "trivial.cpp"
    trivial.write_text("#include <vector>\nint main() { std::vector<int> v(4, 1); return v[3] - 1; }\n")
    r = subprocess.run([cxx, "-std=c++17", *SAN, str(trivial), "-o", str(work / "trivial")], capture_output=True)
    if r.returncode != 0 or subprocess.run([str(work / "trivial")], capture_output=True).returncode != 0:
        pytest.skip("a trivial sanitized program does not build and run here")
    exe = work / "vorbis_core_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", *SAN, str(ROOT / "tools" / "vorbis_core_check.cpp"), "-o",
                    str(exe)], check=True)
    return exe


def _run(exe, args):
    r = subprocess.run([str(exe), *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout.splitlines()


def test_fuzz_set_is_clean(checker, tmp_path):
    args = []
    for name, bad in vc.fuzz():
        p = tmp_path / f"{name}.ogg"
        p.write_bytes(bad)
        args.append(str(p))
    lines = _run(checker, args)
    assert len(lines) == len(vc.fuzz()) == 200
    assert sum("checksum" in ln for ln in lines) >= 190  # decoded, and equal to the host decoder inside


def test_stream_table_is_clean_and_checksums_repeat(checker, tmp_path):
    args = []
    for name, data in vc.table().items():
        p = tmp_path / f"{name}.ogg"
        p.write_bytes(data)
        args.append(str(p))
    a = _run(checker, args)
    assert len(a) == len(args)
    for name, ln in zip(vc.table(), a):
        assert ("index 3" in ln) if name == vc.FLOOR0 else ("checksum" in ln), ln
    assert a == _run(checker, args)
