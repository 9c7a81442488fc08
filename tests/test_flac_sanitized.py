"""The device FLAC decoder's core and indexer under host ASan + UBSan:
tools/flac_core_check.cpp (stand-alone, its own main; nothing is loaded into
Python) is built with the sanitizers and run over the seeded damaged streams
of tests/flac_cases.py -- each one indexed as it is, and decoded through its
undamaged original's table -- and over the feature table.  Exit status 0 and
no sanitizer report."""
import shutil
import subprocess
from pathlib import Path

import pytest

import flac_cases as fc

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
    work = tmp_path_factory.mktemp("flac_core_check")
    cxx = _clangxx()
    if cxx is None:
        pytest.skip("no clang++ next to hipcc")
    trivial = work / "trivial.cpp"
    trivial.write_text("#include <vector>\nint main() { std::vector<int> v(4, 1); return v[3] - 1; }\n")
    r = subprocess.run([cxx, "-std=c++17", *SAN, str(trivial), "-o", str(work / "trivial")], capture_output=True)
    if r.returncode != 0 or subprocess.run([str(work / "trivial")], capture_output=True).returncode != 0:
        pytest.skip("a trivial sanitized program does not build and run here")
    exe = work / "flac_core_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", *SAN, str(ROOT / "tools" / "flac_core_check.cpp"), "-o", str(exe)],
                   check=True)
    return exe


def _run(exe, args):
    r = subprocess.run([str(exe), *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout.splitlines()


def test_fuzz_set_is_clean(checker, tmp_path):
    args, originals = [], {}
    for name, mode, bad, good, k in fc.fuzz():
        p = tmp_path / f"{name}.flac"
        p.write_bytes(bad)
        g = originals.get(good)
        if g is None:
            g = originals[good] = tmp_path / f"good{len(originals)}.flac"
            g.write_bytes(good)
        args += [str(p), f"{p}@{g}"]
    lines = _run(checker, args)
    assert len(lines) == 2 * len(fc.fuzz()) == 600
    # through the original's table every stream is decoded, none refused
    assert all("checksum" in ln for ln in lines[1::2])


def test_feature_table_is_clean_and_checksums_repeat(checker, tmp_path):
    args = []
    for name, data, _ in fc.table():
        p = tmp_path / f"{name}.flac"
        p.write_bytes(data)
        args.append(str(p))
    a = _run(checker, args)
    assert len(a) == len(args) and all("checksum" in ln for ln in a)
    assert a == _run(checker, args)
