"""Host sanitizer run of the graph planner (no GPU, nothing loaded into Python):
writes every node table and rejection of tests/graph_tables.py to files,
builds tools/graph_plan_check.cpp with aa_graph.hip and aa_api.cpp under host
ASan + UBSan, and runs it over the files.

    python tools/graph_plan_check.py [WORKDIR]
"""
import ctypes as C
import struct
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "audio-analysis_amd"), str(ROOT / "tests")]


def write_tables(out):
    import graph_tables as gt
    files = []
    todo = [(name, t, prec, nofuse) for name, t in gt.tables().items() for prec in gt.PRECS for nofuse in (0, 1)]
    todo += [("reject_" + name, t, prec, 0) for name, (t, prec) in gt.rejections().items()]
    for name, (nodes, blob, (H, W, Cin)), prec, nofuse in todo:
        p = out / f"{name}_{prec}_{nofuse}.tab"
        p.write_bytes(struct.pack("<6iq", len(nodes), H, W, Cin, gt.PRECS[prec], nofuse, blob.size) +
                      C.string_at(nodes, C.sizeof(nodes)) + blob.tobytes())
        files.append(str(p))
    return files


def main():
    from aa_amd import _build
    work = Path(sys.argv[1]) if len(sys.argv) > 1 else Path(tempfile.mkdtemp(prefix="graph_plan_check_"))
    work.mkdir(parents=True, exist_ok=True)
    files = write_tables(work)
    exe = work / "graph_plan_check"
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-Xarch_host", "-fno-omit-frame-pointer"]
    cmd = [_build.hipcc(), "-O1", "-g", "-std=c++17", f"--offload-arch={_build.ARCH}", f"-I{_build.INCLUDE}",
           "-Wno-unused-function", *san, *_build.EXTRA_FLAGS["aa_graph.hip"], str(ROOT / "tools" / "graph_plan_check.cpp"),
           str(_build.CSRC / "aa_graph.hip"), str(_build.CSRC / "aa_api.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True)
    r = subprocess.run([str(exe), *files])
    print("graph_plan_check:", "clean" if r.returncode == 0 else f"FAILED ({r.returncode})")
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
