"""Instruction classes of one aa_cnn.hip kernel, per barrier-delimited phase.

    python tools/isa_count.py <mangled-name-substring> [--asm LISTING] [--list]

Compiles audio-analysis_amd/csrc/aa_cnn.hip to assembly with the flags
aa_amd/_build.py builds it with (or reads --asm, a listing made earlier) and
prints, for the first kernel whose mangled name contains the substring, one row
per phase -- the instructions between two s_barrier in listing order:

    mfma   lines starting v_mfma
    valu   other lines starting v_
    ds     lines starting ds_
    vmem   lines starting buffer_ or global_
    v_pk   lines starting v_pk_ (a subset of valu)
    maxxx  v_max_f32 whose two sources are the same register (a canonicalising
           max; a subset of valu)

The counts are static: a loop body counts once, an untaken branch counts too.
"""
import argparse
import importlib.util
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
COLS = ["mfma", "valu", "ds", "vmem", "v_pk", "maxxx"]


def compile_listing(out: Path) -> None:
    spec = importlib.util.spec_from_file_location("_aa_build", ROOT / "audio-analysis_amd" / "aa_amd" / "_build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    cmd = [b.hipcc(), "-O3", "-std=c++17", "-fPIC", f"--offload-arch={b.ARCH}", f"-I{b.INCLUDE}", "-Wall",
           "-Wno-unused-function", *b.EXTRA_FLAGS.get("aa_cnn.hip", []), "--cuda-device-only", "-S",
           str(b.CSRC / "aa_cnn.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(f"hipcc failed:\n{r.stderr}")
    v = subprocess.run([b.hipcc(), "--version"], capture_output=True, text=True).stdout.splitlines()
    print("compiler: " + " | ".join(l.strip() for l in v[:2]))


def kernels(lines):
    """(name, first body line, end line) of every function in the listing"""
    out, start, name = [], None, None
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\w+):", l)
        if m and start is None:
            name, start = m.group(1), i + 1
        elif start is not None and l.startswith(".Lfunc_end"):
            out.append((name, start, i))
            start = None
    return out


def count(body):
    phases = [dict.fromkeys(COLS, 0)]
    for l in body:
        s = l.split(";")[0].strip()
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        op = s.split()[0]
        c = phases[-1]
        if op.startswith("s_barrier"):
            phases.append(dict.fromkeys(COLS, 0))
        elif op.startswith("v_mfma"):
            c["mfma"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
            if op.startswith("v_pk_"):
                c["v_pk"] += 1
            if op.startswith("v_max_f32"):
                a = [x.strip() for x in s[len(op):].split(",")]
                if len(a) == 3 and a[1] == a[2]:
                    c["maxxx"] += 1
        elif op.startswith("ds_"):
            c["ds"] += 1
        elif op.startswith(("buffer_", "global_")):
            c["vmem"] += 1
    return phases


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("kernel", nargs="?", default="", help="substring of the kernel's mangled name")
    ap.add_argument("--asm", help="read this listing instead of compiling")
    ap.add_argument("--list", action="store_true", help="print the mangled names that match and exit")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as td:
        path = Path(a.asm) if a.asm else Path(td) / "aa_cnn.s"
        if not a.asm:
            compile_listing(path)
        lines = path.read_text().split("\n")
    ks = [k for k in kernels(lines) if a.kernel in k[0]]
    if a.list:
        print("\n".join(k[0] for k in ks))
        return
    if not ks:
        sys.exit(f"no kernel whose name contains {a.kernel!r}")
    name, lo, hi = ks[0]
    print(name)
    phases = count(lines[lo:hi])
    print(f"{'phase':<8}" + "".join(f"{c:>7}" for c in COLS))
    tot = dict.fromkeys(COLS, 0)
    for i, p in enumerate(phases):
        print(f"{i:<8}" + "".join(f"{p[c]:>7}" for c in COLS))
        for c in COLS:
            tot[c] += p[c]
    print(f"{'total':<8}" + "".join(f"{tot[c]:>7}" for c in COLS))


if __name__ == "__main__":
    main()
