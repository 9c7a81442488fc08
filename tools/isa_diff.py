"""Which kernels differ between two device listings of the same source.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -Iinclude <the source's extra flags> \
        --cuda-device-only -S audio-analysis_amd/csrc/aa_cnn.hip -o new.s
    python tools/isa_diff.py parent.s new.s

Per kernel (function label up to its .Lfunc_end) the whole instruction stream is
compared -- comments, blank lines and directives stripped, the function's index
taken out of its block labels -- together with the kernel descriptor's
next_free_vgpr / accum_offset / private_segment_fixed_size.  Prints one line
per kernel that differs or exists on one side only; exit status 1 if any.
"""
import re
import subprocess
import sys

KEEP = (".amdhsa_next_free_vgpr", ".amdhsa_accum_offset", ".amdhsa_private_segment_fixed_size")


def kernels(path):
    out, name = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, out[m.group(1)] = m.group(1), ([], {})
            continue
        if name is None:
            continue
        s = line.split(";")[0].strip()
        if s.startswith(".Lfunc_end"):
            name = None
        elif s.startswith(KEEP):
            out[name][1][s.split()[0][8:]] = s.split()[1]
        elif s and (not s.startswith(".") or s.startswith(".LBB")):
            out[name][0].append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    names = [n for n in a if n not in b or a[n] != b[n]] + [n for n in b if n not in a]
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    for n, d in zip(names, dem):
        d = re.sub(r"^void |\(.*", "", d)
        if n not in a or n not in b:
            print(f"only in {sys.argv[1 if n in a else 2]}: {d}")
            continue
        res = " ".join(f"{k} {a[n][1].get(k)}->{b[n][1].get(k)}" for k in a[n][1] if a[n][1][k] != b[n][1].get(k))
        print(f"differs: {len(a[n][0])} -> {len(b[n][0])} instructions {res} {d}")
    print(f"{len(names)} of {len(set(a) | set(b))} kernels differ")
    sys.exit(1 if names else 0)


if __name__ == "__main__":
    main()
