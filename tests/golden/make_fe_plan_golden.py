"""Record tests/golden/fe_plan_parent.json from the commit before the front-end
planner was split out (2fd07ce), whose plan existed only inside aa_fe_create.

    git worktree add /tmp/fe_parent 2fd07ce
    python tests/golden/make_fe_plan_golden.py /tmp/fe_parent

A scratch copy of that commit's aa_frontend.hip gets two edits, nothing else:
its upload helper writes each image to a file instead of the device (in upload
order: Hann, tw, tw2, CSR rows, CSR values, the 4096 image), and one accessor
is appended that reports what its own code decides -- the kernel by fe_small /
fe_fast4096, T, kmin, kmax, nnz, nfblk, the LDS bytes by its fe_lds_bytes*
and the grid by the arithmetic of its three launchers.  The copy is built with
aa_api.cpp into a library of its own and run on tests/fe_plan_cases.py.
No GPU is needed: with the upload gone, aa_fe_create makes no device call.
"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT / "audio-analysis_amd"), str(ROOT / "tests")]

UPLOAD_OLD = """    auto up = [](void** d, const void* h, size_t b) -> hipError_t {
        hipError_t e = hipMalloc(d, b);
        if (e != hipSuccess) return e;
        return hipMemcpy(*d, h, b, hipMemcpyHostToDevice);
    };"""
UPLOAD_NEW = """    int n_up = 0;
    auto up = [&n_up](void** d, const void* h, size_t b) -> hipError_t {
        char path[4096];
        snprintf(path, sizeof path, "%s/img%d.bin", getenv("AA_FE_RECORD_DIR"), n_up++);
        FILE* f = fopen(path, "wb");
        fwrite(h, 1, b, f);
        fclose(f);
        *d = nullptr;
        return hipSuccess;
    };"""
ACCESSOR = """
extern "C" int aa_fe_record_info(const void* plan, int32_t n_win, int64_t* out) {
    const FePlan& p = *static_cast<const FePlan*>(plan);
    size_t lds;
    int grid;
    if (fe_fast4096(p)) {
        lds = fe_lds_bytes4096(p);
        const int per_cu = std::max(1, std::min(2, (int)((160 * 1024) / lds)));
        grid = std::min((p.T * n_win + kWpb - 1) / kWpb, 256 * per_cu);
        grid = (grid + 7) & ~7;
    } else {
        lds = fe_small(p) ? fe_lds_bytes_small(p) : fe_lds_bytes(p);
        const int n_items = (fe_small(p) ? p.nfblk / kSmallWaves : p.nfblk) * n_win;
        const int per_cu = std::max(1, (int)((160 * 1024) / (lds + 256)));
        grid = std::min(n_items, 256 * per_cu);
    }
    const int64_t v[8] = {fe_small(p) ? 0 : fe_fast4096(p) ? 1 : 2, p.T, p.kmin, p.kmax, p.nnz, p.nfblk, (int64_t)lds, grid};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    return 0;
}
"""
FIELDS = ("kernel", "T", "kmin", "kmax", "nnz", "nparts", "lds_bytes", "grid")


def main():
    parent = Path(sys.argv[1])
    import fe_plan_cases as fc
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        src = (parent / "audio-analysis_amd/csrc/aa_frontend.hip").read_text()
        assert src.count(UPLOAD_OLD) == 1
        src = src.replace(UPLOAD_OLD, UPLOAD_NEW).replace('#include "aa_common.h"', '#include "aa_common.h"\n#include <cstdlib>', 1)
        csrc = tmp / "audio-analysis_amd/csrc"
        csrc.mkdir(parents=True)
        (tmp / "include").mkdir()
        for f in (parent / "audio-analysis_amd/csrc").glob("*.[hc]*"):
            (csrc / f.name).write_bytes(f.read_bytes())
        (tmp / "include/aa.h").write_bytes((parent / "include/aa.h").read_bytes())
        (csrc / "aa_frontend.hip").write_text(src + ACCESSOR)
        so = tmp / "libfe_parent.so"
        subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950",
                        f"-I{tmp / 'include'}", str(csrc / "aa_frontend.hip"), str(csrc / "aa_api.cpp"), "-o", str(so)],
                       check=True)
        rec = tmp / "rec"
        rec.mkdir()
        os.environ["AA_FE_RECORD_DIR"] = str(rec)
        L = C.CDLL(str(so))
        L.aa_last_error.restype = C.c_char_p
        L.aa_fe_workspace_bytes.restype = C.c_size_t
        L.aa_fe_workspace_bytes.argtypes = [C.c_void_p, C.c_int32]
        for f in ("aa_fe_n_frames", "aa_fe_destroy"):
            getattr(L, f).argtypes = [C.c_void_p]
        L.aa_fe_stage_info.argtypes = [C.c_void_p, C.c_int32, C.c_char_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.aa_fe_record_info.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]

        def create(cfg, fb, h):
            for f in rec.glob("img*.bin"):
                f.unlink()
            return L.aa_fe_create(cfg, C.c_void_p(fb), h)

        def info(h, n):
            v = (C.c_int64 * 8)()
            assert L.aa_fe_record_info(h, n, v) == 0
            return dict(zip(FIELDS, map(int, v)))

        def image(h, w):
            f = rec / f"img{w}.bin"
            return f.read_bytes() if f.exists() else b""

        commit = subprocess.run(["git", "-C", str(parent), "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
        out = {"parent_commit": commit or "2fd07ce",
               "cases": {k: fc.describe(L, create, *v, info, image) for k, v in fc.cases().items()},
               "refusals": {k: fc.describe(L, create, *v, info, image) for k, v in fc.refusals().items()}}
    (Path(__file__).parent / "fe_plan_parent.json").write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
