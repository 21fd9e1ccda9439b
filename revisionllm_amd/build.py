"""Build the HIP library (gfx950) in-tree with hipcc, in its two operand flavours: ``librevision_hip.so`` (fp16 operands, the default) and
``librevision_hip_bf16.so`` (bf16 operands) - the same sources compiled with ``-DRV_OP_F16=1`` / ``0`` (csrc/common.h).  No JIT cache: the
``.so`` files ship with the tree.  Only the entry points ``include/revision_hip.h`` declares are exported (``-fvisibility=hidden``).  After the two
flavours comes the companion library ``librevision_hip_ext.so`` (``include/revision_hip_ext.h``, the ``rvx_*`` entries): f32-only kernels, one build
for both flavours, linked with its own copy of ``error.o`` and its own version script; and, built the same way, the chain library
``librevision_hip_chain.so`` (``include/revision_hip_chain.h``, the ``rvc_*`` entries)."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(CSRC, "build")
FLAVOURS = {"f16": ("librevision_hip.so", "-DRV_OP_F16=1"), "bf16": ("librevision_hip_bf16.so", "-DRV_OP_F16=0")}
LIB = os.path.join(HERE, FLAVOURS["f16"][0])


def lib_path(flavour):
    return os.path.join(HERE, FLAVOURS[flavour][0])
SOURCES = ["error.hip", "init.hip", "gemm.hip", "gemm_pp.hip", "gemm_arows.hip", "gemm_rows.hip", "gemm_rows_p1.hip", "gemm_rows_p2.hip", "gemm_rows_p3.hip", "rowops.hip", "attention.hip", "sample.hip", "similarity.hip", "rank.hip", "propose.hip", "prefilter.hip", "gather.hip", "frames.hip", "frames_yuv.hip", "engine.hip"]
HEADERS = ["exports.map", "common.h", "kernels.h", "gemv_finish.h", "frames_common.h", "grounding.h", "window_select.h", "span_scores.h", "span_propose.h", "gemm_rows.hip", os.path.join("..", "..", "include", "revision_hip.h")]
EXT_LIB = os.path.join(HERE, "librevision_hip_ext.so")
EXT_SOURCES = ["prefilter_ext.hip"]          # compiled once (in the f16 object directory: nothing in them depends on the flavour)
EXT_SHARED = ["error.hip"]                   # objects of the f16 build linked in as well, their rv_* names local
EXT_HEADERS = ["exports_ext.map", os.path.join("..", "..", "include", "revision_hip_ext.h")]
CHAIN_LIB = os.path.join(HERE, "librevision_hip_chain.so")
CHAIN_SOURCES = ["prefilter_chain.hip", "spans_chain.hip", "valid_chain.hip", "refine_chain.hip", "anchors_chain.hip"]    # compiled once, as the companion's
CHAIN_HEADERS = ["exports_chain.map", os.path.join("..", "..", "include", "revision_hip_chain.h")]
#: the f32-only libraries: (path, own sources, headers beyond HEADERS, version script); each links EXT_SHARED's objects with their rv_* names local
COMPANIONS = [(EXT_LIB, EXT_SOURCES, EXT_HEADERS, "exports_ext.map"), (CHAIN_LIB, CHAIN_SOURCES, CHAIN_HEADERS, "exports_chain.map")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-fvisibility-inlines-hidden", "-Wall", "-Wno-unused-function",
         "-Wno-pass-failed"]


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build_library(force=False, verbose=False, flavours=("f16", "bf16")):
    """Compile every HIP translation unit for gfx950 in each flavour and link the shared libraries, then the companion and the chain library. Returns
    the default library's path."""
    hipcc = _hipcc()
    hdrs = [os.path.join(CSRC, h) for h in HEADERS]
    jobs = []
    ext_dir = os.path.join(OBJ, "f16")
    os.makedirs(ext_dir, exist_ok=True)
    for n, (_, sources, headers, _) in enumerate(COMPANIONS):
        ext_hdrs = hdrs + [os.path.join(CSRC, h) for h in headers]
        for s in sources + ([] if "f16" in flavours or n else EXT_SHARED):
            src = os.path.join(CSRC, s)
            obj = os.path.join(ext_dir, s.replace(".hip", ".o"))
            if force or _stale(obj, [src] + ext_hdrs):
                jobs.append([hipcc] + FLAGS + [FLAVOURS["f16"][1], "-DRV_TU=" + s.replace(".hip", ""), "-c", src, "-o", obj])
    for fl in flavours:
        os.makedirs(os.path.join(OBJ, fl), exist_ok=True)
        for s in SOURCES:
            src = os.path.join(CSRC, s)
            obj = os.path.join(OBJ, fl, s.replace(".hip", ".o"))
            if force or _stale(obj, [src] + hdrs):
                jobs.append([hipcc] + FLAGS + [FLAVOURS[fl][1], "-DRV_TU=" + s.replace(".hip", ""), "-c", src, "-o", obj])

    def run(cmd):
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed: %s\n%s" % (" ".join(cmd), r.stderr))
        if verbose and r.stderr:
            sys.stderr.write(r.stderr)

    with ThreadPoolExecutor(max_workers=int(os.environ.get("REVISION_BUILD_JOBS", "7"))) as ex:
        list(ex.map(run, jobs))
    for fl in flavours:
        objs = [os.path.join(OBJ, fl, s.replace(".hip", ".o")) for s in SOURCES]
        lib = lib_path(fl)
        if force or _stale(lib, objs):
            run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--version-script=" + os.path.join(CSRC, "exports.map"), "-o", lib] + objs)
    for lib, sources, _, script in COMPANIONS:
        ext_objs = [os.path.join(ext_dir, s.replace(".hip", ".o")) for s in sources + EXT_SHARED]
        if force or _stale(lib, ext_objs + [os.path.join(CSRC, script)]):
            run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--version-script=" + os.path.join(CSRC, script), "-o", lib] + ext_objs)
    return LIB


if __name__ == "__main__":
    fl = tuple(a for a in sys.argv[1:] if a in FLAVOURS) or tuple(FLAVOURS)
    print(build_library(force="--force" in sys.argv, verbose=True, flavours=fl))
