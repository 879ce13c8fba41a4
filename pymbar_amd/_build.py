"""Build libmbar_hip.so (gfx950 only) in-tree with hipcc.  Used by ``__graft_entry__.build()``.

The shared object is git-ignored but travels with the working tree; nothing is compiled at
import time and there is no fallback if it is missing (see ``pymbar_amd/_lib.py``).
"""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(CSRC, "libmbar_hip.so")
# Kernel families in separate translation units (compiled in parallel: ~40 s on 8 cores instead of 2.5 min for the one file of
# rounds 1-3; an edit to one family recompiles that family: a source depends on the headers it includes, see source_deps).
KERNEL_SOURCES = ["mbar_k_eval.hip", "mbar_k_gram.hip", "mbar_k_quad.hip", "mbar_k_pmode.hip", "mbar_k_fused.hip", "mbar_k_loop.hip",
                  "mbar_k_rows.hip", "mbar_k_kde.hip", "mbar_k_acf.hip", "mbar_k_bar.hip", "mbar_k_bspline.hip", "mbar_k_batch.hip", "mbar_k_hist.hip",
                  "mbar_k_scan.hip", "mbar_k_family.hip"]
HOST_SOURCES = ["mbar_capi.cpp", "mbar_eval.cpp", "mbar_rows.cpp", "mbar_ext.cpp", "mbar_loops.cpp", "mbar_loop_device.cpp",
                "mbar_loop_host.cpp", "mbar_comm.cpp", "mbar_host.cpp", "mbar_kde.cpp", "mbar_acf.cpp", "mbar_bar.cpp", "mbar_bspline.cpp", "mbar_batch.cpp", "mbar_hist.cpp",
                "mbar_scan.cpp"]
SOURCES = KERNEL_SOURCES + HOST_SOURCES
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"]
# (A/B builds of kernel variants kept behind macros: MBAR_EXTRA_HIPCC_FLAGS="-DMBAR_..." python -m pymbar_amd._build --force)
FLAGS += os.environ.get("MBAR_EXTRA_HIPCC_FLAGS", "").split()


_INCLUDE = re.compile(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', re.M)


def source_deps(src):
    """The files a source of csrc is built from: itself and the transitive closure of its ``#include "..."`` lines (headers, .inc
    tables, include/mbar_hip.h), each path taken relative to the including file.  Absolute, normalised paths, the source first."""
    todo = [os.path.normpath(os.path.join(CSRC, src))]
    seen = []
    while todo:
        path = todo.pop()
        if path in seen:
            continue
        seen.append(path)
        with open(path) as fh:
            text = fh.read()
        todo += [os.path.normpath(os.path.join(os.path.dirname(path), inc)) for inc in _INCLUDE.findall(text)]
    return seen


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _compile(src):
    obj = os.path.join(CSRC, os.path.splitext(src)[0] + ".o")
    if _stale(obj, source_deps(src)):
        cmd = [HIPCC] + FLAGS + ["-x", "hip", "-c", os.path.join(CSRC, src), "-o", obj]
        subprocess.run(cmd, check=True, cwd=CSRC)
    return obj


def build_library(force=False, verbose=True):
    """Compile the HIP sources for gfx950 and link ``csrc/libmbar_hip.so``."""
    if force:
        for f in os.listdir(CSRC):
            if f.endswith((".o", ".so")):
                os.remove(os.path.join(CSRC, f))
    if not force and not _stale(LIB, [d for src in SOURCES for d in source_deps(src)]):
        return LIB
    # (MAX_JOBS: what a build may use where the machine reports more processors than the job has been given)
    with ThreadPoolExecutor(max_workers=min(len(SOURCES), int(os.environ.get("MAX_JOBS", 16)))) as ex:
        objs = list(ex.map(_compile, SOURCES))
    cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs + ["-ldl"]
    subprocess.run(cmd, check=True, cwd=CSRC)
    if verbose:
        print(f"built {LIB}", file=sys.stderr)
    return LIB


if __name__ == "__main__":
    build_library(force="--force" in sys.argv)
