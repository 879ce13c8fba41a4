"""The dependencies the build reads from the sources (``pymbar_amd._build.source_deps``: the transitive closure of the
``#include "..."`` lines) and the layering of the headers of ``pymbar_amd/csrc`` that they show: a header per kernel family, the
sweep and scan device helpers out of the other kernels' way, the handle layer below the context.  No compiler runs here."""
import os
import re

import pytest

from pymbar_amd import _build

CSRC = _build.CSRC
BACKENDS = ("kde", "acf", "bar", "bspline", "batch")  # the handles that are no context: mbar_<name>.cpp + mbar_k_<name>.hip


def closure(src):
    """base names of the files ``src`` is built from (the sources of csrc have distinct base names, include/mbar_hip.h too)"""
    return {os.path.basename(p) for p in _build.source_deps(src)}


def test_every_include_resolves():
    pat = re.compile(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', re.M)
    seen = 0
    for fn in sorted(os.listdir(CSRC)):
        if not fn.endswith((".h", ".inc", ".hip", ".cpp")):
            continue
        with open(os.path.join(CSRC, fn)) as fh:
            for inc in pat.findall(fh.read()):
                seen += 1
                assert os.path.isfile(os.path.join(CSRC, inc)), (fn, inc)
    assert seen >= len(_build.SOURCES)  # every source includes at least one project header
    for src in _build.SOURCES:
        deps = _build.source_deps(src)
        assert deps[0] == os.path.join(CSRC, src) and all(os.path.isabs(p) and os.path.isfile(p) for p in deps), src
        assert "mbar_hip.h" in closure(src), src


def test_every_header_is_in_some_closure():
    used = set().union(*(closure(src) for src in _build.SOURCES))
    headers = {fn for fn in os.listdir(CSRC) if fn.endswith((".h", ".inc"))}
    assert headers and headers <= used, sorted(headers - used)


@pytest.mark.parametrize("name", ["kde", "acf", "bar", "bspline", "batch", "hist", "rows"])
def test_other_kernels_see_no_sweep_or_scan_device_code(name):
    c = closure("mbar_k_%s.hip" % name)
    assert "mbar_sweep_device.h" not in c and "mbar_scan_device.h" not in c, sorted(c)


@pytest.mark.parametrize("name", BACKENDS)
def test_backends_see_neither_context_nor_solver_interface(name):
    c = closure("mbar_%s.cpp" % name)
    assert "mbar_ctx.h" not in c and "mbar_internal.h" not in c, sorted(c)
    assert "mbar_handle.h" in c and "mbar_%s.h" % name in c


@pytest.mark.parametrize("name", BACKENDS)
def test_backend_header_stays_in_its_family(name):
    own = {"mbar_%s.cpp" % name, "mbar_k_%s.hip" % name}
    assert own <= set(_build.SOURCES)
    for src in _build.SOURCES:
        assert ("mbar_%s.h" % name in closure(src)) == (src in own), (name, src)


def test_every_kernel_source_sees_the_device_helpers():
    assert len(_build.KERNEL_SOURCES) == 15
    for src in _build.KERNEL_SOURCES:
        assert {"mbar_device.h", "exp2_table.inc", "log_table.inc"} <= closure(src), src
