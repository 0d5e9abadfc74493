"""`-m "not gpu"`: the host decision of csrc/ks_stencil_geom.hpp -- "the masks of this stencil-mask layout are the box rule of an
nx x ny x nz grid", which lets the z-marching stencil product derive its masks from the row number -- in a stand-alone host program
under the address and undefined-behaviour sanitizers (tests/stencil_geom_check.cpp): true for 4x3x5, 7x2x2 and 2x2x2 box masks, false
for a cleared bit, an extra bit, a periodic wrap, deltas in another order, a cut last plane and a 5-point dictionary."""
import os
import shutil
import subprocess

import pytest

from __graft_entry__ import ROOT


def _host_compiler():
    for cand in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        cc = shutil.which(cand)
        if cc:
            return cc
    return None


def test_geometry_header_alone_under_the_sanitizers(tmp_path):
    cc = _host_compiler()
    if cc is None:
        pytest.skip("no host C++ compiler (g++, c++, clang++) found")
    exe = str(tmp_path / "stencil_geom_check")
    src = os.path.join(ROOT, "tests", "stencil_geom_check.cpp")
    # (GCC links the sanitizer runtimes as shared libraries unless told otherwise, and a shared ASan runtime refuses to start behind
    # any other preloaded library; clang links them statically)
    gnu = "clang" not in subprocess.run([cc, "--version"], capture_output=True, text=True).stdout
    b = subprocess.run([cc, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
                       + (["-static-libasan", "-static-libubsan"] if gnu else []) + [src, "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout[-3000:] + b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "STENCIL_GEOM_CHECK_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
