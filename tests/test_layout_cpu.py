"""The host-built sparse layouts (csrc/fpsq_layout.h: row blocks, 16-bit columns, padded / column-sorted / shared-value
blocks of A', the row-group copy of A, the dependence ranges of the one-launch iteration) checked without a GPU:
tests/host/layout_check.cpp builds every layout for a list of small cases and decodes it the way the kernel that reads it
does.  A wrong index there would be an out-of-range gather on the device, so the program also runs under the address and
undefined-behaviour sanitizers -- as a stand-alone executable; nothing sanitized is loaded into this process."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "layout_check.cpp")
INC = os.path.join(ROOT, "fletcherpenaltysolver.jl_amd", "csrc")


def _compiler():
    for c in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    raise RuntimeError("no host C++ compiler found")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_every_layout_decodes_to_the_csr(tmp_path, flags):
    exe = str(tmp_path / "layout_check")
    build = subprocess.run([_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", INC, "-o", exe, SRC],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "0 failure(s)" in run.stdout


def test_the_layout_header_is_plain_host_code():
    """no device runtime, no handle, no environment, no device allocation: what makes the builders testable here"""
    text = open(os.path.join(INC, "fpsq_layout.h")).read()
    for word in ("hip", "dalloc", "getenv", "handle"):
        assert word not in text.lower(), word
    check = subprocess.run([_compiler(), "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", INC, "-x", "c++", "-"],
                           input='#include "fpsq_layout.h"\n', capture_output=True, text=True)
    assert check.returncode == 0, check.stderr
