"""The sparse symmetric objective Hessian on the ITERATIVE device eq-QP (fpsq_qp_create_csr, DeviceSparseHessianEqQP), as far
as it can be checked without a GPU: the ABI declaration and its binding, the guards of the two Python classes (before the library
is touched), and the host-side check / split Q = diag(q) + R that both create entries share (csrc/fpsq_qcsr.h), driven by the
stand-alone tests/host/qcsr_check.cpp -- plain and under the address / undefined-behaviour sanitizers; nothing sanitized is loaded
into this process."""
import os
import re
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import fps_amd  # noqa: E402,F401
from fps_amd import _lib, problems  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "qcsr_check.cpp")
INC = os.path.join(ROOT, "fletcherpenaltysolver.jl_amd", "csrc")


def _base():
    return problems.pde_control_like(n=400, m=40, per_row=8, window=64)


def _compiler():
    for c in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    raise RuntimeError("no host C++ compiler found")


def test_header_declares_qp_create_csr_and_the_binding_types_it():
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "fpsq.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+fpsq_qp_create_csr\s*\(([^)]*)\)\s*;", text)
    assert m, "fpsq_qp_create_csr is not declared in include/fpsq.h"
    args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
    assert len(args) == 7, args
    assert args[0].startswith("fpsq_handle ")
    assert args[1].startswith("const int32_t *") and args[2].startswith("const int32_t *")
    assert all(a.startswith("const double *") for a in args[3:6])
    assert args[6].startswith("fpsq_qp *")
    table = {name: (res, a) for name, res, a in _lib.SYMBOLS}
    assert "fpsq_qp_create_csr" in table
    res, a = table["fpsq_qp_create_csr"]
    assert res is _lib.C.c_int and len(a) == 7 and a[0] is _lib.C.c_void_p and a[6] == _lib.C.POINTER(_lib.C.c_void_p)
    # the banded entry has the same shape: one contract
    assert table["fpsq_band_qp_create_csr"] == table["fpsq_qp_create_csr"]


def test_the_guards_come_before_the_library_is_touched(monkeypatch):
    from fps_amd.device_qp import DeviceEqQP, DeviceSparseHessianEqQP

    def no_load():
        raise AssertionError("the guard must come before the library is touched")

    monkeypatch.setattr(_lib, "load", no_load)
    qp = problems.with_sparse_hessian(_base(), 1, 7)
    with pytest.raises(ValueError, match="DeviceBandEqQP") as info:
        DeviceEqQP(qp)
    assert "DeviceSparseHessianEqQP" in str(info.value)
    assert issubclass(DeviceSparseHessianEqQP, DeviceEqQP)
    for kw in ({"comm": ("local", None, 0)}, {"halo": (0, 0)}, {"comm": ("rccl", 1, 0, bytes(128)), "halo": (0, 0)}):
        for q in (qp, _base()):        # with and without hess_vals: the class is single-GPU
            with pytest.raises(ValueError, match="single-GPU"):
                DeviceSparseHessianEqQP(q, **kw)
    # (past the guards the class does reach for the library)
    with pytest.raises(AssertionError, match="before the library"):
        DeviceSparseHessianEqQP(qp)


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_the_check_and_split_of_a_sparse_hessian(tmp_path, flags):
    exe = str(tmp_path / "qcsr_check")
    build = subprocess.run([_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", INC, "-o", exe, SRC],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "0 failure(s)" in run.stdout
    for case in ("unsorted columns", "absent diagonal", "empty matrix", "stored zeros"):
        assert re.search(rf"{case}\s+accepted", run.stdout), case
    for case in ("unsymmetric value", "unsymmetric pattern", "duplicate", "column n", "column -1"):
        assert re.search(rf"{re.escape(case)}\s+refused", run.stdout), case


def test_the_shared_headers_are_plain_host_code():
    """no device runtime, no handle, no environment: what makes the check testable here, and what lets both units include it"""
    for name in ("fpsq_qcsr.h", "fpsq_lanegroup.h"):
        text = open(os.path.join(INC, name)).read()
        code = re.sub(r"//.*", "", text)
        for word in ("hip", "dalloc", "getenv", "handle"):
            assert word not in code.lower(), (name, word)
        check = subprocess.run([_compiler(), "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", INC, "-x", "c++", "-"],
                               input=f'#include "{name}"\n', capture_output=True, text=True)
        assert check.returncode == 0, check.stderr
    # one rule for the lanes per row, one check of Q: neither back-end keeps a copy
    for unit in ("fpsq_band.hip", "fpsq.hip"):
        text = open(os.path.join(INC, unit)).read()
        assert "qcsr_check_split(" in text and "has no transpose" not in text, unit
    assert "inline int lane_group" not in open(os.path.join(INC, "fpsq_direct.hip.h")).read()
