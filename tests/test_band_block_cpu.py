"""The block entries of the banded direct back-end (fpsq_band_solve_two_least_squares_block, fpsq_band_qp_hprod_block), as far
as they can be checked without a GPU: the header declares them, the built library exports them, the ctypes table types them
with the same arity, a NULL handle is an argument error before any device call, the Python class has the methods."""
import ctypes as C
import inspect
import os
import re

import fps_amd  # noqa: F401
from fps_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> number of arguments in include/fpsq.h
ENTRIES = {
    "fpsq_band_solve_two_least_squares_block": 8,
    "fpsq_band_qp_hprod_block": 9,
}


def _header_prototypes():
    text = open(os.path.join(ROOT, "include", "fpsq.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return {m.group(1): [a for a in m.group(2).split(",") if a.strip()]
            for m in re.finditer(r"\bint\s+(fpsq_\w+)\s*\(([^)]*)\)\s*;", text)}


def test_the_library_exports_the_block_entries_and_the_binding_types_them():
    lib = _lib.load()
    protos = _header_prototypes()
    table = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    for name, arity in ENTRIES.items():
        assert name in protos, f"{name} is not declared in include/fpsq.h"
        assert len(protos[name]) == arity, (name, protos[name])
        assert hasattr(lib, name), f"libfpsq.so does not export {name}"
        assert name in table, f"{name} is missing from _lib.SYMBOLS"
        res, args = table[name]
        assert res is C.c_int and len(args) == arity, (name, args)
    # k travels as an int32 behind the handle(s); the scalars by value as doubles, hessian_approx as an int32
    assert table["fpsq_band_solve_two_least_squares_block"][1][1] is C.c_int32
    args = table["fpsq_band_qp_hprod_block"][1]
    assert args[2] is C.c_int32 and args[4:7] == [C.c_double] * 3 and args[7] is C.c_int32


def test_a_null_handle_is_an_argument_error_without_a_device():
    lib = _lib.load()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    assert lib.fpsq_band_solve_two_least_squares_block(None, 1, p, p, p, p, p, p) == -1
    assert lib.fpsq_band_qp_hprod_block(None, None, 1, p, 1e3, 1.0, 0.5, 2, p) == -1


def test_device_band_eqqp_has_the_block_methods():
    from fps_amd.device_qp import DeviceBandEqQP

    assert list(inspect.signature(DeviceBandEqQP.hprod_block).parameters) == ["self", "V", "HV", "hessian_approx"]
    assert inspect.signature(DeviceBandEqQP.hprod_block).parameters["hessian_approx"].default == 2
    assert list(inspect.signature(DeviceBandEqQP.solve_two_least_squares_block).parameters) == [
        "self", "rhs1", "rhs2", "p1", "q1", "p2", "q2"]
