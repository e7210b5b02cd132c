"""fpsq_band_qp_objgrad_block (k penalty evaluations, or k QPs that differ in d and b, per pass over the cached banded factor),
as far as it can be checked without a GPU: the header declares it, the built library exports it, the ctypes table types it
with the same arity, a NULL handle is an argument error before any device call, the Python class has the method."""
import ctypes as C
import inspect
import os
import re

import fps_amd  # noqa: F401
from fps_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fpsq_band_qp_objgrad_block"
ARITY = 14


def _header_prototypes():
    text = open(os.path.join(ROOT, "include", "fpsq.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return {m.group(1): [a for a in m.group(2).split(",") if a.strip()]
            for m in re.finditer(r"\bint\s+(fpsq_\w+)\s*\(([^)]*)\)\s*;", text)}


def test_the_header_declares_the_entry_with_14_arguments():
    protos = _header_prototypes()
    assert NAME in protos, f"{NAME} is not declared in include/fpsq.h"
    assert len(protos[NAME]) == ARITY, protos[NAME]
    names = [re.sub(r"[^\w]", " ", a).split()[-1] for a in protos[NAME]]
    assert names == ["b", "qp", "k", "X", "D", "Bv", "sigma", "rho", "eta", "XK", "fx", "GX", "YS", "GS"]


def test_the_library_exports_the_entry_and_the_binding_types_it():
    lib = _lib.load()
    assert hasattr(lib, NAME), f"libfpsq.so does not export {NAME}"
    table = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    assert NAME in table, f"{NAME} is missing from _lib.SYMBOLS"
    res, args = table[NAME]
    assert res is C.c_int and len(args) == ARITY, args
    # k travels as an int32 behind the two handles; sigma, rho, eta by value as doubles; everything else is an address
    assert args[2] is C.c_int32 and args[6:9] == [C.c_double] * 3
    assert all(a is C.c_void_p for i, a in enumerate(args) if i != 2 and not 6 <= i < 9)


def test_a_null_handle_is_an_argument_error_without_a_device():
    lib = _lib.load()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    assert getattr(lib, NAME)(None, None, 1, p, None, None, 1e3, 1.0, 0.5, None, p, None, None, None) == -1
    assert getattr(lib, NAME)(None, None, 1, p, p, p, 1e3, 1.0, 0.5, p, p, p, p, p) == -1


def test_device_band_eqqp_has_the_method():
    from fps_amd.device_qp import DeviceBandEqQP, DeviceBorderedBandEqQP

    sig = inspect.signature(DeviceBandEqQP.objgrad_block)
    assert list(sig.parameters) == ["self", "X", "GX", "YS", "GS", "XK", "D", "B"]
    assert all(sig.parameters[p].default is None for p in ("GX", "YS", "GS", "XK", "D", "B"))
    assert DeviceBorderedBandEqQP.objgrad_block is DeviceBandEqQP.objgrad_block      # inherited, not overridden
