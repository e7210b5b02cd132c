"""The device-resident evaluations on the banded direct back-end (fpsq_band_qp_*), as far as they can be checked without a
GPU: the header declares the entry points, the ctypes table types them with the same arity, the Python class is there."""
import inspect
import os
import re

import fps_amd  # noqa: F401
from fps_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> number of arguments in include/fpsq.h
ENTRIES = {
    "fpsq_band_qp_create": 5,
    "fpsq_band_qp_destroy": 1,
    "fpsq_band_qp_objgrad": 11,
    "fpsq_band_qp_hprod": 8,
    "fpsq_band_jac_mul": 6,
    "fpsq_band_set_input_stream": 3,
}


def _header_prototypes():
    text = open(os.path.join(ROOT, "include", "fpsq.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return {m.group(1): [a for a in m.group(2).split(",") if a.strip()]
            for m in re.finditer(r"\bint\s+(fpsq_\w+)\s*\(([^)]*)\)\s*;", text)}


def test_header_declares_the_band_qp_entries_and_the_binding_types_them():
    protos = _header_prototypes()
    table = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    for name, arity in ENTRIES.items():
        assert name in protos, f"{name} is not declared in include/fpsq.h"
        assert len(protos[name]) == arity, (name, protos[name])
        assert name in table, f"{name} is missing from _lib.SYMBOLS"
        res, args = table[name]
        assert res is _lib.C.c_int and len(args) == arity, (name, args)
    # the scalars travel by value as doubles, hessian_approx as an int32, phi comes back through a double*
    args = table["fpsq_band_qp_objgrad"][1]
    assert args[3:6] == [_lib.C.c_double] * 3 and args[7] == _lib.C.POINTER(_lib.C.c_double)
    args = table["fpsq_band_qp_hprod"][1]
    assert args[3:6] == [_lib.C.c_double] * 3 and args[6] is _lib.C.c_int32


def test_device_band_eqqp_is_exported_with_the_surface_fps_solve_device_uses():
    from fps_amd.device_qp import DeviceBandEqQP, DeviceEqQP

    for name in ("objgrad", "hprod", "jac_mul", "set_delta", "set_jacobian_values", "info", "close"):
        assert callable(getattr(DeviceBandEqQP, name)), name
    sig = inspect.signature(DeviceBandEqQP.__init__)
    assert list(sig.parameters)[1:] == ["qp", "sigma", "rho", "delta", "eta", "device", "ldlt_tol", "ldlt_r2"]
    assert list(inspect.signature(DeviceBandEqQP.objgrad).parameters) == list(inspect.signature(DeviceEqQP.objgrad).parameters)
    assert list(inspect.signature(DeviceBandEqQP.hprod).parameters) == list(inspect.signature(DeviceEqQP.hprod).parameters)
