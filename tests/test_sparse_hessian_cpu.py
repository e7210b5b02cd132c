"""The sparse symmetric objective Hessian of the eq-QP model (fpsq_band_qp_create_csr, EqQP.hess_*, with_sparse_hessian), as
far as it can be checked without a GPU: the ABI declaration, the generator, the host mirror against the exact scipy
reference (tests/sparse_hessian_ref.py), and the guards."""
import dataclasses
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import fps_amd  # noqa: E402,F401
from fps_amd import _lib, nlpmodels, problems  # noqa: E402
from fps_amd.penalty_nlp import FletcherPenaltyNLP  # noqa: E402
from oracle_qdsolver import OracleQDSolver  # noqa: E402
from sparse_hessian_ref import SparseHessianRef  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA = 1e3


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def _base():
    return problems.pde_control_like(n=400, m=40, per_row=8, window=64)


def test_header_declares_create_csr_and_the_binding_types_it():
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "fpsq.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+fpsq_band_qp_create_csr\s*\(([^)]*)\)\s*;", text)
    assert m, "fpsq_band_qp_create_csr is not declared in include/fpsq.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 7, args
    assert args[1].startswith("const int32_t *") and args[2].startswith("const int32_t *") and args[3].startswith("const double *")
    table = {name: (res, a) for name, res, a in _lib.SYMBOLS}
    assert "fpsq_band_qp_create_csr" in table
    res, a = table["fpsq_band_qp_create_csr"]
    assert res is _lib.C.c_int and len(a) == 7 and a[6] == _lib.C.POINTER(_lib.C.c_void_p)


@pytest.mark.parametrize("hw", [1, 4])
def test_with_sparse_hessian_is_symmetric_dominant_and_deterministic(hw):
    qp = _base()
    sq = problems.with_sparse_hessian(qp, hw, 99)
    Q = sq.hess_csr()
    assert Q.shape == (qp.n, qp.n) and sq.hess_rowptr.dtype == np.int32 and sq.hess_colind.dtype == np.int32
    assert (Q != Q.T).nnz == 0
    dense = Q.toarray()
    i, j = np.nonzero(dense)
    assert np.max(np.abs(i - j)) == hw                                   # banded, and the outermost diagonal is populated
    diag = np.diag(dense)
    off = np.abs(dense).sum(axis=1) - np.abs(diag)
    assert np.all(diag > off) and np.all(diag > 0)                       # strictly diagonally dominant: SPD
    assert np.array_equal(sq.qdiag, diag)
    rows_off = np.diff(sq.hess_rowptr) - 1
    assert np.any(rows_off == 0) and np.max(rows_off) > hw               # empty rows of R next to two-sided ones
    again = problems.with_sparse_hessian(qp, hw, 99)
    assert np.array_equal(again.hess_vals, sq.hess_vals) and np.array_equal(again.hess_colind, sq.hess_colind)
    assert not np.array_equal(problems.with_sparse_hessian(qp, hw, 100).hess_vals, sq.hess_vals)
    # the Jacobian, d, b and the points are the base QP's; dataclasses.replace keeps the Hessian
    assert sq.vals is qp.vals and sq.d is qp.d and sq.b is qp.b
    moved = dataclasses.replace(sq, b=sq.b + 1.0)
    assert moved.hess_vals is sq.hess_vals and (moved.hess_csr() != Q).nnz == 0
    # the diagonal model answers hess_csr too
    assert qp.hess_vals is None and (qp.hess_csr() != __import__("scipy.sparse").sparse.diags(qp.qdiag).tocsr()).nnz == 0


@pytest.mark.parametrize("rho,eta", [(0.0, 0.0), (1.0, 0.5)])
@pytest.mark.parametrize("hw", [1, 4])
def test_host_mirror_with_a_sparse_hessian_matches_the_exact_reference(oracle, hw, rho, eta):
    qp = problems.with_sparse_hessian(_base(), hw, 7)
    ref = SparseHessianRef(qp, 0.0)
    model = nlpmodels.EqQPModel(qp)
    x, xk = qp.x, qp.xhat
    v = np.random.default_rng(0).standard_normal(qp.n)
    want = ref.objgrad(x, SIGMA, rho, eta, xk)
    want_hv = ref.hprod(v, SIGMA, rho, eta)
    for ha in (2, 1):
        fp = FletcherPenaltyNLP(model, SIGMA, rho, 0.0, ha, qds=OracleQDSolver(model, 0.0))
        fp.eta = eta
        fp.xk[:] = xk
        fx, gx = fp.objgrad(x)
        errs = {"fx": abs(fx - want["fx"]) / abs(want["fx"]), "gx": _rel(gx, want["gx"]), "ys": _rel(fp.ys, want["ys"]),
                "Hv": _rel(fp.hprod(x, v), want_hv)}
        print(f"\nhw={hw} rho={rho} eta={eta} Val({ha}): {errs}")
        assert all(e < 1e-10 for e in errs.values()), errs
    # the Hessian matters: the diagonal part alone is far from the reference
    diag_only = dataclasses.replace(qp, hess_rowptr=None, hess_colind=None, hess_vals=None)
    fd = FletcherPenaltyNLP(nlpmodels.EqQPModel(diag_only), SIGMA, rho, 0.0, 2, qds=OracleQDSolver(model, 0.0))
    assert _rel(fd.objgrad(x)[1], want["gx"]) > 1e-3


def test_a_diagonal_eqqp_evaluates_bitwise_as_before():
    qp = _base()
    model = nlpmodels.EqQPModel(qp)
    rng = np.random.default_rng(3)
    x, v, y = qp.x, rng.standard_normal(qp.n), rng.standard_normal(qp.m)
    assert model.obj(x) == float(x @ (0.5 * qp.qdiag * x + qp.d))
    assert np.array_equal(model.grad(x), qp.qdiag * x + qp.d)
    assert np.array_equal(model.hprod(x, y, v), 1.0 * qp.qdiag * v)
    assert np.array_equal(model.hprod(x, y, v, obj_weight=0.3), 0.3 * qp.qdiag * v)
    assert np.array_equal(model.hprod(x, y, v, obj_weight=0.0), np.zeros(qp.n))


def test_the_iterative_device_model_rejects_a_sparse_hessian(monkeypatch):
    from fps_amd.device_qp import DeviceEqQP

    def no_load():
        raise AssertionError("the guard must come before the library is touched")

    monkeypatch.setattr(_lib, "load", no_load)
    qp = problems.with_sparse_hessian(_base(), 1, 7)
    with pytest.raises(ValueError, match="DeviceBandEqQP"):
        DeviceEqQP(qp)
