"""Device-resident objgrad / hprod on the banded direct back-end with a SPARSE SYMMETRIC objective Hessian
(fpsq_band_qp_create_csr, DeviceBandEqQP on an EqQP that carries hess_*).  The yardstick is the exact evaluation in scipy
(tests/sparse_hessian_ref.py: one sparse LU of K = [I A'; A -delta I]) at the bar tests/test_gpu_band_qp.py holds the diagonal
model to on the same factor: max|a - b| / max|b| < 1e-9 per vector, |phi - phi_exact| <= 1e-9 |phi_exact|.

Lanes per row of R = Q - diag(Q) follow lane_group(nnz(R), n) = the largest power of two <= nnz(R) // n: with the empty rows
with_sparse_hessian leaves, half_width 1 / 2 / 8 give groups of 1 / 2 / 8 lanes (asserted below through the same rule)."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import fps_amd  # noqa: E402,F401
from fps_amd import problems  # noqa: E402
from fps_amd.device_qp import DeviceBandEqQP, DeviceEqQP  # noqa: E402
from sparse_hessian_ref import SparseHessianRef  # noqa: E402

pytestmark = pytest.mark.gpu

SE = float(np.sqrt(np.finfo(float).eps))
SIGMA = 1e3


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def _shuffled(qp, seed):
    """the same QP with its constraint rows in a random order (a full natural band: the symbolic phase reorders)"""
    import scipy.sparse as sp

    perm = np.random.default_rng(seed).permutation(qp.m)
    A = sp.csr_matrix(qp.scipy_csr()[perm])
    A.sort_indices()
    return dataclasses.replace(qp, rowptr=A.indptr.astype(np.int32), colind=A.indices.astype(np.int32), vals=A.data.copy(),
                               b=qp.b[perm])


def _small():
    return problems.pde_control_like(n=4000, m=400, per_row=16, window=512, seed=21)


def _lanes(qp):
    """lane_group(nnz(R), n) of csrc/fpsq_direct.hip.h"""
    mean = (int(qp.hess_vals.size) - int(np.count_nonzero(qp.hess_csr().diagonal()))) // qp.n
    lg = 1
    while lg < 64 and 2 * lg <= mean:
        lg *= 2
    return lg


BASES = {
    "small-delta0": (_small, 0.0, {}),                                            # m = 400: not a multiple of 128
    "row-shuffled": (lambda: _shuffled(_small(), 5), 0.0, {"reordered": 1}),
    "aug2dc": (lambda: problems.aug2dc_like(N=100), SE, {"chains": 2}),            # two chains, one lane per row of A'
    "m-multiple-of-128": (lambda: problems.pde_control_like(n=6000, m=640, per_row=24, window=512, seed=5), 1e-3, {}),
}


def _objgrad(dev, x, xk, on=None, want=("gx", "ys", "gs")):
    """one evaluation; `on`: a torch device to run it on device tensors, None: numpy arrays; outputs not in `want` are null"""
    qp = dev.qp
    size = {"gx": qp.n, "ys": qp.m, "gs": qp.n}
    if on is None:
        out = {k: np.full(size[k], np.nan) for k in want}
        fx, rc = dev.objgrad(x, xk=xk, **out)
        return fx, rc, out
    import torch

    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(on)  # noqa: E731
    out = {k: torch.full((size[k],), float("nan"), dtype=torch.float64, device=on) for k in want}
    fx, rc = dev.objgrad(t(x), xk=t(xk), **out)
    return fx, rc, {k: v.cpu().numpy() for k, v in out.items()}


def test_half_widths_give_the_lane_groups_and_ragged_tiles_the_cases_rely_on():
    lanes = {hw: _lanes(problems.with_sparse_hessian(_small(), hw, 11)) for hw in (1, 2, 8)}
    assert lanes == {1: 1, 2: 2, 8: 8}
    # n that is no multiple of the rows of a tile, 256 / LG, and one that is
    assert 4000 % (256 // lanes[1]) != 0 and 6000 % (256 // lanes[8]) != 0 and 20200 % (256 // lanes[8]) != 0
    assert 4000 % (256 // lanes[8]) == 0


@pytest.mark.parametrize("hw", [1, 8])
@pytest.mark.parametrize("case", list(BASES))
def test_objgrad_and_hprod_with_a_sparse_hessian_match_the_exact_reference(case, hw):
    make, delta, want_info = BASES[case]
    qp = problems.with_sparse_hessian(make(), hw, 11)
    ref = SparseHessianRef(qp, delta)
    x = qp.x
    dev = DeviceBandEqQP(qp, sigma=SIGMA, rho=0.0, delta=delta, eta=0.0)
    info = dev.info()
    for k, v in want_info.items():
        assert info[k] == v, (k, info)
    v = np.random.default_rng(0).standard_normal(qp.n)
    for rho, eta in ((0.0, 0.0), (1.0, 0.5)):
        dev.rho, dev.eta = rho, eta
        for xk in (qp.xhat, None):
            fx, rc, o = _objgrad(dev, x, xk)
            e = ref.objgrad(x, SIGMA, rho, eta, xk)
            errs = {k: _rel(o[k], e[k]) for k in ("gx", "ys", "gs")}
            errs["fx"] = abs(fx - e["fx"]) / abs(e["fx"])
            print(f"\n{case} hw={hw} rho={rho} eta={eta} xk={'given' if xk is not None else 'None'}: {errs}")
            assert rc == 0
            assert errs["gx"] < 1e-9 and errs["ys"] < 1e-9 and errs["gs"] < 1e-9
            assert abs(fx - e["fx"]) <= 1e-9 * abs(e["fx"])
        Hv2, Hv1 = np.empty(qp.n), np.empty(qp.n)
        assert dev.hprod(v, Hv2, 2) == 0 and dev.hprod(v, Hv1, 1) == 0
        err = _rel(Hv2, ref.hprod(v, SIGMA, rho, eta))
        print(f"{case} hw={hw} rho={rho} eta={eta} hprod: {err:.3e}")
        assert err < 1e-9
        assert np.array_equal(Hv1, Hv2)      # Val(1): the extra terms vanish identically for linear constraints
    assert dev.info()["factorizations"] == 1
    dev.close()


@pytest.mark.parametrize("hw", [1, 8])
def test_host_and_device_arguments_repeats_and_null_outputs_are_bitwise_the_same(hw):
    import torch

    qp = problems.with_sparse_hessian(_small(), hw, 11)
    x, xk = qp.point(2), qp.xhat
    on = torch.device("cuda", 0)
    dev = DeviceBandEqQP(qp, sigma=SIGMA, rho=1.0, delta=0.0, eta=0.5)
    host = _objgrad(dev, x, xk)
    again = _objgrad(dev, x, xk)
    devt = _objgrad(dev, x, xk, on=on)
    for other in (again, devt):
        assert other[0] == host[0] and other[1] == 0
        for k in ("gx", "ys", "gs"):
            assert np.array_equal(other[2][k], host[2][k]), k
    # every subset of the output vectors, host- and device-resident: the others (and phi) do not change a bit
    for want in ((), ("gx",), ("ys",), ("gs",), ("gx", "ys"), ("ys", "gs")):
        for where in (None, on):
            fx, rc, o = _objgrad(dev, x, xk, on=where, want=want)
            assert fx == host[0] and rc == 0
            for k in want:
                assert np.array_equal(o[k], host[2][k]), (want, k)
    v = np.random.default_rng(1).standard_normal(qp.n)
    Hh, Hh2, Hd = np.empty(qp.n), np.empty(qp.n), torch.empty(qp.n, dtype=torch.float64, device=on)
    dev.hprod(v, Hh)
    dev.hprod(v, Hh2)
    dev.hprod(torch.from_numpy(v).to(on), Hd)
    assert np.array_equal(Hh, Hh2) and np.array_equal(Hh, Hd.cpu().numpy())
    dev.close()


def _raw_objgrad(lib, h, q, qp, x, xk, rho, eta):
    fx = C.c_double()
    gx, ys, gs = np.empty(qp.n), np.empty(qp.m), np.empty(qp.n)
    rc = lib.fpsq_band_qp_objgrad(h, q, x.ctypes.data, SIGMA, rho, eta, xk.ctypes.data, C.byref(fx), gx.ctypes.data,
                                  ys.ctypes.data, gs.ctypes.data)
    assert rc == 0, lib.fpsq_band_last_error(h)
    Hv = np.empty(qp.n)
    assert lib.fpsq_band_qp_hprod(h, q, x.ctypes.data, SIGMA, rho, eta, 2, Hv.ctypes.data) == 0
    return fx.value, gx, ys, gs, Hv


def test_stored_zeros_agree_with_the_diagonal_model_and_models_do_not_disturb_each_other():
    qp = _small()
    pattern = problems.with_sparse_hessian(qp, 2, 11)
    Q = pattern.hess_csr().copy()
    Q.data[:] = 0.0                     # every off-diagonal entry STORED, with value 0.0 ...
    Q.setdiag(qp.qdiag)                 # ... and the diagonal model's diagonal
    zeros = dataclasses.replace(pattern, qdiag=qp.qdiag, hess_vals=Q.data.copy())
    assert zeros.hess_vals.size == pattern.hess_vals.size and np.count_nonzero(zeros.hess_vals) == qp.n
    x, xk = qp.point(1), qp.xhat
    dev = DeviceBandEqQP(qp, sigma=SIGMA, rho=1.0, delta=0.0, eta=0.5)
    lib, h = dev._lib, dev._h
    dev.objgrad(x)                      # (the factorisation)
    first = _raw_objgrad(lib, h, dev._q, qp, x, xk, 1.0, 0.5)
    # two more models on the SAME handle: the stored-zeros one and the truly sparse one
    qz, qs, qd2 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    for mdl, out in ((zeros, qz), (pattern, qs)):
        assert lib.fpsq_band_qp_create_csr(h, mdl.hess_rowptr.ctypes.data, mdl.hess_colind.ctypes.data,
                                           mdl.hess_vals.ctypes.data, qp.d.ctypes.data, qp.b.ctypes.data,
                                           C.byref(out)) == 0, lib.fpsq_band_last_error(h)
    got = _raw_objgrad(lib, h, qz, qp, x, xk, 1.0, 0.5)
    # each element differs at most by the order in which a few fp64 terms (exact zeros among them) are added; f is summed
    # over another partition of the rows
    assert abs(got[0] - first[0]) <= 1e-13 * abs(first[0])
    for name, a, b in zip(("gx", "ys", "gs", "Hv"), got[1:], first[1:]):
        assert _rel(a, b) <= 1e-14, (name, _rel(a, b))
    sparse = _raw_objgrad(lib, h, qs, qp, x, xk, 1.0, 0.5)
    assert _rel(sparse[1], first[1]) > 1e-3          # (a different model)
    # the diagonal model after the sparse ones, and a diagonal model created after them: bitwise the first answer
    assert lib.fpsq_band_qp_create(h, qp.qdiag.ctypes.data, qp.d.ctypes.data, qp.b.ctypes.data, C.byref(qd2)) == 0
    for q in (dev._q, qd2):
        after = _raw_objgrad(lib, h, q, qp, x, xk, 1.0, 0.5)
        assert after[0] == first[0]
        for a, b in zip(after[1:], first[1:]):
            assert np.array_equal(a, b)
    # ... and the sparse one is not disturbed by them either
    sparse2 = _raw_objgrad(lib, h, qs, qp, x, xk, 1.0, 0.5)
    assert sparse2[0] == sparse[0] and all(np.array_equal(a, b) for a, b in zip(sparse2[1:], sparse[1:]))
    for q in (qz, qs, qd2):
        assert lib.fpsq_band_qp_destroy(q) == 0
    dev.close()


def test_create_csr_refuses_an_unsymmetric_duplicate_or_out_of_range_hessian():
    qp = problems.with_sparse_hessian(_small(), 2, 11)
    dev = DeviceBandEqQP(qp, sigma=SIGMA, rho=1.0, delta=0.0)
    lib, h = dev._lib, dev._h
    before = _objgrad(dev, qp.x, None)
    rp, ci, va = qp.hess_rowptr, qp.hess_colind, qp.hess_vals
    k = int(rp[7])                                    # row 7, first entry: column 5 (rows 5 .. 9 have every neighbour)
    assert ci[k] == 5 and rp[8] - rp[7] == 5

    def attempt(rp, ci, va):
        q = C.c_void_p()
        rc = lib.fpsq_band_qp_create_csr(h, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, qp.d.ctypes.data,
                                         qp.b.ctypes.data, C.byref(q))
        return rc, lib.fpsq_band_last_error(h).decode(), q

    bad_val = va.copy()
    bad_val[k] += 1e-9                                # Q[7, 5] != Q[5, 7]
    bad_pat = ci.copy()
    bad_pat[k] = 4                                    # (7, 4) has no transpose: half_width 2
    dup = ci.copy()
    dup[k] = ci[k + 1]                                # column 6 twice in row 7
    oob, neg = ci.copy(), ci.copy()
    oob[k], neg[k] = qp.n, -1
    for what, args in (("values", (rp, ci, bad_val)), ("pattern", (rp, bad_pat, va)), ("duplicate", (rp, dup, va)),
                       ("out of range", (rp, oob, va)), ("out of range", (rp, neg, va))):
        rc, msg, q = attempt(*args)
        print(what, "->", rc, msg)
        assert rc == -1 and not q.value and "band_qp_create_csr" in msg and what.split()[0] in msg, (what, rc, msg)
    # unsorted columns and an absent diagonal are fine
    flip = ci.copy(), va.copy()
    for a in flip:
        a[k:k + 5] = a[k:k + 5][::-1].copy()
    rc, msg, q = attempt(rp, *flip)
    assert rc == 0, msg
    x, xk = qp.x, np.zeros(qp.n)
    got = _raw_objgrad(lib, h, q, qp, x, xk, 1.0, 0.0)
    lib.fpsq_band_qp_destroy(q)
    assert got[0] == before[0] and np.array_equal(got[1], before[2]["gx"])   # stored sorted: the same bits
    # the handle and its model stay usable
    after = _objgrad(dev, qp.x, None)
    assert after[0] == before[0] and all(np.array_equal(after[2][k], before[2][k]) for k in before[2])
    dev.close()


def test_an_absent_diagonal_is_zero():
    qp = problems.with_sparse_hessian(_small(), 2, 11)
    Q = qp.hess_csr().tolil()
    Q.setdiag(0.0)
    Q = Q.tocsr()
    Q.eliminate_zeros()
    nodiag = dataclasses.replace(qp, qdiag=np.zeros(qp.n), hess_rowptr=Q.indptr.astype(np.int32),
                                 hess_colind=Q.indices.astype(np.int32), hess_vals=Q.data.copy())
    assert nodiag.hess_vals.size == qp.hess_vals.size - qp.n
    ref = SparseHessianRef(nodiag, 0.0)
    dev = DeviceBandEqQP(nodiag, sigma=SIGMA, rho=1.0, delta=0.0)
    fx, rc, o = _objgrad(dev, qp.x, None)
    e = ref.objgrad(qp.x, SIGMA, 1.0)
    assert rc == 0 and _rel(o["gx"], e["gx"]) < 1e-9 and _rel(o["ys"], e["ys"]) < 1e-9 and _rel(o["gs"], e["gs"]) < 1e-9
    assert abs(fx - e["fx"]) <= 1e-9 * abs(e["fx"])
    dev.close()


def test_the_factor_is_reused_with_a_sparse_hessian():
    qp = problems.with_sparse_hessian(_small(), 2, 11)
    dev = DeviceBandEqQP(qp, sigma=SIGMA, rho=1.0, delta=0.0)
    assert dev.info()["factorizations"] == 0
    for t in range(3):
        dev.objgrad(qp.point(t), gx=np.empty(qp.n))
        dev.hprod(qp.point(t), np.empty(qp.n))
    assert dev.info()["factorizations"] == 1
    dev.set_delta(1e-3)
    x = qp.point(7)
    fx, rc, o = _objgrad(dev, x, None)
    dev.hprod(x, np.empty(qp.n))
    assert dev.info()["factorizations"] == 2
    e = SparseHessianRef(qp, 1e-3).objgrad(x, SIGMA, 1.0)
    assert rc == 0 and _rel(o["gx"], e["gx"]) < 1e-9 and _rel(o["ys"], e["ys"]) < 1e-9
    assert abs(fx - e["fx"]) <= 1e-9 * abs(e["fx"])
    dev.close()


def test_the_iterative_device_model_rejects_a_sparse_hessian():
    with pytest.raises(ValueError, match="DeviceBandEqQP"):
        DeviceEqQP(problems.with_sparse_hessian(_small(), 1, 11))


@pytest.mark.parametrize("sub", ["trunk", "lbfgs"])
def test_fps_solve_device_with_a_sparse_hessian(sub):
    """The device-resident outer loop at the default tolerances, to the bounds
    test_gpu_band_qp.py::test_fps_solve_device_on_the_banded_direct_backend holds the diagonal model to."""
    import torch

    from fps_amd.fps_solve import fps_solve_device

    qp = problems.with_sparse_hessian(_small(), 2, 11)
    xstar, lam = SparseHessianRef(qp, 0.0).kkt_point()
    dev = DeviceBandEqQP(qp)
    x0 = torch.from_numpy(qp.x).to(torch.device("cuda", 0))
    stats = fps_solve_device(dev, x0, subproblem_solver=sub, max_time=120)
    x, y = stats.solution.cpu().numpy(), stats.multipliers.cpu().numpy()
    print(f"\n{sub}: {stats.status}, |x - x*|/|x*| = {np.linalg.norm(x - xstar) / np.linalg.norm(xstar):.2e}, "
          f"|y - y*| = {np.linalg.norm(y - lam):.2e} (|y*| = {np.linalg.norm(lam):.2e}), "
          f"{dev.info()['factorizations']} factorisations")
    assert stats.status == "first_order", (stats.status, stats.solver_specific)
    assert np.linalg.norm(x - xstar) <= 1e-6 * np.linalg.norm(xstar)
    assert np.linalg.norm(y - lam) <= 1e-5 * max(1.0, np.linalg.norm(lam))
    dev.close()
