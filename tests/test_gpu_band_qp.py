"""Device-resident objgrad / hprod on the banded direct back-end (fpsq_band_qp_*, DeviceBandEqQP).  The yardstick is the
exact KKT solve on the CPU (oracle.exact_qp_objgrad / exact_qp_hprod: sparse LU of K), at the bar the banded back-end is
already held to against it: max|a - b| / max|b| < 1e-9 per vector, |phi - phi_exact| <= 1e-9 |phi_exact|."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import fps_amd  # noqa: F401
from fps_amd import _lib, nlpmodels, problems
from fps_amd.device_qp import DeviceBandEqQP

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


def _smoke_shape():
    return problems.pde_control_like(n=20000, m=2000, per_row=40, window=1024, seed=3)


CASES = {
    "small-delta0": (_small, 0.0, {}),                                            # m = 400: not a multiple of 128
    "smoke-shape": (_smoke_shape, SE, {}),
    "aug2dc": (lambda: problems.aug2dc_like(N=100), SE, {"chains": 2}),            # two chains, short rows
    "row-shuffled": (lambda: _shuffled(_small(), 5), 0.0, {"reordered": 1}),
    "m-multiple-of-128": (lambda: problems.pde_control_like(n=6000, m=640, per_row=24, window=512, seed=5), 1e-3, {}),
}


def _objgrad(dev, x, xk, on=None):
    """one evaluation with every output; `on`: a torch device to run it on device tensors, None: numpy arrays"""
    qp = dev.qp
    if on is None:
        gx, ys, gs = np.empty(qp.n), np.empty(qp.m), np.empty(qp.n)
        fx, rc = dev.objgrad(x, gx=gx, ys=ys, gs=gs, xk=xk)
        return fx, rc, gx, ys, gs
    import torch

    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(on)  # noqa: E731
    gx, ys, gs = (torch.empty(k, dtype=torch.float64, device=on) for k in (qp.n, qp.m, qp.n))
    fx, rc = dev.objgrad(t(x), gx=gx, ys=ys, gs=gs, xk=t(xk))
    return fx, rc, gx.cpu().numpy(), ys.cpu().numpy(), gs.cpu().numpy()


@pytest.mark.parametrize("case", list(CASES))
def test_band_qp_objgrad_and_hprod_match_the_exact_kkt_solve(oracle, case):
    make, delta, want_info = CASES[case]
    qp = make()
    x, xk = qp.x, qp.xhat
    dev = DeviceBandEqQP(qp, sigma=SIGMA, rho=0.0, delta=delta, eta=0.0)
    info = dev.info()
    for k, v in want_info.items():
        assert info[k] == v, (k, info)
    assert (qp.m % 128 == 0) == (case == "m-multiple-of-128")
    for rho, eta in ((0.0, 0.0), (1.0, 0.5)):
        dev.rho, dev.eta = rho, eta
        fx, rc, gx, ys, gs = _objgrad(dev, x, xk)
        e = oracle.exact_qp_objgrad(qp, x, SIGMA, rho, delta, eta, xk)
        errs = {"gx": _rel(gx, e["gx"]), "ys": _rel(ys, e["ys"]), "gs": _rel(gs, e["gs"]),
                "fx": abs(fx - e["fx"]) / abs(e["fx"])}
        print(f"\n{case} rho={rho} eta={eta}: {errs}")
        assert rc == 0
        assert errs["gx"] < 1e-9 and errs["ys"] < 1e-9 and errs["gs"] < 1e-9
        assert abs(fx - e["fx"]) <= 1e-9 * abs(e["fx"])
    v = np.random.default_rng(0).standard_normal(qp.n)
    Hv2, Hv1 = np.empty(qp.n), np.empty(qp.n)
    assert dev.hprod(v, Hv2, 2) == 0 and dev.hprod(v, Hv1, 1) == 0
    err = _rel(Hv2, oracle.exact_qp_hprod(qp, v, SIGMA, 1.0, delta, 0.5))
    print(f"{case} hprod: {err:.3e}")
    assert err < 1e-9
    assert np.array_equal(Hv1, Hv2)          # Val(1): the extra terms vanish identically on this model
    assert dev.info()["factorizations"] == 1
    dev.close()


def test_host_and_device_arguments_repeat_calls_and_both_sweep_forms_agree(monkeypatch):
    import torch

    qp = _smoke_shape()
    x, xk = qp.point(2), qp.xhat
    on = torch.device("cuda", 0)
    dev = DeviceBandEqQP(qp, sigma=SIGMA, rho=1.0, delta=SE, eta=0.5)
    host = _objgrad(dev, x, xk)
    again = _objgrad(dev, x, xk)
    devt = _objgrad(dev, x, xk, on=on)
    for a, b, c in zip(host, again, devt):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    v = np.random.default_rng(1).standard_normal(qp.n)
    Hh, Hd = np.empty(qp.n), torch.empty(qp.n, dtype=torch.float64, device=on)
    dev.hprod(v, Hh)
    dev.hprod(torch.from_numpy(v).to(on), Hd)
    assert np.array_equal(Hh, Hd.cpu().numpy())
    # A x and A' y through the same handle, against scipy, host and device arguments
    A = qp.scipy_csr()
    u = np.random.default_rng(2).standard_normal(qp.m)
    y0, z0 = np.random.default_rng(3).standard_normal(qp.m), np.empty(qp.n)
    y = y0.copy()
    dev.jac_mul(0, 2.0, x, -1.0, y)
    dev.jac_mul(1, 1.0, u, 0.0, z0)
    assert _rel(y, 2.0 * (A @ x) - y0) < 1e-13 and _rel(z0, A.T @ u) < 1e-13
    yd = torch.from_numpy(y0).to(on)
    dev.jac_mul(0, 2.0, torch.from_numpy(x).to(on), -1.0, yd)
    assert np.array_equal(yd.cpu().numpy(), y)
    dev.close()
    monkeypatch.setenv("FPSQ_TRSV_CHAIN", "0")   # one launch per step instead of one per sweep
    steps = DeviceBandEqQP(qp, sigma=SIGMA, rho=1.0, delta=SE, eta=0.5)
    other = _objgrad(steps, x, xk)
    steps.close()
    assert abs(other[0] - host[0]) <= 1e-13 * abs(host[0]) and other[1] == 0
    for a, b in zip(other[2:], host[2:]):
        assert _rel(a, b) < 1e-13


def test_row_shuffled_model_gives_device_outputs_in_the_callers_row_order(oracle):
    """jac_mul and ys on a handle whose symbolic phase reordered the rows: everything in the caller's numbering"""
    qp = _shuffled(_small(), 7)
    dev = DeviceBandEqQP(qp, sigma=SIGMA, rho=1.0, delta=0.0)
    assert dev.info()["reordered"] == 1
    A = qp.scipy_csr()
    u = np.random.default_rng(2).standard_normal(qp.m)
    y, z = np.zeros(qp.m), np.empty(qp.n)
    dev.jac_mul(0, 1.0, qp.x, 0.0, y)
    dev.jac_mul(1, 1.0, u, 0.0, z)
    assert _rel(y, A @ qp.x) < 1e-13 and _rel(z, A.T @ u) < 1e-13
    dev.close()


def test_null_outputs_state_and_argument_errors():
    qp = _small()
    dev = DeviceBandEqQP(qp, sigma=SIGMA, rho=1.0, delta=0.0, eta=0.5)
    lib, h, q = dev._lib, dev._h, dev._q
    fx = C.c_double()
    gx = np.empty(qp.n)
    # before any factorisation: the state error of the solve entries
    assert lib.fpsq_band_qp_objgrad(h, q, qp.x.ctypes.data, SIGMA, 1.0, 0.5, None, C.byref(fx), gx.ctypes.data, None,
                                    None) == -3
    assert b"no valid factorisation" in lib.fpsq_band_last_error(h)
    assert lib.fpsq_band_qp_hprod(h, q, qp.x.ctypes.data, SIGMA, 1.0, 0.5, 2, gx.ctypes.data) == -3
    assert lib.fpsq_band_jac_mul(h, 0, 1.0, qp.x.ctypes.data, 0.0, np.empty(qp.m).ctypes.data) == -3
    full = _objgrad(dev, qp.x, None)            # xk null with eta > 0: xk = 0
    zero = _objgrad(dev, qp.x, np.zeros(qp.n))
    for a, b in zip(full, zero):
        assert np.array_equal(a, b)
    f_only, rc = dev.objgrad(qp.x)              # every output vector null
    assert rc == 0 and f_only == full[0]
    ys = np.empty(qp.m)
    f_ys, _ = dev.objgrad(qp.x, ys=ys)
    assert f_ys == full[0] and np.array_equal(ys, full[3])
    assert lib.fpsq_band_qp_hprod(h, q, qp.x.ctypes.data, SIGMA, 1.0, 0.5, 3, gx.ctypes.data) == -1
    assert lib.fpsq_band_qp_objgrad(h, q, None, SIGMA, 1.0, 0.5, None, C.byref(fx), None, None, None) == -1
    dev.close()


def test_the_factor_is_reused_until_delta_or_the_jacobian_changes(oracle):
    qp = _small()
    dev = DeviceBandEqQP(qp, sigma=SIGMA, rho=1.0, delta=0.0)
    assert dev.info()["factorizations"] == 0
    for t in range(5):
        dev.objgrad(qp.point(t), gx=np.empty(qp.n))
    assert dev.info()["factorizations"] == 1
    dev.set_delta(1e-3)
    assert dev.info()["factorizations"] == 1   # lazily: at the next evaluation
    x = qp.point(7)
    fx, rc, gx, ys, gs = _objgrad(dev, x, None)
    dev.hprod(x, np.empty(qp.n))
    assert dev.info()["factorizations"] == 2
    e = oracle.exact_qp_objgrad(qp, x, SIGMA, 1.0, 1e-3)
    assert _rel(gx, e["gx"]) < 1e-9 and _rel(ys, e["ys"]) < 1e-9 and abs(fx - e["fx"]) <= 1e-9 * abs(e["fx"])
    dev.set_jacobian_values(-2.5 * qp.vals)
    fx, rc, gx, ys, gs = _objgrad(dev, x, None)
    dev.objgrad(qp.point(8))
    assert dev.info()["factorizations"] == 3
    scaled = dataclasses.replace(qp, vals=-2.5 * qp.vals)
    e = oracle.exact_qp_objgrad(scaled, x, SIGMA, 1.0, 1e-3)
    assert rc == 0 and _rel(gx, e["gx"]) < 1e-9 and _rel(ys, e["ys"]) < 1e-9 and _rel(gs, e["gs"]) < 1e-9
    assert abs(fx - e["fx"]) <= 1e-9 * abs(e["fx"])
    dev.close()


def test_inputs_produced_on_the_registered_stream_are_waited_for():
    """x comes out of torch kernels enqueued right before the call, with no host synchronisation: the handle's stream
    waits for the registered (torch's current) stream, so the call reads the finished x."""
    import torch

    qp = _smoke_shape()
    on = torch.device("cuda", 0)
    dev = DeviceBandEqQP(qp, sigma=SIGMA, rho=1.0, delta=SE)
    a = torch.from_numpy(qp.xhat).to(on)
    b = torch.from_numpy(qp.point(4) - qp.xhat).to(on)
    big = torch.rand(4096, 4096, dtype=torch.float64, device=on)
    gx1, gx2 = (torch.empty(qp.n, dtype=torch.float64, device=on) for _ in range(2))
    x = a + b
    torch.cuda.synchronize()
    f1, _ = dev.objgrad(x, gx=gx1)               # the synchronised call
    x.zero_()
    torch.cuda.synchronize()
    for _ in range(4):                           # keeps the stream busy: x below is not ready when the call is made
        big = big @ big * 1e-3
    x = torch.add(a, b, out=x)
    f2, _ = dev.objgrad(x, gx=gx2)
    assert f1 == f2 and torch.equal(gx1, gx2)
    dev.close()


def _kkt_point(qp):
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla

    A = qp.scipy_csr()
    K = sp.bmat([[sp.diags(qp.qdiag), A.T], [A, None]], format="csc")
    sol = spla.spsolve(K, np.concatenate([-qp.d, qp.b]))
    return sol[:qp.n], sol[qp.n:]


@pytest.mark.parametrize("sub", ["trunk", "lbfgs"])
@pytest.mark.parametrize("shape", ["pde", "aug2dc"])
def test_fps_solve_device_on_the_banded_direct_backend(sub, shape):
    """The device-resident outer loop on the exact back-end, at the default tolerances, to the bounds
    test_fps_solve_through_the_banded_direct_backend holds the host seam to -- also on the AUG2DC-like grid, the shape
    class the iterative device loop stops unsolved on."""
    import torch

    from fps_amd.fps_solve import fps_solve_device

    qp = _small() if shape == "pde" else problems.aug2dc_like(N=30)
    xstar, lam = _kkt_point(qp)
    dev = DeviceBandEqQP(qp)
    x0 = torch.from_numpy(qp.x).to(torch.device("cuda", 0))
    stats = fps_solve_device(dev, x0, subproblem_solver=sub, max_time=120)
    x, y = stats.solution.cpu().numpy(), stats.multipliers.cpu().numpy()
    print(f"\n{shape}/{sub}: {stats.status}, |x - x*|/|x*| = {np.linalg.norm(x - xstar) / np.linalg.norm(xstar):.2e}, "
          f"|y - y*| = {np.linalg.norm(y - lam):.2e} (|y*| = {np.linalg.norm(lam):.2e}), {dev.info()['factorizations']} factorisations")
    assert stats.status == "first_order", (stats.status, stats.solver_specific)
    assert np.linalg.norm(x - xstar) <= 1e-6 * np.linalg.norm(xstar)
    assert np.linalg.norm(y - lam) <= 1e-5 * max(1.0, np.linalg.norm(lam))
    dev.close()


def test_the_seam_and_the_device_entry_agree(oracle):
    """HIPBandedDirectQDSolver behind FletcherPenaltyNLP (host model, host epilogue) and fpsq_band_qp_objgrad: the same
    factor, different summation orders in the products -- 1e-12 relative."""
    from fps_amd.penalty_nlp import FletcherPenaltyNLP
    from fps_amd.qdsolver import HIPBandedDirectQDSolver

    qp = _small()
    model = nlpmodels.EqQPModel(qp)
    qds = HIPBandedDirectQDSolver(model, 0.0)
    fp = FletcherPenaltyNLP(model, SIGMA, 1.0, 0.0, 2, qds=qds)
    f_seam, g_seam = fp.objgrad(qp.x)
    dev = DeviceBandEqQP(qp, sigma=SIGMA, rho=1.0, delta=0.0)
    fx, rc, gx, ys, gs = _objgrad(dev, qp.x, None)
    assert abs(fx - f_seam) <= 1e-12 * abs(f_seam)
    assert _rel(gx, g_seam) < 1e-12 and _rel(ys, fp.ys) < 1e-12 and _rel(gs, fp.gs) < 1e-12
    qds.close()
    dev.close()
