"""Device-resident nonlinear equality constraints on the banded direct back-end (fpsq_band_nlp_*, DeviceBandSepQuadNLP).  The
yardstick is the CPU restatement tests/sepquad_ref.py (exact KKT solves at J(x), the gradient in the -ys form, the mirror's
hprod_), at the bar tests/test_gpu_band_qp.py holds this back-end to: max|a - b| / max|b| < 1e-9 per vector,
|fx - fx_ref| <= 1e-9 |fx_ref|.  The two gradient forms differ by more than 1e-2 (tests/test_band_nlp_cpu.py), so the bar tells
them apart."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import fps_amd  # noqa: E402,F401
from fps_amd import _lib, nlpmodels, problems  # noqa: E402
from fps_amd.device_qp import DeviceBandEqQP, DeviceBandSepQuadNLP, DeviceBorderedBandEqQP  # noqa: E402
from fps_amd.qdsolver import FpsqError  # noqa: E402
from sepquad_ref import SepQuadRef  # noqa: E402

pytestmark = pytest.mark.gpu

SE = float(np.sqrt(np.finfo(float).eps))
SIGMA, CURV = 1e3, 0.3
ERR_STATE = -3


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


CASES = {
    "small": (_small, {}),                                                        # m = 400: not a multiple of 128
    "row-shuffled": (lambda: _shuffled(_small(), 5), {"reordered": 1}),
    "aug2dc": (lambda: problems.aug2dc_like(N=100), {"chains": 2}),              # two chains, short rows
    "m-multiple-of-128": (lambda: problems.pde_control_like(n=6000, m=640, per_row=24, window=512, seed=5), {}),
}


def _data(qp):
    return problems.with_quadratic_constraints(qp, curv=CURV, seed=7)


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


@pytest.mark.parametrize("delta", [0.0, SE], ids=["delta0", "deltaSE"])
@pytest.mark.parametrize("case", list(CASES))
def test_objgrad_hprod_and_cons_match_the_exact_restatement(case, delta):
    """Val(1) at delta = sqrt(eps) is the same quantity as the mirror's (tau = delta); at delta = 0 the mirror solves with
    tau = 1e-14 and the device with the cached factor (tau = 0): they differ by O(1e-14 |M^-1|), far inside the bar."""
    make, want_info = CASES[case]
    qp = make()
    data = _data(qp)
    x, xk = qp.x, qp.xhat
    dev = DeviceBandSepQuadNLP(data, sigma=SIGMA, rho=0.0, delta=delta, eta=0.0)
    info = dev.info()
    for k, v in want_info.items():
        assert info[k] == v, (k, info)
    assert info["border_rows"] == 0 and info["border_cols"] == 0
    assert (qp.m % 128 == 0) == (case == "m-multiple-of-128")
    ref = SepQuadRef(data, SIGMA, 0.0, delta, 0.0, xk)   # (ys, gs, c depend on sigma and delta alone: one solve for both pairs)
    v = np.random.default_rng(0).standard_normal(qp.n)
    c = np.empty(qp.m)
    assert dev.cons(x, c) == 0
    nobj = 0
    for rho, eta in ((0.0, 0.0), (1.0, 0.5)):
        dev.rho, dev.eta = rho, eta
        ref.pen.rho, ref.pen.eta = rho, eta
        fx, rc, gx, ys, gs = _objgrad(dev, x, xk)
        nobj += 1
        e = ref.objgrad(x)
        errs = {"gx": _rel(gx, e["gx"]), "ys": _rel(ys, e["ys"]), "gs": _rel(gs, e["gs"]), "c": _rel(c, e["c"]),
                "fx": abs(fx - e["fx"]) / abs(e["fx"])}
        Hv2, Hv1 = np.empty(qp.n), np.empty(qp.n)
        assert dev.hprod(v, Hv2, 2) == 0 and dev.hprod(v, Hv1, 1) == 0
        errs["Hv2"] = _rel(Hv2, ref.hprod(x, v, 2))
        errs["Hv1"] = _rel(Hv1, ref.hprod(x, v, 1))
        errs["Hv1-Hv2"] = _rel(Hv1, Hv2)
        print(f"\n{case} delta={delta:.1e} rho={rho} eta={eta}: " + " ".join(f"{k}={v_:.2e}" for k, v_ in errs.items()))
        assert rc == 0
        for k in ("gx", "ys", "gs", "c", "Hv2", "Hv1"):
            assert errs[k] < 1e-9, (k, errs[k])
        assert abs(fx - e["fx"]) <= 1e-9 * abs(e["fx"])
        assert errs["Hv1-Hv2"] > 1e-6          # the terms that vanish on the linear model are live here
    assert dev.info()["factorizations"] == nobj   # one per objgrad, none for hprod / cons
    # the handle's values are J(x) now: fpsq_band_jac_mul multiplies with it
    J = nlpmodels.SepQuadConModel(data)._J(x)
    u, y, z = np.random.default_rng(2).standard_normal(qp.m), np.empty(qp.m), np.empty(qp.n)
    assert dev.jac_mul(0, 1.0, v, 0.0, y) == 0 and dev.jac_mul(1, 1.0, u, 0.0, z) == 0
    assert _rel(y, J @ v) < 1e-13 and _rel(z, J.T @ u) < 1e-13
    dev.close()


@pytest.mark.parametrize("case", ["small", "row-shuffled"])
def test_linear_limit_agrees_with_the_linear_model(case):
    """h_vals = 0: the model IS the eq-QP, and objgrad / hprod agree with DeviceBandEqQP on the same QP within 1e-12 relative
    (not bitwise: the product kernels differ); Val(1) equals Val(2) within that."""
    qp = CASES[case][0]()
    data = problems.SepQuadNLP(qp, np.zeros_like(qp.vals), qp.b.copy())
    x, xk = qp.x, qp.xhat
    v = np.random.default_rng(0).standard_normal(qp.n)
    for delta in (0.0, SE):
        lin = DeviceBandEqQP(qp, sigma=SIGMA, rho=1.0, delta=delta, eta=0.5)
        dev = DeviceBandSepQuadNLP(data, sigma=SIGMA, rho=1.0, delta=delta, eta=0.5)
        a, b = _objgrad(lin, x, xk), _objgrad(dev, x, xk)
        assert a[1] == 0 and b[1] == 0
        assert abs(a[0] - b[0]) <= 1e-12 * abs(a[0])
        for p, q in zip(a[2:], b[2:]):
            assert _rel(q, p) < 1e-12
        Hl, H2, H1 = np.empty(qp.n), np.empty(qp.n), np.empty(qp.n)
        assert lin.hprod(v, Hl, 2) == 0 and dev.hprod(v, H2, 2) == 0 and dev.hprod(v, H1, 1) == 0
        assert _rel(H2, Hl) < 1e-12 and _rel(H1, H2) < 1e-12
        lin.close()
        dev.close()


def test_repeatability_placement_and_no_state_between_evaluations():
    import torch

    qp = _small()
    data = _data(qp)
    x1, x2, xk = qp.x, qp.point(2), qp.xhat
    on = torch.device("cuda", 0)
    v = np.random.default_rng(1).standard_normal(qp.n)

    def hprods(dev, device_args):
        out = []
        for ha in (2, 1):
            if device_args:
                H = torch.empty(qp.n, dtype=torch.float64, device=on)
                assert dev.hprod(torch.from_numpy(v).to(on), H, ha) == 0
                out.append(H.cpu().numpy())
            else:
                H = np.empty(qp.n)
                assert dev.hprod(v, H, ha) == 0
                out.append(H)
        return out

    dev = DeviceBandSepQuadNLP(data, sigma=SIGMA, rho=1.0, delta=SE, eta=0.5)
    host = _objgrad(dev, x1, xk)
    hh = hprods(dev, False)
    again = _objgrad(dev, x1, xk)
    devt = _objgrad(dev, x1, xk, on=on)
    hd = hprods(dev, True)
    assert host[1] == 0
    for a, b, c in zip(host, again, devt):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    for a, b in zip(hh, hd):
        assert np.array_equal(a, b)
    ch, cd = np.empty(qp.m), torch.empty(qp.m, dtype=torch.float64, device=on)
    assert dev.cons(x1, ch) == 0 and dev.cons(torch.from_numpy(x1).to(on), cd) == 0
    assert np.array_equal(ch, cd.cpu().numpy())
    # a second x: another J, and nothing of the first evaluation is left -- a fresh handle gives the same bits
    second = _objgrad(dev, x2, xk)
    h2 = hprods(dev, False)
    fresh_dev = DeviceBandSepQuadNLP(data, sigma=SIGMA, rho=1.0, delta=SE, eta=0.5)
    fresh = _objgrad(fresh_dev, x2, xk)
    hf = hprods(fresh_dev, False)
    assert second[1] == 0 and fresh[1] == 0
    assert not np.array_equal(second[2], host[2])
    for a, b in zip(second, fresh):
        assert np.array_equal(a, b)
    for a, b in zip(h2, hf):
        assert np.array_equal(a, b)
    assert dev.info()["factorizations"] == 4 and fresh_dev.info()["factorizations"] == 1
    dev.close()
    fresh_dev.close()


def test_state_rules(oracle):
    lib = _lib.load()
    qp = _small()
    data = _data(qp)
    x, xk = qp.x, qp.xhat
    v, Hv = np.random.default_rng(1).standard_normal(qp.n), np.empty(qp.n)
    dev = DeviceBandSepQuadNLP(data, sigma=SIGMA, rho=1.0, delta=SE, eta=0.0)
    h, q = dev._h, dev._q

    def hprod_rc(ha=2):
        return lib.fpsq_band_nlp_hprod(h, q, v.ctypes.data, SIGMA, 1.0, 0.0, ha, Hv.ctypes.data)

    # before any objgrad
    assert hprod_rc() == ERR_STATE and b"objgrad" in lib.fpsq_band_last_error(h)
    with pytest.raises(FpsqError):
        dev.hprod(v, Hv)
    first = _objgrad(dev, x, xk)
    assert first[1] == 0 and hprod_rc() == 0 and hprod_rc(1) == 0
    assert hprod_rc(3) == -1
    # someone else factorises the handle: a fpsq_band_qp model on it evaluates correctly on ITS Jacobian ...
    lq = C.c_void_p()
    assert lib.fpsq_band_qp_create(h, qp.qdiag.ctypes.data, qp.d.ctypes.data, qp.b.ctypes.data, C.byref(lq)) == 0
    assert lib.fpsq_band_factorize(h, qp.vals.ctypes.data, SE, None) == 0
    fx, gx, ys, gs = C.c_double(), np.empty(qp.n), np.empty(qp.m), np.empty(qp.n)
    assert lib.fpsq_band_qp_objgrad(h, lq, x.ctypes.data, SIGMA, 1.0, 0.0, None, C.byref(fx), gx.ctypes.data, ys.ctypes.data,
                                    gs.ctypes.data) == 0
    e = oracle.exact_qp_objgrad(qp, x, SIGMA, 1.0, SE, 0.0, None)
    assert _rel(gx, e["gx"]) < 1e-9 and _rel(ys, e["ys"]) < 1e-9 and _rel(gs, e["gs"]) < 1e-9
    assert abs(fx.value - e["fx"]) <= 1e-9 * abs(e["fx"])
    # ... and the nonlinear model's point is gone until its next objgrad, which returns what it returned before
    assert hprod_rc() == ERR_STATE and b"factorised again" in lib.fpsq_band_last_error(h)
    assert hprod_rc(1) == ERR_STATE
    back = _objgrad(dev, x, xk)
    for a, b in zip(first, back):
        assert np.array_equal(a, b)
    assert hprod_rc() == 0
    assert lib.fpsq_band_qp_destroy(lq) == 0
    dev.close()

    # handles the model does not take: border rows, long columns, COO-created
    def create_rc(handle, prob):
        out = C.c_void_p()
        z = np.zeros_like(prob.vals)
        rc = lib.fpsq_band_nlp_create(handle, prob.qdiag.ctypes.data, prob.d.ctypes.data, prob.b.ctypes.data,
                                      prob.vals.ctypes.data, z.ctypes.data, C.byref(out))
        return rc, lib.fpsq_band_last_error(handle)

    big = problems.pde_control_like(n=12000, m=1280, per_row=16, window=512, seed=9)
    rows = DeviceBorderedBandEqQP(problems.with_border_rows(big, 2), border=16, cols=0)
    assert rows.info()["border_rows"] > 0
    rc, msg = create_rc(rows._h, rows.qp)
    assert rc == ERR_STATE and b"band_nlp_create" in msg and b"border rows" in msg
    rows.close()
    cols = DeviceBorderedBandEqQP(problems.with_long_columns(big, 2), border=0, cols=16)
    assert cols.info()["border_cols"] > 0
    rc, msg = create_rc(cols._h, cols.qp)
    assert rc == ERR_STATE and b"band_nlp_create" in msg and b"long columns" in msg
    cols.close()
    coo = C.c_void_p()
    r = np.repeat(np.arange(qp.m, dtype=np.int64), np.diff(qp.rowptr))
    cidx = qp.colind.astype(np.int64)
    assert lib.fpsq_band_create_coo(C.byref(coo), qp.n, qp.m, qp.nnz, r.ctypes.data, cidx.ctypes.data, 0, 0) == 0
    rc, msg = create_rc(coo, qp)
    assert rc == ERR_STATE and b"band_nlp_create" in msg and b"fpsq_band_create_coo" in msg
    assert lib.fpsq_band_destroy(coo) == 0


@pytest.mark.parametrize("sub", ["lbfgs", "trunk"])
def test_fps_solve_device_end_to_end(sub):
    """fps_solve_device on the nonlinear model from x0 = xhat + 0.1 (x - xhat), with the default sub-solver (gradients only)
    and with `trunk` (Hessian products, among them products after a rejected trial point: _DeviceNLPPenalty evaluates again
    at the point the sub-solver moved back to).  The returned point is checked INDEPENDENTLY
    in numpy with the solver's own score rule: primal |c(x*)|inf / max(|x*|, 1), dual |grad f + J'lambda|inf / max(|lambda|, 1),
    both <= 10 tol, tol = max(atol, rtol max(p0, d0)) from atol = rtol = sqrt(eps) -- the factor 10 covers the difference
    between the penalty gradient the loop stops on and the Lagrangian residual."""
    import torch

    from fps_amd.fps_solve import fps_solve_device

    qp = _small()
    data = _data(qp)
    nlp = nlpmodels.SepQuadConModel(data)
    x0 = qp.xhat + 0.1 * (qp.x - qp.xhat)
    dev = DeviceBandSepQuadNLP(data)
    st = fps_solve_device(dev, torch.from_numpy(x0).to(torch.device("cuda", 0)), max_iter=30, subproblem_solver=sub)
    xs, lam = st.solution.cpu().numpy(), st.multipliers.cpu().numpy()
    p0 = np.abs(nlp.cons(x0)).max() / max(np.linalg.norm(x0), 1.0)
    d0 = np.abs(nlp.grad(x0)).max()
    tol = max(SE, SE * max(p0, d0))
    primal = np.abs(nlp.cons(xs)).max() / max(np.linalg.norm(xs), 1.0)
    dual = np.abs(nlp.grad(xs) + nlp.jtprod(xs, lam)).max() / max(np.linalg.norm(lam), 1.0)
    info = dev.info()
    print(f"\nfps_solve_device: {st.status} in {st.iter} outer iterations, primal {primal:.2e} dual {dual:.2e} tol {tol:.2e}, "
          f"{st.solver_specific}, factorizations {info['factorizations']}")
    assert st.status == "first_order"
    assert primal <= 10 * tol and dual <= 10 * tol
    assert info["factorizations"] == st.solver_specific["objgrad_calls"]
    dev.close()
