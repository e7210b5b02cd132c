"""Elementwise function terms on the banded device-resident nonlinear model (fpsq_band_nlp_create_fn, DeviceBandSepFuncNLP,
DeviceArrowBandSepFuncNLP): c_i(x) = sum_j (A_ij x_j + H_ij phi(x_j)) - b_i with phi per entry from {1/2 x^2, x^3/6, sin, cos,
exp, tanh}.  Every test goes through the C ABI by way of the new classes.

Yardstick: the CPU restatement tests/sepfunc_ref.py (exact KKT solves at J(x), the gradient in the -ys form, the mirror's
hprod_) at the bar tests/test_gpu_band_nlp.py holds these quantities to: max|a - b| / max|b| <= 1e-9 per vector, and here
|fx - ref| <= 1e-12 |ref|.  The device's sin / cos / exp / tanh are a few ulp from numpy's, which costs nothing at 1e-9.
tests/test_band_fn_nlp_cpu.py shows that the restatement's gx and c move by more than 1 (relative) when the codes are ignored,
and that every input used here is well posed (sigma_min(J(x)) >= 1/2 sigma_min(A), curvature 0.1).

Shapes: the 14 cases of tests/lane_group_cases.py (every lane-group width of k_bn_tvals_fn, k_bn_cons_fn and the FN form of
k_bn_prologue on both sides; `stride` reaches the second trip of their capped grids and of k_bn_vals_fn's) and the six arrow
shapes of tests/test_gpu_band_arrow_nlp.py (border rows, long columns, both, reordered, two chains).  fpsq_band_get_info has
no wait counters (a band handle runs no bounded waits of the iterative kind); the tests assert regularized_pivots == 0 where
the existing band tests do."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import fps_amd  # noqa: E402,F401
import lane_group_cases as lg  # noqa: E402
import test_gpu_band_arrow_nlp as arrow  # noqa: E402
from fps_amd import _lib, nlpmodels, problems  # noqa: E402
from fps_amd.device_qp import (DeviceArrowBandSepFuncNLP, DeviceArrowBandSepQuadNLP, DeviceBandEqQP,  # noqa: E402
                               DeviceBandSepFuncNLP, DeviceBandSepQuadNLP)
from fps_amd.qdsolver import FpsqError  # noqa: E402
from sepfunc_ref import CURV, SepFuncRef, exact_fn, fn_codes, fn_data, fn_data_of  # noqa: E402
from test_gpu_band_nlp import _objgrad, _small  # noqa: E402

pytestmark = pytest.mark.gpu

SE = float(np.sqrt(np.finfo(float).eps))
SIGMA = lg.SIGMA
BAR, BAR_FX = 1e-9, 1e-12
ERR_ARG, ERR_STATE = -1, -3
PAIRS = ((0.0, 0.0), (1.0, 0.5))   # (rho, eta)
KEYS = ("fx", "gx", "ys", "gs", "c", "Hv2", "Hv1")


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def _v(qp):
    return np.random.default_rng(0).standard_normal(qp.n)


def _evaluate(dev, rho, eta, x=None):
    """cons, one objgrad with every output and both Hessian products at x (default qp.x), xk = qp.xhat"""
    qp = dev.qp
    x = qp.x if x is None else x
    dev.rho, dev.eta = rho, eta
    c = np.full(qp.m, np.nan)
    assert dev.cons(x, c) == 0
    fx, rc, gx, ys, gs = _objgrad(dev, x, qp.xhat)
    assert rc == 0
    Hv2, Hv1 = np.full(qp.n, np.nan), np.full(qp.n, np.nan)
    assert dev.hprod(_v(qp), Hv2, 2) == 0 and dev.hprod(_v(qp), Hv1, 1) == 0
    return {"fx": fx, "gx": gx, "ys": ys, "gs": gs, "c": c, "Hv2": Hv2, "Hv1": Hv1}


def _same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in KEYS)


def _reference(ref, qp):
    out = {}
    for rho, eta in PAIRS:
        ref.pen.rho, ref.pen.eta = rho, eta
        e = ref.objgrad(qp.x)
        e["Hv2"], e["Hv1"] = ref.hprod(qp.x, _v(qp), 2), ref.hprod(qp.x, _v(qp), 1)
        for a in e.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        out[(rho, eta)] = e
    return out


@functools.lru_cache(maxsize=None)
def _expected(name, delta):
    """the restatement on a lane-group case at x = qp.x, xk = qp.xhat: one dict per (rho, eta), computed once, left unchanged"""
    return _reference(exact_fn(name, delta), lg.qp(name))


# ---- 1: every lane-group width and the second grid-stride trip

@pytest.mark.parametrize("delta", [0.0, SE], ids=["delta0", "deltaSE"])
@pytest.mark.parametrize("name", lg.NAMES)
def test_every_lane_group_width_matches_the_exact_restatement(name, delta):
    qp, data, case = lg.qp(name), fn_data(name), lg.CASES[name]
    assert set(np.unique(data.codes)) == set(range(6))
    dev = DeviceBandSepFuncNLP(data, sigma=SIGMA, rho=0.0, delta=delta, eta=0.0)
    info = dev.info()
    assert info["chains"] == case.band["chains"] and info["reordered"] == case.band["reordered"]
    for rho, eta in PAIRS:
        got, e = _evaluate(dev, rho, eta), _expected(name, delta)[(rho, eta)]
        errs = {k: _rel(got[k], e[k]) for k in KEYS[1:]}
        errs["fx"] = abs(got["fx"] - e["fx"]) / abs(e["fx"])
        print(f"\n{name} lgA={case.lgA} lgT={case.lgT} delta={delta:.1e} rho={rho} eta={eta}: "
              + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
        for k in KEYS[1:]:
            assert errs[k] <= BAR, (k, errs[k])
        assert abs(got["fx"] - e["fx"]) <= BAR_FX * abs(e["fx"])
    assert dev.info()["factorizations"] == len(PAIRS) and dev.info()["regularized_pivots"] == 0
    # the handle's values are J(x): fpsq_band_jac_mul multiplies with it
    J = nlpmodels.SepFuncConModel(data)._J(qp.x)
    v, u = _v(qp), np.random.default_rng(2).standard_normal(qp.m)
    y, z = np.empty(qp.m), np.empty(qp.n)
    assert dev.jac_mul(0, 1.0, v, 0.0, y) == 0 and dev.jac_mul(1, 1.0, u, 0.0, z) == 0
    assert _rel(y, J @ v) < 1e-13 and _rel(z, J.T @ u) < 1e-13
    dev.close()


# ---- 2: arrow handles

@functools.lru_cache(maxsize=None)
def _arrow_problem(case):
    """(qp, data, border rows, long columns): the shape of tests/test_gpu_band_arrow_nlp.py with the function model on it"""
    qp, rows, cols = arrow.CASES[case][0]()
    return qp, fn_data_of(qp), rows, cols


@functools.lru_cache(maxsize=None)
def _arrow_expected(case):
    qp, data, _, _ = _arrow_problem(case)
    return _reference(SepFuncRef(data, SIGMA, 0.0, arrow.CASES[case][1], 0.0, qp.xhat, kept=True), qp)


def _arrow_device(case):
    _, data, _, _ = _arrow_problem(case)
    border, cols = arrow.CASES[case][2]
    dev = DeviceArrowBandSepFuncNLP(data, border=border, cols=cols, sigma=SIGMA, rho=0.0, delta=arrow.CASES[case][1], eta=0.0)
    info = dev.info()
    for k, want in arrow.CASES[case][3].items():
        assert info[k] == want, (k, info)
    return dev


def _arrow_check(dev, case, label):
    qp, data, rows, cols = _arrow_problem(case)
    r = np.repeat(np.arange(qp.m), np.diff(qp.rowptr))
    assert not cols.size or np.any(data.codes[np.isin(qp.colind, cols)] != 0)
    assert not rows.size or np.any(data.codes[np.isin(r, rows)] != 0)
    out = []
    for rho, eta in PAIRS:
        got, e = _evaluate(dev, rho, eta), _arrow_expected(case)[(rho, eta)]
        errs = arrow._errors(got, e, rows, cols)   # every vector, and the long columns' / border rows' entries on their own
        print(f"\n{label} rho={rho} eta={eta}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
        assert max(v for k, v in errs.items() if k != "fx") <= BAR, errs
        assert abs(got["fx"] - e["fx"]) <= BAR_FX * abs(e["fx"])
        out.append(got)
    assert dev.info()["regularized_pivots"] == 0
    return out


@pytest.mark.parametrize("case", list(arrow.CASES))
def test_arrow_handles_match_the_exact_restatement(case):
    dev = _arrow_device(case)
    _arrow_check(dev, case, case)
    assert dev.info()["factorizations"] == len(PAIRS)
    dev.close()


@pytest.mark.parametrize("form,case,env", [("nested", "m640-r16-c16-stride-first", ("FPSQ_ARROW_FUSED", "0")),
                                           ("by-row-pairs", arrow.CASE_643, ("FPSQ_BAND_FORM", "1"))])
def test_the_other_correction_and_formation_forms_meet_the_same_bars(form, case, env, monkeypatch):
    monkeypatch.setenv(*env)   # (both are read at create)
    dev = _arrow_device(case)
    _arrow_check(dev, case, f"{case}, {form}")
    dev.close()


# ---- 3: identities, bit for bit

class _NullCodes(DeviceBandSepFuncNLP):
    def _model_extra(self, nlp_data):
        return (None,)


class _NullCodesArrow(DeviceArrowBandSepFuncNLP):
    def _model_extra(self, nlp_data):
        return (None,)


def _zero_codes(data):
    return problems.SepFuncNLP(data.qp, data.hvals, data.b, np.zeros(data.hvals.size, dtype=np.uint8))


@pytest.mark.parametrize("name", ["lgT-8", "both-64-shuffled", "stride"])   # plain, reordered, two chains
def test_all_codes_zero_and_null_codes_give_the_bits_of_the_separable_model(name):
    data = lg.nlp_data(name)
    want = None
    for cls, d in ((DeviceBandSepQuadNLP, data), (DeviceBandSepFuncNLP, _zero_codes(data)), (_NullCodes, data)):
        dev = cls(d, sigma=SIGMA, rho=1.0, delta=SE, eta=0.5)
        got = _evaluate(dev, 1.0, 0.5)
        dev.close()
        want = got if want is None else want
        assert _same_bits(got, want), cls.__name__


def test_all_codes_zero_and_null_codes_give_the_bits_of_the_separable_model_on_an_arrow_handle():
    _, data, _, _ = arrow._problem(arrow.CASE_643)
    border, cols = arrow.CASES[arrow.CASE_643][2]
    want = None
    for cls, d in ((DeviceArrowBandSepQuadNLP, data), (DeviceArrowBandSepFuncNLP, _zero_codes(data)), (_NullCodesArrow, data)):
        dev = cls(d, border=border, cols=cols, sigma=SIGMA, rho=1.0, delta=SE, eta=0.5)
        assert dev.info()["border_rows"] == 3 and dev.info()["border_cols"] == 5
        got = _evaluate(dev, 1.0, 0.5)
        dev.close()
        want = got if want is None else want
        assert _same_bits(got, want), cls.__name__


# ---- 4: the linear limit

@pytest.mark.parametrize("name", ["lgT-8", "both-64-shuffled"])
def test_linear_limit_agrees_with_the_linear_model(name):
    """h_vals = 0 under arbitrary codes: the model IS the eq-QP (the function kernels run: the codes are not all 0)"""
    qp = lg.qp(name)
    data = problems.SepFuncNLP(qp, np.zeros_like(qp.vals), qp.b.copy(), fn_codes(qp.vals.size))
    v = _v(qp)
    for delta in (0.0, SE):
        lin = DeviceBandEqQP(qp, sigma=SIGMA, rho=1.0, delta=delta, eta=0.5)
        dev = DeviceBandSepFuncNLP(data, sigma=SIGMA, rho=1.0, delta=delta, eta=0.5)
        a, b = _objgrad(lin, qp.x, qp.xhat), _objgrad(dev, qp.x, qp.xhat)
        assert a[1] == 0 and b[1] == 0
        assert abs(a[0] - b[0]) <= 1e-12 * abs(a[0])
        for p, q in zip(a[2:], b[2:]):
            assert _rel(q, p) < 1e-12
        Hl, H2, H1 = np.empty(qp.n), np.empty(qp.n), np.empty(qp.n)
        assert lin.hprod(v, Hl, 2) == 0 and dev.hprod(v, H2, 2) == 0 and dev.hprod(v, H1, 1) == 0
        assert _rel(H2, Hl) < 1e-12 and _rel(H1, H2) < 1e-12
        lin.close()
        dev.close()


# ---- 5: repeatability and state

def test_repeatability_placement_and_no_state_between_evaluations():
    import torch

    qp = _small()
    data = fn_data_of(qp)
    x1, x2, xk = qp.x, qp.point(2), qp.xhat
    on = torch.device("cuda", 0)
    v = _v(qp)

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

    dev = DeviceBandSepFuncNLP(data, sigma=SIGMA, rho=1.0, delta=SE, eta=0.5)
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
    # a second x: another J and another G, and nothing of the first evaluation is left -- a fresh handle gives the same bits
    second = _objgrad(dev, x2, xk)
    h2 = hprods(dev, False)
    fresh_dev = DeviceBandSepFuncNLP(data, sigma=SIGMA, rho=1.0, delta=SE, eta=0.5)
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


def test_state_rules_and_argument_checks():
    lib = _lib.load()
    qp = _small()
    data = fn_data_of(qp)
    x, xk = qp.x, qp.xhat
    v, Hv = _v(qp), np.empty(qp.n)
    dev = DeviceBandSepFuncNLP(data, sigma=SIGMA, rho=1.0, delta=SE, eta=0.0)
    h, q = dev._h, dev._q

    def hprod_rc(model=None, ha=2):
        return lib.fpsq_band_nlp_hprod(h, model or q, v.ctypes.data, SIGMA, 1.0, 0.0, ha, Hv.ctypes.data)

    def create_rc(handle, codes, out):
        return lib.fpsq_band_nlp_create_fn(handle, qp.qdiag.ctypes.data, qp.d.ctypes.data, data.b.ctypes.data, qp.vals.ctypes.data,
                                           data.hvals.ctypes.data, codes.ctypes.data, C.byref(out))

    # before any objgrad
    assert hprod_rc() == ERR_STATE and b"objgrad" in lib.fpsq_band_last_error(h)
    with pytest.raises(FpsqError):
        dev.hprod(v, Hv)
    first = _objgrad(dev, x, xk)
    assert first[1] == 0 and hprod_rc() == 0 and hprod_rc(ha=1) == 0
    assert hprod_rc(ha=3) == ERR_ARG
    # after ANOTHER model's objgrad on the handle
    other = C.c_void_p()
    assert create_rc(h, data.codes, other) == 0
    fx = C.c_double()
    assert lib.fpsq_band_nlp_objgrad(h, other, qp.point(2).ctypes.data, SIGMA, 1.0, 0.0, SE, None, C.byref(fx), None, None, None,
                                     None) == 0
    assert hprod_rc() == ERR_STATE and b"factorised again" in lib.fpsq_band_last_error(h)
    assert hprod_rc(other) == 0
    back = _objgrad(dev, x, xk)
    for a, b in zip(first, back):
        assert np.array_equal(a, b)
    assert hprod_rc() == 0 and hprod_rc(other) == ERR_STATE
    assert lib.fpsq_band_nlp_destroy(other) == 0
    # after fpsq_band_factorize
    assert lib.fpsq_band_factorize(h, qp.vals.ctypes.data, SE, None) == 0
    assert hprod_rc() == ERR_STATE and hprod_rc(ha=1) == ERR_STATE
    # a code that is not in the table: the first offending entry is named
    bad = data.codes.copy()
    bad[[37, 90]] = 6, 200
    out = C.c_void_p()
    assert create_rc(h, bad, out) == ERR_ARG
    msg = lib.fpsq_band_last_error(h)
    assert b"band_nlp_create_fn" in msg and b"fn_codes[37] = 6" in msg
    with pytest.raises(FpsqError):
        DeviceBandSepFuncNLP(problems.SepFuncNLP(qp, data.hvals, data.b, bad))
    dev.close()
    # a handle of a _coo entry
    coo = C.c_void_p()
    r = np.repeat(np.arange(qp.m, dtype=np.int64), np.diff(qp.rowptr))
    cidx = qp.colind.astype(np.int64)
    assert lib.fpsq_band_create_coo(C.byref(coo), qp.n, qp.m, qp.nnz, r.ctypes.data, cidx.ctypes.data, 0, 0) == 0
    assert create_rc(coo, data.codes, out) == ERR_STATE
    msg = lib.fpsq_band_last_error(coo)
    assert b"band_nlp_create_fn" in msg and b"fpsq_band_create_coo" in msg
    assert lib.fpsq_band_destroy(coo) == 0


# ---- 6: a non-finite J(x)

def test_a_non_finite_jacobian_is_refused_before_the_factorisation():
    """an argument check: the value launch sees exp(800) = inf, the objgrad returns before it enqueues the factorisation"""
    qp = _small()
    codes = np.zeros(qp.vals.size, dtype=np.uint8)
    k = int(qp.rowptr[200]) + 3
    codes[k] = problems.FN_EXP
    data = fn_data_of(qp, codes)
    assert data.hvals[k] != 0.0
    bad = qp.x.copy()
    bad[qp.colind[k]] = 800.0
    dev = DeviceBandSepFuncNLP(data, sigma=SIGMA, rho=1.0, delta=SE, eta=0.5)
    good = _evaluate(dev, 1.0, 0.5)
    assert dev.info()["factorizations"] == 1
    gx, ys, gs = np.full(qp.n, 7.0), np.full(qp.m, 8.0), np.full(qp.n, 9.0)
    with pytest.warns(UserWarning, match="non-finite"):
        fx, rc = dev.objgrad(bad, gx=gx, ys=ys, gs=gs, xk=qp.xhat)
    assert rc == 1 and np.isnan(fx)
    assert np.all(gx == 7.0) and np.all(ys == 8.0) and np.all(gs == 9.0)
    assert dev.info()["factorizations"] == 1                      # no numeric factorisation ran for it
    Hv = np.empty(qp.n)
    with pytest.raises(FpsqError):                                # and the model has no point: the state a failed one leaves
        dev.hprod(_v(qp), Hv)
    # the C entry itself: soft code 1, *fx = nan, *info = -1
    lib = _lib.load()
    cfx, where = C.c_double(1.0), C.c_int32(5)
    assert lib.fpsq_band_nlp_objgrad(dev._h, dev._q, bad.ctypes.data, SIGMA, 1.0, 0.5, SE, qp.xhat.ctypes.data, C.byref(cfx),
                                     gx.ctypes.data, ys.ctypes.data, gs.ctypes.data, C.byref(where)) == 1
    assert np.isnan(cfx.value) and where.value == -1 and np.all(gx == 7.0)
    # the next objgrad at qp.x gives the bits of a fresh handle's (which are those of before)
    after = _evaluate(dev, 1.0, 0.5)
    fresh_dev = DeviceBandSepFuncNLP(data, sigma=SIGMA, rho=1.0, delta=SE, eta=0.5)
    fresh = _evaluate(fresh_dev, 1.0, 0.5)
    assert _same_bits(after, fresh) and _same_bits(after, good)
    assert dev.info()["factorizations"] == 2
    dev.close()
    fresh_dev.close()


# ---- 7: end to end

@functools.lru_cache(maxsize=None)
def _pendulum():
    return problems.pendulum_like(2000)


def _solve(dev, sub):
    import torch

    from fps_amd.fps_solve import fps_solve_device

    x0 = torch.from_numpy(dev.qp.x.copy()).to(torch.device("cuda", 0))
    st = fps_solve_device(dev, x0, atol=SE, rtol=SE, max_iter=30, subproblem_solver=sub)
    return st, st.solution.cpu().numpy(), st.multipliers.cpu().numpy()


@pytest.mark.parametrize("sub", ["trunk", "lbfgs"])
def test_fps_solve_device_on_the_pendulum(sub):
    data = _pendulum()
    nlp = nlpmodels.SepFuncConModel(data)
    dev = DeviceBandSepFuncNLP(data)
    st, xs, lam = _solve(dev, sub)
    primal = np.max(np.abs(nlp.cons(xs)))
    dual = np.max(np.abs(nlp.grad(xs) + nlp.jtprod(xs, lam)))
    print(f"\npendulum N=2000, {sub}: {st.status} in {st.iter} outer iterations, |c| {primal:.2e}, "
          f"|grad f + J'lambda| {dual:.2e}, {st.solver_specific}, factorizations {dev.info()['factorizations']}")
    assert st.status == "first_order"
    assert primal <= 1e-8 and dual <= 1e-5
    assert dev.info()["regularized_pivots"] == 0
    dev.close()
    if sub == "trunk":   # the same model through the arrow handle's entry, nothing taken out of the band: the same bits
        adev = DeviceArrowBandSepFuncNLP(data, border=0, cols=0)
        st2, xs2, lam2 = _solve(adev, sub)
        adev.close()
        assert st2.status == st.status and st2.iter == st.iter
        assert np.array_equal(xs2, xs) and np.array_equal(lam2, lam)
