"""Elementwise function terms in the OBJECTIVE of the banded device-resident nonlinear model
(fpsq_band_nlp_set_objective_terms, DeviceBandSepQuadNLP.set_objective_terms and every subclass):
f(x) = 1/2 x' diag(q) x + d'x + sum_j w_j psi(x_j), psi per variable from {1/2 x^2, x^3/6, sin, cos, exp, tanh}.  Every test goes
through the C ABI by way of the classes.

Yardstick: the EXISTING CPU restatements (tests/sepquad_ref.py with kept factors, sepfunc_ref.py, coupled_quad_ref.py) on data that carries the
terms (tests/objfn_cases.py) -- they build nlpmodels' host classes, whose obj / grad / hprod honour them -- at the project's
bars: max|a - b| / max|b| <= 1e-9 per vector, |fx - ref| <= 1e-12 |ref|.  tests/test_band_objfn_nlp_cpu.py shows that dropping the
terms moves every vector by >= 1e-4 and fx by >= 1e-5 on every case used in part 1.

The new kernel k_bn_objfn runs on the grid of the prologue's objective slice, min(ceil(mpad / (256 / lgA)), 2048) workgroups,
each on a contiguous chunk of ceil(n / grid) entries, a thread striding its chunk by 256.  On the 14 lane-group cases:
  * `thin` and `lg2` (3 workgroups, n = 900, chunk 300): threads 0 .. 43 walk TWO entries, the others one;
  * `stride` (n = 9000, mpad = 8320, lgA = 64): 2080 tiles, the grid is the CAPPED one (2048), chunk 5, and 248 workgroups
    start behind n and write a zero partial;
  * `m-near-n`, `ragged` and the two 600-column cases: a last chunk shorter than the others (2 of 9, 2 of 11) and 5 .. 9 empty
    workgroups; `wide-rows`, `lg4-2`, `lg8-4`, `lg16-2`: chunks that divide n, most threads of a workgroup idle.
tests/test_band_objfn_nlp_cpu.py recomputes these facts (test_the_partition_the_lane_group_cases_reach)."""
import ctypes as C
import dataclasses
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import fps_amd  # noqa: E402,F401
import coupled_arrow_cases as ca  # noqa: E402
import coupled_cases as cc  # noqa: E402
import lane_group_cases as lg  # noqa: E402
import objfn_cases as oc  # noqa: E402
import test_gpu_band_arrow_nlp as arrow  # noqa: E402
from coupled_quad_ref import CoupledQuadRef  # noqa: E402
from fps_amd import _lib, nlpmodels, problems  # noqa: E402
from fps_amd.device_qp import (DeviceArrowBandCoupledQuadNLP, DeviceArrowBandSepQuadNLP, DeviceBandCoupledQuadNLP,  # noqa: E402
                               DeviceBandSepFuncNLP, DeviceBandSepQuadNLP)
from fps_amd.qdsolver import FpsqError  # noqa: E402
from sepfunc_ref import fn_codes, fn_data  # noqa: E402
from test_gpu_band_fn_nlp import KEYS, PAIRS, _evaluate, _reference, _rel, _same_bits, _v  # noqa: E402
from test_gpu_band_nlp import _objgrad  # noqa: E402

pytestmark = pytest.mark.gpu

SE = float(np.sqrt(np.finfo(float).eps))
SIGMA = lg.SIGMA
BAR, BAR_FX = 1e-9, 1e-12
ERR_ARG, ERR_STATE = -1, -3
KW = dict(sigma=SIGMA, rho=1.0, delta=SE, eta=0.5)


def _errs(got, e):
    errs = {k: _rel(got[k], e[k]) for k in KEYS[1:]}
    errs["fx"] = abs(got["fx"] - e["fx"]) / abs(e["fx"])
    return errs


def _hold(label, got, e, extra=None):
    """print every figure, then hold it to its bar"""
    errs = _errs(got, e) if extra is None else extra
    print(f"\n{label}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert max(v for k, v in errs.items() if k != "fx") <= BAR, errs
    assert abs(got["fx"] - e["fx"]) <= BAR_FX * abs(e["fx"]), errs["fx"]


# ---- 1: the lane-group cases

@functools.lru_cache(maxsize=None)
def _expected(name, delta):
    """the restatement with terms on a lane-group case at x = qp.x, xk = qp.xhat: one dict per (rho, eta), computed once"""
    return _reference(oc.exact_objfn(name, delta), lg.qp(name))


@pytest.mark.parametrize("delta", [0.0, SE], ids=["delta0", "deltaSE"])
@pytest.mark.parametrize("name", lg.NAMES)
def test_the_function_model_with_terms_on_every_lane_group_case(name, delta):
    data, case = oc.objfn_data(name), lg.CASES[name]
    w, codes = data.obj_w, data.obj_codes
    assert set(np.unique(codes[w != 0])) == set(range(6)) and np.any(w == 0)
    dev = DeviceBandSepFuncNLP(data, sigma=SIGMA, rho=0.0, delta=delta, eta=0.0)    # (the constructor sets the terms)
    info = dev.info()
    assert info["chains"] == case.band["chains"] and info["reordered"] == case.band["reordered"]
    for rho, eta in PAIRS:
        _hold(f"{name} lgA={case.lgA} lgT={case.lgT} delta={delta:.1e} rho={rho} eta={eta}", _evaluate(dev, rho, eta),
              _expected(name, delta)[(rho, eta)])
    assert dev.info()["factorizations"] == len(PAIRS) and dev.info()["regularized_pivots"] == 0
    dev.close()


# ---- 2: the other four kinds of model

def _pairs(dev, ref, label, errors=None):
    e = _reference(ref, dev.qp)
    for rho, eta in PAIRS:
        got = _evaluate(dev, rho, eta)
        _hold(f"{label} rho={rho} eta={eta}", got, e[(rho, eta)], None if errors is None else errors(got, e[(rho, eta)]))
    assert dev.info()["factorizations"] == len(PAIRS) and dev.info()["regularized_pivots"] == 0
    dev.close()


def test_the_separable_model_with_terms():
    name = "m-near-n"
    data = oc.with_terms(lg.nlp_data(name))
    _pairs(DeviceBandSepQuadNLP(data, sigma=SIGMA, rho=0.0, delta=SE, eta=0.0),
           oc.SepQuadKeptRef(data, SIGMA, 0.0, SE, 0.0, data.qp.xhat), f"separable {name}")


def test_the_coupled_model_with_terms():
    name = "row-shuffled"
    data = oc.with_terms(cc.data(name))
    assert data.nterms > 0
    dev = DeviceBandCoupledQuadNLP(data, sigma=SIGMA, rho=0.0, delta=SE, eta=0.0)
    assert dev.info()["reordered"] == 1
    _pairs(dev, CoupledQuadRef(data, SIGMA, 0.0, SE, 0.0, data.qp.xhat, keep_factors=True), f"coupled {name}")


@pytest.mark.parametrize("case", list(arrow.CASES))
def test_the_arrow_model_with_terms(case):
    """k_bn_lc_epilogue reads q at the long columns: a weight that is not 0 on at least one of them, and the long columns'
    entries of gx, gs and both Hessian products held to the bar on their own (arrow._errors)"""
    qp, plain, rows, cols = arrow._problem(case)
    data = oc.with_terms(plain, always=cols[:1])     # (the first long column carries a weight whatever the draw says)
    assert not cols.size or np.any(data.obj_w[cols] != 0)
    border, lcols = arrow.CASES[case][2]
    delta = arrow.CASES[case][1]
    dev = DeviceArrowBandSepQuadNLP(data, border=border, cols=lcols, sigma=SIGMA, rho=0.0, delta=delta, eta=0.0)
    for k, want in arrow.CASES[case][3].items():
        assert dev.info()[k] == want, k
    _pairs(dev, oc.SepQuadKeptRef(data, SIGMA, 0.0, delta, 0.0, qp.xhat), f"arrow {case}",
           lambda got, e: arrow._errors(got, e, rows, cols))


def test_the_coupled_arrow_model_with_terms():
    name = arrow.CASE_643
    plain, rows, cols = ca.problem(name)
    data = oc.with_terms(plain, always=cols[:1])
    assert np.any(data.obj_w[cols] != 0) and ca.counts(name)[1] > 0       # terms of both kinds meet at a long column
    border, lcols = ca.limits(name)
    dev = DeviceArrowBandCoupledQuadNLP(data, border=border, cols=lcols, sigma=SIGMA, rho=0.0, delta=ca.delta(name), eta=0.0)
    for k, want in ca.want_info(name).items():
        assert dev.info()[k] == want, k
    _pairs(dev, CoupledQuadRef(data, SIGMA, 0.0, ca.delta(name), 0.0, data.qp.xhat, keep_factors=True), f"coupled arrow {name}",
           lambda got, e: arrow._errors(got, e, rows, cols))


# ---- 3: identities

def _arrow_643(data):
    border, cols = arrow.CASES[arrow.CASE_643][2]
    return DeviceArrowBandSepQuadNLP(data, border=border, cols=cols, **KW)


@pytest.mark.parametrize("shape", ["lgT-8", "both-64-shuffled", "stride", arrow.CASE_643])   # plain, reordered, two chains, arrow
def test_never_set_and_set_then_removed_give_the_bits_of_a_fresh_model(shape):
    if shape == arrow.CASE_643:
        make, data = _arrow_643, arrow._problem(shape)[1]
    else:
        make, data = (lambda d: DeviceBandSepFuncNLP(d, **KW)), fn_data(shape)
    w, codes = oc.terms(data.qp.n)
    fresh = make(data)
    want = _evaluate(fresh, 1.0, 0.5)
    fresh.close()
    dev = make(data)
    assert dev.set_objective_terms(w, codes) == 0
    moved = _evaluate(dev, 1.0, 0.5)
    assert _rel(moved["gx"], want["gx"]) > 1e-4 and np.array_equal(moved["c"], want["c"])
    assert dev.set_objective_terms(None) == 0 and dev.obj_w is None
    assert _same_bits(_evaluate(dev, 1.0, 0.5), want)
    dev.close()
    # a model created WITH terms (the constructor's call), then cleared
    dev = make(problems.with_objective_terms(data, w, codes))
    assert np.array_equal(dev.obj_w, w)
    assert dev.set_objective_terms(None) == 0
    assert _same_bits(_evaluate(dev, 1.0, 0.5), want)
    dev.close()


def test_zero_weights_are_not_evaluated():
    """w = 0 everywhere under arbitrary codes, one of them exp at x_j = 800 (a column of `thin` that lies in no constraint, so
    the point is an ordinary one for J): rc 0 and the model without terms to 1e-12"""
    name = "thin"
    data = lg.nlp_data(name)
    qp = data.qp
    j = int(np.flatnonzero(np.bincount(qp.colind, minlength=qp.n) == 0)[0])
    _, codes = oc.terms(qp.n)
    codes[j] = problems.FN_EXP
    codes[(j + 1) % qp.n] = 200              # (no function code at all: harmless under w = 0)
    x = qp.x.copy()
    x[j] = 800.0
    plain = DeviceBandSepQuadNLP(data, **KW)
    want = _evaluate(plain, 1.0, 0.5, x)
    plain.close()
    dev = DeviceBandSepQuadNLP(problems.with_objective_terms(data, np.zeros(qp.n), codes), **KW)
    got = _evaluate(dev, 1.0, 0.5, x)
    errs = _errs(got, want)
    print("\nw = 0: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) <= 1e-12
    assert dev.info()["regularized_pivots"] == 0
    dev.close()


@pytest.mark.parametrize("name", ["lgT-8", "both-64-shuffled"])
def test_code_0_is_a_shift_of_qdiag(name):
    data = lg.nlp_data(name)
    qp = data.qp
    w, _ = oc.terms(qp.n)
    shifted = dataclasses.replace(data, qp=dataclasses.replace(qp, qdiag=qp.qdiag + w))
    a, b = DeviceBandSepQuadNLP(shifted, **KW), DeviceBandSepQuadNLP(problems.with_objective_terms(data, w), **KW)
    want, got = _evaluate(a, 1.0, 0.5), _evaluate(b, 1.0, 0.5)
    errs = _errs(got, want)
    print(f"\n{name}, codes 0: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) <= 1e-12
    a.close()
    b.close()


@pytest.mark.parametrize("name", ["lgT-8", "both-64-shuffled"])
def test_the_two_hessian_products_agree_in_the_linear_limit(name):
    """h_vals = 0 under arbitrary codes: the constraints are linear, and with them Val(1) = Val(2) whatever the objective"""
    qp = lg.qp(name)
    data = oc.with_terms(problems.SepFuncNLP(qp, np.zeros_like(qp.vals), qp.b.copy(), fn_codes(qp.vals.size)))
    dev = DeviceBandSepFuncNLP(data, **KW)
    got = _evaluate(dev, 1.0, 0.5)
    model = nlpmodels.SepFuncConModel(data)
    assert _rel(got["Hv1"], got["Hv2"]) <= 1e-12 and _rel(got["c"], model.cons(qp.x)) <= 1e-12
    dev.close()


# ---- 4: state rules and argument checks

def test_state_rules_and_argument_checks():
    lib = _lib.load()
    data = fn_data("lgT-8")
    qp = data.qp
    w, codes = oc.terms(qp.n)
    v, Hv = _v(qp), np.empty(qp.n)
    dev = DeviceBandSepFuncNLP(data, **KW)
    h, q = dev._h, dev._q

    def set_rc(handle, model, wv, cv):
        return lib.fpsq_band_nlp_set_objective_terms(handle, model, None if wv is None else wv.ctypes.data,
                                                     None if cv is None else cv.ctypes.data)

    # a code outside the table: refused under a weight, with the first such j named, accepted under w_j = 0
    on, off = np.flatnonzero(w != 0), np.flatnonzero(w == 0)
    bad = codes.copy()
    bad[[on[5], on[9]]] = 6, 200
    bad[off[0]] = 77
    assert set_rc(h, q, w, bad) == ERR_ARG
    msg = lib.fpsq_band_last_error(h)
    assert b"band_nlp_set_objective_terms" in msg and f"codes[{on[5]}] = 6".encode() in msg
    with pytest.raises(FpsqError):
        dev.set_objective_terms(w, bad)
    ok = codes.copy()
    ok[off[0]] = 77
    assert set_rc(h, q, w, ok) == 0
    assert set_rc(None, q, w, codes) == ERR_ARG and set_rc(h, None, w, codes) == ERR_ARG
    # a model of another handle
    other = DeviceBandSepFuncNLP(data, **KW)
    assert set_rc(h, other._q, w, codes) == ERR_ARG and b"another handle" in lib.fpsq_band_last_error(h)
    assert set_rc(other._h, q, None, None) == ERR_ARG
    other.close()
    # hprod after the setter: FPSQ_ERR_STATE until the next objgrad, whether terms are set, changed or removed
    assert dev.set_objective_terms(None) == 0
    first = _evaluate(dev, 1.0, 0.5)
    for args in ((w, codes), (w, None), (None, None)):
        assert dev.hprod(v, Hv, 2) == 0
        assert set_rc(h, q, *args) == 0
        for ha in (2, 1):
            assert lib.fpsq_band_nlp_hprod(h, q, v.ctypes.data, SIGMA, 1.0, 0.5, ha, Hv.ctypes.data) == ERR_STATE
            assert b"no successful fpsq_band_nlp_objgrad" in lib.fpsq_band_last_error(h)
        assert _objgrad(dev, qp.x, qp.xhat)[1] == 0
    # terms changed between two objgrads: the second gives the bits of a fresh model with the second terms
    w2, codes2 = oc.terms(qp.n, seed=14)
    assert dev.set_objective_terms(w, codes) == 0
    one = _evaluate(dev, 1.0, 0.5)
    assert dev.set_objective_terms(w2, codes2) == 0
    two = _evaluate(dev, 1.0, 0.5)
    fresh = DeviceBandSepFuncNLP(problems.with_objective_terms(data, w2, codes2), **KW)
    assert _same_bits(two, _evaluate(fresh, 1.0, 0.5)) and not _same_bits(two, one) and not _same_bits(one, first)
    fresh.close()
    dev.close()


# ---- 5: a non-finite objective

@pytest.mark.parametrize("kind", ["separable", "function", "function, J(x) too"])
def test_a_non_finite_objective_is_refused_before_the_factorisation(kind):
    """one exp entry with w_j != 0 at x_j = 800, on a column of `thin` that lies in no constraint (J(x) stays finite); in the
    third case on a column whose constraint entries carry exp as well, so that both kinds of terms raise the word"""
    lib = _lib.load()
    name = "thin"
    plain = lg.nlp_data(name) if kind == "separable" else fn_data(name)
    cls = DeviceBandSepQuadNLP if kind == "separable" else DeviceBandSepFuncNLP
    qp = plain.qp
    if kind.endswith("too"):
        k = int(np.flatnonzero((plain.codes == problems.FN_EXP) & (plain.hvals != 0))[0])
        j, said = int(qp.colind[k]), b"J(x) and the objective"
    else:
        j, said = int(np.flatnonzero(np.bincount(qp.colind, minlength=qp.n) == 0)[0]), b"the objective's function terms hold"
    w, codes = oc.terms(qp.n)
    w[j], codes[j] = 0.75, problems.FN_EXP
    data = problems.with_objective_terms(plain, w, codes)
    bad = qp.x.copy()
    bad[j] = 800.0
    dev = cls(data, **KW)
    good = _evaluate(dev, 1.0, 0.5)
    assert dev.info()["factorizations"] == 1
    gx, ys, gs = np.full(qp.n, 7.0), np.full(qp.m, 8.0), np.full(qp.n, 9.0)
    with pytest.warns(UserWarning, match="non-finite"):
        fx, rc = dev.objgrad(bad, gx=gx, ys=ys, gs=gs, xk=qp.xhat)
    assert rc == 1 and np.isnan(fx)
    assert said in lib.fpsq_band_last_error(dev._h)
    assert np.all(gx == 7.0) and np.all(ys == 8.0) and np.all(gs == 9.0)
    assert dev.info()["factorizations"] == 1                      # no numeric factorisation ran for it
    with pytest.raises(FpsqError):                                # and the model has no point
        dev.hprod(_v(qp), np.empty(qp.n))
    cfx, where = C.c_double(1.0), C.c_int32(5)
    assert lib.fpsq_band_nlp_objgrad(dev._h, dev._q, bad.ctypes.data, SIGMA, 1.0, 0.5, SE, qp.xhat.ctypes.data, C.byref(cfx),
                                     gx.ctypes.data, ys.ctypes.data, gs.ctypes.data, C.byref(where)) == 1
    assert np.isnan(cfx.value) and where.value == -1 and np.all(gx == 7.0)
    # the word is cleared: the next objgrad at qp.x gives the bits of a fresh handle's (which are those of before)
    after = _evaluate(dev, 1.0, 0.5)
    fresh_dev = cls(data, **KW)
    assert _same_bits(after, _evaluate(fresh_dev, 1.0, 0.5)) and _same_bits(after, good)
    assert dev.info()["factorizations"] == 2
    dev.close()
    fresh_dev.close()


# ---- 6: pointers and repetition

def test_host_and_device_arguments_and_repeated_calls_give_the_same_bits():
    import torch

    data = lg.nlp_data("lgT-8")
    qp = data.qp
    w, codes = oc.terms(qp.n)
    on = torch.device("cuda", 0)
    dev = DeviceBandSepQuadNLP(data, **KW)
    assert dev.set_objective_terms(w, codes) == 0
    host = _evaluate(dev, 1.0, 0.5)
    assert _same_bits(_evaluate(dev, 1.0, 0.5), host)                                  # the same model again
    assert dev.set_objective_terms(w, codes) == 0 and _same_bits(_evaluate(dev, 1.0, 0.5), host)   # the same terms again
    assert dev.set_objective_terms(torch.from_numpy(w).to(on), torch.from_numpy(codes).to(on)) == 0
    assert np.array_equal(dev.obj_w, w) and np.array_equal(dev.obj_codes, codes)
    assert _same_bits(_evaluate(dev, 1.0, 0.5), host)
    devt = _objgrad(dev, qp.x, qp.xhat, on=on)                                        # x, xk and the outputs on the device
    assert devt[1] == 0 and devt[0] == host["fx"]
    assert all(np.array_equal(a, host[k]) for a, k in zip(devt[2:], ("gx", "ys", "gs")))
    # NULL codes are codes 0, from either side
    zero = np.zeros(qp.n, dtype=np.uint8)
    assert dev.set_objective_terms(w, zero) == 0
    want = _evaluate(dev, 1.0, 0.5)
    assert dev.set_objective_terms(torch.from_numpy(w).to(on)) == 0 and np.all(dev.obj_codes == 0)
    assert _same_bits(_evaluate(dev, 1.0, 0.5), want) and not _same_bits(want, host)
    dev.close()


# ---- 7: end to end

def _solve(dev):
    import torch

    from fps_amd.fps_solve import fps_solve_device

    x0 = torch.from_numpy(dev.qp.x.copy()).to(torch.device("cuda", 0))
    st = fps_solve_device(dev, x0, atol=SE, rtol=SE, max_iter=30, subproblem_solver="trunk")
    return st, st.solution.cpu().numpy(), st.multipliers.cpu().numpy()


def test_fps_solve_device_on_the_pendulum_with_energy_terms():
    data = problems.pendulum_energy_like(200)
    assert (data.qp.n, data.qp.m) == (602, 400)
    nlp = nlpmodels.SepFuncConModel(data)
    dev = DeviceBandSepFuncNLP(data)
    st, xs, lam = _solve(dev)
    primal = np.max(np.abs(nlp.cons(xs)))
    dual = np.max(np.abs(nlp.grad(xs) + nlp.jtprod(xs, lam)))
    print(f"\npendulum with energy terms N=200, trunk: {st.status} in {st.iter} outer iterations, |c| {primal:.2e}, "
          f"|grad f + J'lambda| {dual:.2e}, {st.solver_specific}, factorizations {dev.info()['factorizations']}")
    assert st.status == "first_order"
    assert primal <= 1e-8 and dual <= 1e-5
    # the outer loop reports the user's f, terms included (torch's cos / exp on the device against numpy's: a few ulp a term)
    assert abs(st.objective - nlp.obj(xs)) <= 1e-10 * max(abs(nlp.obj(xs)), 1.0)
    assert dev.info()["regularized_pivots"] == 0
    dev.close()
    base = DeviceBandSepFuncNLP(problems.pendulum_like(200))
    st0, xs0, _ = _solve(base)
    base.close()
    moved = np.max(np.abs(xs - xs0))
    print(f"the solution without the terms lies {moved:.2f} away (max norm)")
    assert st0.status == "first_order" and moved > 0.1
