"""Coupling terms on bordered and arrow band handles (fpsq_band_nlp_create_coupled_arrow, DeviceArrowBandCoupledQuadNLP): the
device-resident model of tests/test_gpu_band_coupled_nlp.py on the handles of tests/test_gpu_band_arrow_nlp.py.

Yardstick: the CPU restatement tests/coupled_quad_ref.py (pattern-agnostic: exact KKT solves at J(x), the gradient in the -ys
form, the mirror's hprod_), at the project's bars: max|a - b| / max|b| < 1e-9 per vector, |fx - fx_ref| <= 1e-9 |fx_ref|, 1e-13
for J v / J'u; gx, gs, Hv1, Hv2 at the LONG COLUMNS and ys at the BORDER ROWS are each held to 1e-9 of their own magnitude, as in
tests/test_gpu_band_arrow_nlp.py -- the long rows of S end in exactly those entries.  Dropping the terms that touch a long column
or a border row moves the reference gx and Hv by more than 1e-3 on every case (tests/test_band_coupled_arrow_nlp_cpu.py).

Shapes: tests/coupled_arrow_cases.py.  The new kernel (k_bq_long_rows, four modes) runs one workgroup per long column, threads
striding the column's row of S: 574 entries are three trips, 1183 enter the four-entries-per-trip loop once, 160 leave threads
without an entry; its grid has no cap (<= 16 workgroups).  FPSQ_BAND_NLP_LONG_ROWS=0 (read at create) leaves those rows to the
lane-group kernels: the independent form, held to the same bars and to 1e-12 against the split one.

WITH_LANE_GROUP sites: none are new."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import fps_amd  # noqa: E402,F401
import coupled_arrow_cases as ca  # noqa: E402
import coupled_cases as cc  # noqa: E402
from fps_amd import _lib, nlpmodels, problems  # noqa: E402
from fps_amd.device_qp import (DeviceArrowBandCoupledQuadNLP, DeviceArrowBandEqQP, DeviceArrowBandSepQuadNLP,  # noqa: E402
                               DeviceBandCoupledQuadNLP, DeviceBandSepQuadNLP)
from fps_amd.qdsolver import FpsqError  # noqa: E402
from test_gpu_band_nlp import _objgrad  # noqa: E402

pytestmark = pytest.mark.gpu

SE, SIGMA = ca.SE, ca.SIGMA
BAR, BAR_PRODUCT, BAR_FORMS = 1e-9, 1e-13, 1e-12
ERR_STATE = -3
CASE_643 = "m640-r3-c5-param"
OUTS = ("gx", "ys", "gs", "c", "Hv2", "Hv1")


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def _device(name, **kw):
    data, rows, cols = ca.problem(name)
    border, ncols = ca.limits(name)
    dev = DeviceArrowBandCoupledQuadNLP(data, border=border, cols=ncols, sigma=SIGMA, rho=0.0, delta=ca.delta(name), eta=0.0, **kw)
    info = dev.info()
    for k, want in ca.want_info(name).items():
        assert info[k] == want, (k, info)
    assert (info["border_rows"], info["border_cols"]) == (rows.size, cols.size)
    return dev


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
    assert dev.hprod(ca.v_of(qp), Hv2, 2) == 0 and dev.hprod(ca.v_of(qp), Hv1, 1) == 0
    return {"fx": fx, "gx": gx, "ys": ys, "gs": gs, "c": c, "Hv2": Hv2, "Hv1": Hv1}


def _errors(got, e, rows, cols):
    errs = {k: _rel(got[k], e[k]) for k in OUTS}
    errs["fx"] = abs(got["fx"] - e["fx"]) / abs(e["fx"])
    if cols.size:
        errs.update({f"{k}[L]": _rel(got[k][cols], e[k][cols]) for k in ("gx", "gs", "Hv2", "Hv1")})
    if rows.size:
        errs["ys[border]"] = _rel(got["ys"][rows], e["ys"][rows])
    return errs


def _check(dev, name, label):
    _, rows, cols = ca.problem(name)
    out = []
    for rho, eta in ca.RHO_ETA:
        got = _evaluate(dev, rho, eta)
        errs = _errors(got, ca.expected(name)[(rho, eta)], rows, cols)
        split = _rel(got["Hv1"], got["Hv2"])
        print(f"\n{label} rho={rho} eta={eta}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()) + f" Hv1-Hv2={split:.2e}")
        assert max(errs.values()) < BAR, errs
        assert split > 1e-6
        out.append(got)
    return out


def _jac_mul(dev, name):
    data, rows, cols = ca.problem(name)
    qp = data.qp
    J = nlpmodels.CoupledQuadConModel(data)._J(qp.x)
    v, u = ca.v_of(qp), np.random.default_rng(2).standard_normal(qp.m)
    y, z = np.full(qp.m, np.nan), np.full(qp.n, np.nan)
    assert dev.jac_mul(0, 1.0, v, 0.0, y) == 0 and dev.jac_mul(1, 1.0, u, 0.0, z) == 0
    Jv, Jtu = J @ v, J.T @ u
    errs = [_rel(y, Jv), _rel(z, Jtu)]
    if rows.size:
        errs.append(_rel(y[rows], Jv[rows]))
    if cols.size:
        errs.append(_rel(z[cols], Jtu[cols]))
    print(f"{name}: jac_mul {max(errs):.2e}")
    assert max(errs) < BAR_PRODUCT


@pytest.mark.parametrize("name", ca.NAMES)
def test_every_entry_matches_the_exact_restatement_in_both_forms(name, monkeypatch):
    """the split form (one workgroup per long row of S) and, under FPSQ_BAND_NLP_LONG_ROWS=0, the form that leaves the long rows
    to the lane-group kernels: each at the bars, and the two within 1e-12 of each other"""
    dev = _device(name)
    split = _check(dev, name, name)
    info = dev.info()
    assert info["factorizations"] == len(ca.RHO_ETA) and info["regularized_pivots"] == 0
    _jac_mul(dev, name)                         # the handle's values are J(x), terms included
    dev.close()
    monkeypatch.setenv("FPSQ_BAND_NLP_LONG_ROWS", "0")
    dev = _device(name)
    whole = _check(dev, name, f"{name}, long rows inside S")
    dev.close()
    for a, b in zip(split, whole):
        assert abs(a["fx"] - b["fx"]) <= BAR_FORMS * abs(b["fx"])
        for k in OUTS:
            assert _rel(a[k], b[k]) < BAR_FORMS, k
    _, _, cols = ca.problem(name)
    if ca.COUNTS[name][1]:    # (the switch did switch: another summation order at the long columns)
        assert not all(np.array_equal(a[k][cols], b[k][cols]) for a, b in zip(split, whole) for k in ("gx", "Hv2", "Hv1"))


@pytest.mark.parametrize("form,name,env", [("nested", "m640-r16-c16-stride-first", ("FPSQ_ARROW_FUSED", "0")),
                                           ("by-row-pairs", CASE_643, ("FPSQ_BAND_FORM", "1"))])
def test_the_other_correction_and_formation_forms_meet_the_same_bars(form, name, env, monkeypatch):
    """FPSQ_ARROW_FUSED=0: the nested correction.  FPSQ_BAND_FORM=1 on a handle with long columns: k_band_form reads the OTHER
    columns' values, which the objgrad of the coupled model gathers too."""
    monkeypatch.setenv(*env)
    dev = _device(name)
    _check(dev, name, f"{name}, {form}")
    dev.close()


def _bits(dev, x=None):
    got = _evaluate(dev, 1.0, 0.5, x)
    return [np.float64(got["fx"])] + [got[k] for k in OUTS]


def _same(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a, b))


def _no_terms(data):
    z = np.zeros(0, np.int32)
    return problems.CoupledQuadNLP(data.qp, data.hvals, data.b, z, z, z, np.zeros(0))


def test_the_three_bit_for_bit_identities():
    kw = dict(sigma=SIGMA, rho=1.0, delta=SE, eta=0.5)
    # no terms: the arrow entry's model on that handle
    data, _, _ = ca.problem(CASE_643)
    outs = []
    for make in (lambda: DeviceArrowBandSepQuadNLP(cc.without_terms(data), **kw),
                 lambda: DeviceArrowBandCoupledQuadNLP(_no_terms(data), **kw)):
        dev = make()
        assert (dev.info()["border_rows"], dev.info()["border_cols"]) == (3, 5)
        outs.append(_bits(dev))
        dev.close()
    assert _same(*outs)
    # a plain handle: the coupled entry's model
    small = cc.data("small")
    outs = []
    for make in (lambda: DeviceBandCoupledQuadNLP(small, **kw), lambda: DeviceArrowBandCoupledQuadNLP(small, border=0, cols=0, **kw)):
        dev = make()
        assert (dev.info()["border_rows"], dev.info()["border_cols"]) == (0, 0)
        outs.append(_bits(dev))
        dev.close()
    assert _same(*outs)
    # a plain handle without terms: fpsq_band_nlp_create's model
    outs = []
    for make in (lambda: DeviceBandSepQuadNLP(cc.without_terms(small), **kw),
                 lambda: DeviceArrowBandCoupledQuadNLP(_no_terms(small), border=0, cols=0, **kw)):
        dev = make()
        outs.append(_bits(dev))
        dev.close()
    assert _same(*outs)


@pytest.mark.parametrize("name", [CASE_643, "m1500-r1-c1-shuffled"])
def test_linear_limit_agrees_with_the_linear_arrow_model(name):
    """h_vals = 0 and every w = 0 WITH THE TERMS PRESENT (every coupled launch, the long rows' included, runs on lists of
    zeros): the model is the eq-QP; objgrad / hprod agree with DeviceArrowBandEqQP within 1e-12, Val(1) equals Val(2) within that"""
    full, rows, cols = ca.problem(name)
    qp = full.qp
    data = dataclasses.replace(full, hvals=np.zeros_like(qp.vals), b=qp.b.copy(), t_w=np.zeros_like(full.t_w))
    assert data.nterms > 0
    delta = ca.delta(name)
    v = ca.v_of(qp)
    lin = DeviceArrowBandEqQP(qp, sigma=SIGMA, rho=1.0, delta=delta, eta=0.5)
    dev = DeviceArrowBandCoupledQuadNLP(data, sigma=SIGMA, rho=1.0, delta=delta, eta=0.5)
    assert (lin.info()["border_rows"], lin.info()["border_cols"]) == (dev.info()["border_rows"], dev.info()["border_cols"]) \
        == (rows.size, cols.size)
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


def test_repeatability_placement_state_rules_and_the_coo_refusal():
    import torch

    name = CASE_643
    data, _, _ = ca.problem(name)
    qp = data.qp
    x1, x2, xk = qp.x, qp.point(2), qp.xhat
    on = torch.device("cuda", 0)
    v = np.random.default_rng(1).standard_normal(qp.n)
    lib = _lib.load()

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

    dev = _device(name)
    dev.rho, dev.eta = 1.0, 0.5
    Hv = np.empty(qp.n)
    for ha in (2, 1):      # an hprod before any objgrad
        assert lib.fpsq_band_nlp_hprod(dev._h, dev._q, v.ctypes.data, SIGMA, 1.0, 0.5, ha, Hv.ctypes.data) == ERR_STATE
        assert b"objgrad" in lib.fpsq_band_last_error(dev._h)
    with pytest.raises(FpsqError):
        dev.hprod(v, Hv, 1)
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
    assert lib.fpsq_band_nlp_hprod(dev._h, dev._q, v.ctypes.data, SIGMA, 1.0, 0.5, 3, Hv.ctypes.data) == -1
    # a foreign factorisation: the model's point is gone until its next objgrad, which returns what it returned before
    assert lib.fpsq_band_factorize(dev._h, qp.vals.ctypes.data, SE, None) == 0
    for ha in (2, 1):
        assert lib.fpsq_band_nlp_hprod(dev._h, dev._q, v.ctypes.data, SIGMA, 1.0, 0.5, ha, Hv.ctypes.data) == ERR_STATE
        assert b"factorised again" in lib.fpsq_band_last_error(dev._h)
    back = _objgrad(dev, x1, xk)
    for a, b in zip(host, back):
        assert np.array_equal(a, b)
    for a, b in zip(hh, hprods(dev, False)):
        assert np.array_equal(a, b)
    # a second x: another J, other Wo values, and nothing of the first evaluation is left -- a fresh handle gives the same bits
    second = _objgrad(dev, x2, xk)
    h2 = hprods(dev, False)
    fresh_dev = _device(name)
    fresh_dev.rho, fresh_dev.eta = 1.0, 0.5
    fresh = _objgrad(fresh_dev, x2, xk)
    hf = hprods(fresh_dev, False)
    assert second[1] == 0 and fresh[1] == 0
    assert not np.array_equal(second[2], host[2])
    for a, b in zip(second, fresh):
        assert np.array_equal(a, b)
    for a, b in zip(h2, hf):
        assert np.array_equal(a, b)
    assert dev.info()["factorizations"] == 5 and fresh_dev.info()["factorizations"] == 1
    # a term off the pattern: the host checks and their message, under the new entry's name; the model made before stays whole
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
    row0 = qp.colind[qp.rowptr[0]:qp.rowptr[1]]
    off = int(np.setdiff1d(np.arange(qp.n), row0)[0])
    out = C.c_void_p()
    tr, tj, tk, tw = i32([0]), i32([off]), i32([int(row0[0])]), np.array([0.1])
    rc = lib.fpsq_band_nlp_create_coupled_arrow(dev._h, qp.qdiag.ctypes.data, qp.d.ctypes.data, data.b.ctypes.data,
                                                qp.vals.ctypes.data, data.hvals.ctypes.data, 1, tr.ctypes.data, tj.ctypes.data,
                                                tk.ctypes.data, tw.ctypes.data, C.byref(out))
    msg = lib.fpsq_band_last_error(dev._h)
    assert rc == -1 and b"band_nlp_create_coupled" in msg and b"not an entry" in msg
    assert _objgrad(dev, x2, xk)[1] == 0
    dev.close()
    fresh_dev.close()
    # a COO-created handle: refused by the new entry as by the existing ones
    coo = C.c_void_p()
    r = np.repeat(np.arange(qp.m, dtype=np.int64), np.diff(qp.rowptr))
    cidx = qp.colind.astype(np.int64)
    assert lib.fpsq_band_create_coo_arrow(C.byref(coo), qp.n, qp.m, qp.nnz, r.ctypes.data, cidx.ctypes.data, 0, 16, 16, 0) == 0
    z = np.zeros_like(qp.vals)
    rc = lib.fpsq_band_nlp_create_coupled_arrow(coo, qp.qdiag.ctypes.data, qp.d.ctypes.data, data.b.ctypes.data,
                                                qp.vals.ctypes.data, z.ctypes.data, 0, None, None, None, None, C.byref(out))
    msg = lib.fpsq_band_last_error(coo)
    assert rc == ERR_STATE and b"band_nlp_create" in msg and b"fpsq_band_create_coo" in msg
    assert lib.fpsq_band_destroy(coo) == 0
    # the plain coupled entry keeps refusing border rows and long columns
    arrow = _device(name)
    rc = lib.fpsq_band_nlp_create_coupled(arrow._h, qp.qdiag.ctypes.data, qp.d.ctypes.data, data.b.ctypes.data,
                                          qp.vals.ctypes.data, z.ctypes.data, 0, None, None, None, None, C.byref(out))
    assert rc == ERR_STATE and b"border rows" in lib.fpsq_band_last_error(arrow._h)
    arrow.close()


@pytest.mark.parametrize("sub", ["lbfgs", "trunk"])
def test_fps_solve_device_on_the_free_final_time_model(sub):
    """fps_solve_device on free_final_time_like(2000) from x0 = xhat + 0.1 (x - xhat): the returned point checked INDEPENDENTLY
    with the host model and the solver's own score rule, as tests/test_gpu_band_coupled_nlp.py does: primal
    |c(x*)|inf / max(|x*|, 1), dual |grad f + J'lambda|inf / max(|lambda|, 1), both <= 10 tol, tol = max(atol, rtol max(p0, d0)),
    atol = rtol = sqrt(eps)."""
    import torch

    from fps_amd.fps_solve import fps_solve_device

    data, _, _ = ca.problem(ca.FFT)
    qp = data.qp
    nlp = nlpmodels.CoupledQuadConModel(data)
    x0 = qp.xhat + 0.1 * (qp.x - qp.xhat)
    dev = DeviceArrowBandCoupledQuadNLP(data)
    assert (dev.info()["border_rows"], dev.info()["border_cols"], dev.info()["bandwidth_blocks"]) == (1, 1, 1)
    st = fps_solve_device(dev, torch.from_numpy(x0.copy()).to(torch.device("cuda", 0)), max_iter=30, subproblem_solver=sub)
    xs, lam = st.solution.cpu().numpy(), st.multipliers.cpu().numpy()
    p0 = np.abs(nlp.cons(x0)).max() / max(np.linalg.norm(x0), 1.0)
    d0 = np.abs(nlp.grad(x0)).max()
    tol = max(SE, SE * max(p0, d0))
    primal = np.abs(nlp.cons(xs)).max() / max(np.linalg.norm(xs), 1.0)
    dual = np.abs(nlp.grad(xs) + nlp.jtprod(xs, lam)).max() / max(np.linalg.norm(lam), 1.0)
    info = dev.info()
    print(f"\nfps_solve_device free-final-time/{sub}: {st.status} in {st.iter} outer iterations, primal {primal:.2e} dual "
          f"{dual:.2e} tol {tol:.2e}, {st.solver_specific}, factorizations {info['factorizations']}")
    assert st.status == "first_order"
    assert primal <= 10 * tol and dual <= 10 * tol
    assert info["factorizations"] == st.solver_specific["objgrad_calls"]
    dev.close()
