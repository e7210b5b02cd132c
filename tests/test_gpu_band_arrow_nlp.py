"""Nonlinear equality constraints on bordered and arrow band handles (fpsq_band_nlp_create_arrow, DeviceArrowBandSepQuadNLP):
the device-resident model of tests/test_gpu_band_nlp.py on the handles of tests/test_gpu_band_arrow.py.

Yardstick: the CPU restatement tests/sepquad_ref.py (pattern-agnostic: exact KKT solves at J(x), the gradient in the -ys form,
the mirror's hprod_) on problems.with_quadratic_constraints(<arrow problem>, curv=0.3, seed=7), at the project's bars:
max|a - b| / max|b| < 1e-9 per vector, |fx - fx_ref| <= 1e-9 |fx_ref|, 1e-13 for J v / J'u.  In addition gx, gs, Hv1, Hv2 at
the LONG COLUMNS and ys at the BORDER ROWS are each held to 1e-9 of their own magnitude: the curvature sums of those <= 16
entries are formed by kernels of their own (k_bn_lc_epilogue, k_bn_lc_epilogue_h1) and a defect there would hide under the
max-norm of an n-vector (left out, they are 1.3e-3 of max|gx| on the 643-row case: tests/test_band_arrow_nlp_cpu.py).

Shapes: those of tests/test_gpu_band_arrow.py, the smallest that reach each branch, and the two one-kind handles through the
new entry.  The new kernels run one workgroup per long column, threads striding the column's entries: 643 entries are three
trips; their grid has no cap (<= 16 workgroups).

WITH_LANE_GROUP sites: none are new.  k_bn_lc_epilogue and k_bn_lc_epilogue_h1 are not lane-group kernels; the sites of
fpsq_band_nlp.hip.h listed in tests/lane_group_cases.py are launched unchanged, with lgT chosen from the entries of the
transposed structure (t_nnz = nnz on a handle without long columns)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import fps_amd  # noqa: E402,F401
from fps_amd import _lib, nlpmodels, problems  # noqa: E402
from fps_amd.device_qp import (DeviceArrowBandEqQP, DeviceArrowBandSepQuadNLP, DeviceBandSepQuadNLP)  # noqa: E402
from fps_amd.qdsolver import FpsqError  # noqa: E402
from sepquad_ref import SepQuadRef  # noqa: E402
from test_gpu_band_arrow import _exactly_singular, _p640, _p1500, _placed  # noqa: E402
from test_gpu_band_nlp import _objgrad, _small  # noqa: E402

pytestmark = pytest.mark.gpu

SE = float(np.sqrt(np.finfo(float).eps))
SIGMA, CURV = 1e3, 0.3
BAR, BAR_PRODUCT = 1e-9, 1e-13
ERR_STATE = -3
PAIRS = ((0.0, 0.0), (1.0, 0.5))   # (rho, eta)
NONE = np.zeros(0, dtype=np.int64)


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def _arrow(make, s_r, s_c, kind, where, shuffle):
    return lambda: _placed(make(), s_r, s_c, kind, where, shuffle)


# name: (-> (qp, border rows, long columns), delta, (border, cols) of the class, expected info of the handle)
CASES = {
    # (640 band rows fill 5 blocks exactly: the border opens a block of padding; one workgroup of the columns' reductions
    # per 256 rows: vgrid = 3)
    "m640-r3-c5-param": (_arrow(_p640, 3, 5, "param", "last", False), 0.0, (16, 16),
                         {"border_rows": 3, "border_cols": 5, "nblocks": 5, "chains": 1, "reordered": 0}),
    "m640-r16-c16-stride-first": (_arrow(_p640, 16, 16, "stride", "first", False), SE, (16, 16),
                                  {"border_rows": 16, "border_cols": 16, "nblocks": 5, "chains": 1}),
    # (rperm / vperm / t_perm are live; the border row lies in the padding of the last block)
    "m1500-r1-c1-shuffled": (_arrow(_p1500, 1, 1, "param", "last", True), SE, (16, 16),
                             {"border_rows": 1, "border_cols": 1, "nblocks": 12, "chains": 1, "reordered": 1}),
    "aug2dc-N51-r2-c16-param": (_arrow(lambda: problems.aug2dc_like(N=51), 2, 16, "param", "last", False), SE, (16, 16),
                                {"border_rows": 2, "border_cols": 16, "nblocks": 21, "chains": 2}),
    "rows-only": (lambda: (problems.with_border_rows(_p640(), 2), 640 + np.arange(2), NONE), SE, (16, 0),
                  {"border_rows": 2, "border_cols": 0, "nblocks": 5}),
    "cols-only": (lambda: (problems.with_long_columns(_p640(), 2), NONE, 3000 + np.arange(2)), SE, (0, 16),
                  {"border_rows": 0, "border_cols": 2, "nblocks": 5}),
}
CASE_643 = "m640-r3-c5-param"


@functools.lru_cache(maxsize=None)
def _problem(case):
    """(qp, data, border rows, long columns)"""
    qp, rows, cols = CASES[case][0]()
    return qp, problems.with_quadratic_constraints(qp, curv=CURV, seed=7), rows, cols


def _v(qp):
    return np.random.default_rng(0).standard_normal(qp.n)


@functools.lru_cache(maxsize=None)
def _expected(case):
    """what the restatement says at x = qp.x, xk = qp.xhat: one dict per (rho, eta), computed once and left unchanged"""
    qp, data, _, _ = _problem(case)
    ref = SepQuadRef(data, SIGMA, 0.0, CASES[case][1], 0.0, qp.xhat)
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


def _device(case, **kw):
    _, data, _, _ = _problem(case)
    border, cols = CASES[case][2]
    dev = DeviceArrowBandSepQuadNLP(data, border=border, cols=cols, sigma=SIGMA, rho=0.0, delta=CASES[case][1], eta=0.0, **kw)
    info = dev.info()
    for k, want in CASES[case][3].items():
        assert info[k] == want, (k, info)
    return dev


def _evaluate(dev, rho, eta):
    """cons, one objgrad with every output and both Hessian products at x = qp.x, xk = qp.xhat"""
    qp = dev.qp
    dev.rho, dev.eta = rho, eta
    c = np.full(qp.m, np.nan)
    assert dev.cons(qp.x, c) == 0
    fx, rc, gx, ys, gs = _objgrad(dev, qp.x, qp.xhat)
    assert rc == 0
    Hv2, Hv1 = np.full(qp.n, np.nan), np.full(qp.n, np.nan)
    assert dev.hprod(_v(qp), Hv2, 2) == 0 and dev.hprod(_v(qp), Hv1, 1) == 0
    return {"fx": fx, "gx": gx, "ys": ys, "gs": gs, "c": c, "Hv2": Hv2, "Hv1": Hv1}


def _errors(got, e, rows, cols):
    """the figures a case is held to: every vector in the max-norm, the long columns' and the border rows' entries on their own"""
    errs = {k: _rel(got[k], e[k]) for k in ("gx", "ys", "gs", "c", "Hv2", "Hv1")}
    errs["fx"] = abs(got["fx"] - e["fx"]) / abs(e["fx"])
    if cols.size:
        errs.update({f"{k}[L]": _rel(got[k][cols], e[k][cols]) for k in ("gx", "gs", "Hv2", "Hv1")})
    if rows.size:
        errs["ys[border]"] = _rel(got["ys"][rows], e["ys"][rows])
    return errs


def _check(dev, case, label):
    qp, _, rows, cols = _problem(case)
    out = []
    for rho, eta in PAIRS:
        got = _evaluate(dev, rho, eta)
        errs = _errors(got, _expected(case)[(rho, eta)], rows, cols)
        split = _rel(got["Hv1"], got["Hv2"])
        print(f"\n{label} rho={rho} eta={eta}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()) + f" Hv1-Hv2={split:.2e}")
        assert max(errs.values()) < BAR, errs
        assert split > 1e-6                    # the terms that vanish on the linear model are live here
        out.append(got)
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_every_entry_matches_the_exact_restatement(case):
    qp, data, rows, cols = _problem(case)
    dev = _device(case)
    _check(dev, case, case)
    info = dev.info()
    assert info["factorizations"] == len(PAIRS)   # one per objgrad, none for hprod / cons
    assert info["regularized_pivots"] == 0
    # the handle's values are J(x): fpsq_band_jac_mul multiplies with it, the long columns' and the border rows' entries too
    J = nlpmodels.SepQuadConModel(data)._J(qp.x)
    v, u = _v(qp), np.random.default_rng(2).standard_normal(qp.m)
    y, z = np.full(qp.m, np.nan), np.full(qp.n, np.nan)
    assert dev.jac_mul(0, 1.0, v, 0.0, y) == 0 and dev.jac_mul(1, 1.0, u, 0.0, z) == 0
    Jv, Jtu = J @ v, J.T @ u
    errs = [_rel(y, Jv), _rel(z, Jtu)]
    if rows.size:
        errs.append(_rel(y[rows], Jv[rows]))
    if cols.size:
        errs.append(_rel(z[cols], Jtu[cols]))
    print(f"{case}: jac_mul {max(errs):.2e}")
    assert max(errs) < BAR_PRODUCT
    dev.close()


@pytest.mark.parametrize("form,case,env", [("nested", "m640-r16-c16-stride-first", ("FPSQ_ARROW_FUSED", "0")),
                                           ("by-row-pairs", CASE_643, ("FPSQ_BAND_FORM", "1"))])
def test_the_other_correction_and_formation_forms_meet_the_same_bars(form, case, env, monkeypatch):
    """FPSQ_ARROW_FUSED=0: the nested correction behind the same band_solve.  FPSQ_BAND_FORM=1 on a handle with long columns:
    k_band_form reads the OTHER columns' values, which the objgrad gathers itself.  Both are read at create."""
    dev = _device(case)
    default = _evaluate(dev, 1.0, 0.5)
    dev.close()
    monkeypatch.setenv(*env)
    dev = _device(case)
    other = _check(dev, case, f"{case}, {form}")[1]
    dev.close()
    if form == "nested":   # (the switch did switch: another summation order)
        assert not all(np.array_equal(default[k], other[k]) for k in ("gx", "ys", "gs", "Hv2", "Hv1"))


class _PlainHandleThroughTheNewEntry(DeviceBandSepQuadNLP):
    _model_entry = "fpsq_band_nlp_create_arrow"


def test_a_plain_handle_through_the_new_entry_gives_the_bits_of_the_existing_entry():
    qp = _small()
    data = problems.with_quadratic_constraints(qp, curv=CURV, seed=7)
    outs = []
    for make in (lambda **kw: DeviceBandSepQuadNLP(data, **kw), lambda **kw: _PlainHandleThroughTheNewEntry(data, **kw),
                 lambda **kw: DeviceArrowBandSepQuadNLP(data, border=0, cols=0, **kw)):
        dev = make(sigma=SIGMA, rho=1.0, delta=SE, eta=0.5)
        assert dev.info()["border_rows"] == 0 and dev.info()["border_cols"] == 0
        got = _evaluate(dev, 1.0, 0.5)
        outs.append([np.float64(got["fx"])] + [got[k] for k in ("gx", "ys", "gs", "c", "Hv2", "Hv1")])
        dev.close()
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("case", [CASE_643, "m1500-r1-c1-shuffled"])
def test_linear_limit_agrees_with_the_linear_arrow_model(case):
    """h_vals = 0: the model IS the eq-QP; objgrad / hprod agree with DeviceArrowBandEqQP within 1e-12 relative (the figure of
    the linear-limit test of tests/test_gpu_band_nlp.py), Val(1) equals Val(2) within that"""
    qp = _problem(case)[0]
    data = problems.SepQuadNLP(qp, np.zeros_like(qp.vals), qp.b.copy())
    delta = CASES[case][1]
    v = _v(qp)
    lin = DeviceArrowBandEqQP(qp, sigma=SIGMA, rho=1.0, delta=delta, eta=0.5)
    dev = DeviceArrowBandSepQuadNLP(data, sigma=SIGMA, rho=1.0, delta=delta, eta=0.5)
    for k in ("border_rows", "border_cols"):
        assert lin.info()[k] == dev.info()[k] == CASES[case][3][k]
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


def test_repeatability_placement_and_state_rules():
    import torch

    case = CASE_643
    qp, data, _, _ = _problem(case)
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

    dev = _device(case)
    dev.rho, dev.eta = 1.0, 0.5
    # an hprod before any objgrad
    Hv = np.empty(qp.n)
    assert lib.fpsq_band_nlp_hprod(dev._h, dev._q, v.ctypes.data, SIGMA, 1.0, 0.5, 2, Hv.ctypes.data) == ERR_STATE
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
    # a second x: another J, and nothing of the first evaluation is left -- a fresh handle gives the same bits
    second = _objgrad(dev, x2, xk)
    h2 = hprods(dev, False)
    fresh_dev = _device(case)
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
    dev.close()
    fresh_dev.close()
    # a COO-created handle: refused by the new entry as by the existing one
    coo, out = C.c_void_p(), C.c_void_p()
    r = np.repeat(np.arange(qp.m, dtype=np.int64), np.diff(qp.rowptr))
    cidx = qp.colind.astype(np.int64)
    assert lib.fpsq_band_create_coo_arrow(C.byref(coo), qp.n, qp.m, qp.nnz, r.ctypes.data, cidx.ctypes.data, 0, 16, 16, 0) == 0
    z = np.zeros_like(qp.vals)
    rc = lib.fpsq_band_nlp_create_arrow(coo, qp.qdiag.ctypes.data, qp.d.ctypes.data, data.b.ctypes.data, qp.vals.ctypes.data,
                                        z.ctypes.data, C.byref(out))
    msg = lib.fpsq_band_last_error(coo)
    assert rc == ERR_STATE and b"band_nlp_create" in msg and b"fpsq_band_create_coo" in msg
    assert lib.fpsq_band_destroy(coo) == 0


def _singular():
    qp, at = _exactly_singular()
    return problems.SepQuadNLP(qp, np.zeros_like(qp.vals), qp.b.copy()), at


def test_singular_border_without_regularisation_reports_the_border_row():
    """the construction of tests/test_gpu_band_arrow.py with h_vals = 0: S_r is an EXACT zero at every x"""
    lib = _lib.load()
    data, at = _singular()
    qp = data.qp
    rp, ci = np.ascontiguousarray(qp.rowptr, dtype=np.int32), np.ascontiguousarray(qp.colind, dtype=np.int32)
    h, q = C.c_void_p(), C.c_void_p()
    assert lib.fpsq_band_create_arrow(C.byref(h), qp.n, qp.m, rp.ctypes.data, ci.ctypes.data, 1, 1, 0) == 0
    assert lib.fpsq_band_nlp_create_arrow(h, qp.qdiag.ctypes.data, qp.d.ctypes.data, data.b.ctypes.data, qp.vals.ctypes.data,
                                          data.hvals.ctypes.data, C.byref(q)) == 0
    fx, pivot = C.c_double(), C.c_int32(-7)
    gx = np.full(qp.n, np.nan)

    def objgrad(delta):
        return lib.fpsq_band_nlp_objgrad(h, q, qp.x.ctypes.data, SIGMA, 1.0, 0.0, delta, None, C.byref(fx), gx.ctypes.data, None,
                                         None, C.byref(pivot))

    assert (objgrad(0.0), pivot.value) == (1, at + 1)          # soft code, the row 1-based in the caller's order
    assert np.all(np.isnan(gx))                                # nothing was evaluated
    Hv = np.empty(qp.n)
    assert lib.fpsq_band_nlp_hprod(h, q, qp.x.ctypes.data, SIGMA, 1.0, 0.0, 2, Hv.ctypes.data) == ERR_STATE
    assert (objgrad(1e-3), pivot.value) == (0, 0)              # delta > 0: positive definite again
    assert np.all(np.isfinite(gx))
    assert lib.fpsq_band_nlp_destroy(q) == 0 and lib.fpsq_band_destroy(h) == 0
    # through the class, regularisation switched off: fx is nan
    dev = DeviceArrowBandSepQuadNLP(data, border=1, cols=1, sigma=SIGMA, rho=1.0, delta=0.0)
    assert lib.fpsq_band_set_regularization(dev._h, 0.0, 0.0) == 0
    with pytest.warns(UserWarning):
        fx_c, rc = dev.objgrad(qp.x, gx=np.empty(qp.n))
    assert rc == 1 and np.isnan(fx_c)
    dev.close()


def test_singular_border_with_the_default_regularisation_is_regularised():
    data, _ = _singular()
    qp = data.qp
    dev = DeviceArrowBandSepQuadNLP(data, border=1, cols=1, sigma=SIGMA, rho=1.0, delta=0.0)
    fx, rc, gx, ys, gs = _objgrad(dev, qp.x, None)
    i = dev.info()
    assert rc == 0 and (i["border_rows"], i["border_cols"]) == (1, 1) and i["regularized_pivots"] >= 1
    assert np.isfinite(fx) and all(np.all(np.isfinite(a)) for a in (gx, ys, gs))
    for ha in (2, 1):
        Hv = np.full(qp.n, np.nan)
        assert dev.hprod(qp.x, Hv, ha) == 0 and np.all(np.isfinite(Hv))
    dev.close()


@pytest.mark.parametrize("sub", ["lbfgs", "trunk"])
def test_fps_solve_device_end_to_end_agrees_with_the_wide_band(sub):
    """fps_solve_device on the 643-row case from x0 = xhat + 0.1 (x - xhat): the independent residuals of the end-to-end test
    of tests/test_gpu_band_nlp.py (primal and dual <= 10 tol), and the same status, outer-iteration count and solution (1e-6)
    as DeviceBandSepQuadNLP on the same problem as a wide band."""
    import torch

    from fps_amd.fps_solve import fps_solve_device

    qp, data, _, _ = _problem(CASE_643)
    nlp = nlpmodels.SepQuadConModel(data)
    x0 = qp.xhat + 0.1 * (qp.x - qp.xhat)
    p0 = np.abs(nlp.cons(x0)).max() / max(np.linalg.norm(x0), 1.0)
    d0 = np.abs(nlp.grad(x0)).max()
    tol = max(SE, SE * max(p0, d0))
    res = {}
    for name, cls in (("arrow", DeviceArrowBandSepQuadNLP), ("wide", DeviceBandSepQuadNLP)):
        dev = cls(data)
        i = dev.info()
        assert (i["border_rows"], i["border_cols"]) == ((3, 5) if name == "arrow" else (0, 0))
        st = fps_solve_device(dev, torch.from_numpy(x0).to(torch.device("cuda", 0)), max_iter=30, subproblem_solver=sub)
        xs, lam = st.solution.cpu().numpy(), st.multipliers.cpu().numpy()
        primal = np.abs(nlp.cons(xs)).max() / max(np.linalg.norm(xs), 1.0)
        dual = np.abs(nlp.grad(xs) + nlp.jtprod(xs, lam)).max() / max(np.linalg.norm(lam), 1.0)
        print(f"\n{name} {sub}: {st.status} in {st.iter} outer iterations, primal {primal:.2e} dual {dual:.2e} tol {tol:.2e}, "
              f"{st.solver_specific}, factorizations {dev.info()['factorizations']}")
        assert st.status == "first_order"
        assert primal <= 10 * tol and dual <= 10 * tol
        assert dev.info()["factorizations"] == st.solver_specific["objgrad_calls"]
        res[name] = (st.status, st.iter, xs)
        dev.close()
    assert res["arrow"][:2] == res["wide"][:2]
    assert np.linalg.norm(res["arrow"][2] - res["wide"][2]) <= 1e-6 * np.linalg.norm(res["wide"][2])
