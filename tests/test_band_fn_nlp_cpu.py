"""Elementwise function terms on the banded nonlinear model (fpsq_band_nlp_create_fn), the part that needs no GPU: the function
table, the host model nlpmodels.SepFuncConModel, the restatement tests/sepfunc_ref.py the GPU tests are held to, the inputs of
those tests, the generators, and a host solve of the pendulum."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import fps_amd  # noqa: E402,F401
import lane_group_cases as lg  # noqa: E402
from fps_amd import nlpmodels, problems  # noqa: E402
from sepfunc_ref import CURV, SepFuncRef, fn_codes, fn_data, fn_data_of  # noqa: E402
from sepquad_ref import _SparseExtrasOracle  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SE = float(np.sqrt(np.finfo(float).eps))
SIGMA = 1e3
NCODES = 6


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def _shape():
    """the 120 x 40 shape the gradient was first measured on"""
    qp = problems.pde_control_like(n=120, m=40, per_row=8, window=64, seed=3)
    return qp, problems.with_function_constraints(qp, curv=0.3, seed=7, codes=fn_codes(qp.vals.size))


def test_the_code_values_are_pinned_in_the_header_and_in_python():
    want = {"HALFSQ": 0, "CUBE6": 1, "SIN": 2, "COS": 3, "EXP": 4, "TANH": 5, "COUNT": 6}
    text = open(os.path.join(ROOT, "include", "fpsq.h")).read()
    got = {k: int(v) for k, v in re.findall(r"FPSQ_FN_([A-Z0-9]+) = (\d+)", text)}
    assert got == want
    assert (problems.FN_HALFSQ, problems.FN_CUBE6, problems.FN_SIN, problems.FN_COS, problems.FN_EXP, problems.FN_TANH) == \
        (0, 1, 2, 3, 4, 5)
    assert len(problems.FN_TABLE) == NCODES
    x = np.array([0.7])
    t = np.tanh(0.7)
    literal = [(0.245, 0.7, 1.0), (0.343 / 6, 0.245, 0.7), (np.sin(0.7), np.cos(0.7), -np.sin(0.7)),
               (np.cos(0.7), -np.sin(0.7), -np.cos(0.7)), (np.exp(0.7),) * 3, (t, 1 - t * t, -2 * t * (1 - t * t))]
    for code, vals in enumerate(literal):
        for order, want_v in enumerate(vals):
            got_v = problems.fn_apply(np.array([code], dtype=np.uint8), x, order)[0]
            assert abs(got_v - want_v) <= 4e-16 * max(abs(want_v), 1.0), (code, order)


@pytest.mark.parametrize("code", range(NCODES))
def test_the_table_is_consistent_with_its_own_derivatives(code):
    """phi' and phi'' against central differences of phi and phi' on [-1.1, 1.1]: step 1e-5, truncation h^2/6 |phi'''| <= 5e-11
    and rounding eps/h ~ 2e-11 on values of size <= 3, so 1e-9 absolute is a bar with room"""
    x = np.linspace(-1.1, 1.1, 45)
    codes = np.full(x.size, code, dtype=np.uint8)
    h = 1e-5
    for order in (0, 1):
        fd = (problems.fn_apply(codes, x + h, order) - problems.fn_apply(codes, x - h, order)) / (2 * h)
        assert np.max(np.abs(fd - problems.fn_apply(codes, x, order + 1))) <= 1e-9


def test_host_model_derivatives():
    qp, data = _shape()
    nlp = nlpmodels.SepFuncConModel(data)
    rng = np.random.default_rng(4)
    x, y, v, g = qp.x, rng.standard_normal(qp.m), rng.standard_normal(qp.n), rng.standard_normal(qp.n)
    assert set(np.unique(data.codes)) == set(range(NCODES))
    # jac_coord against a central difference of cons, column by column
    h = 1e-6
    J = nlp._J(x).toarray()
    for j in range(qp.n):
        e = np.zeros(qp.n)
        e[j] = h
        assert np.max(np.abs((nlp.cons(x + e) - nlp.cons(x - e)) / (2 * h) - J[:, j])) <= 1e-8
    assert _rel(nlp.jprod(x, v), J @ v) <= 1e-14 and _rel(nlp.jtprod(x, y), J.T @ y) <= 1e-14
    # hprod(x, y, v, 0) = d/dt J(x + t v)'y
    fd = (nlp.jtprod(x + h * v, y) - nlp.jtprod(x - h * v, y)) / (2 * h)
    assert _rel(nlp.hprod(x, y, v, 0.0), fd) <= 1e-8
    assert _rel(nlp.hprod(x, y, v, 1.0) - nlp.hprod(x, y, v, 0.0), qp.qdiag * v) <= 1e-14
    # ghjvprod by its definition: (g' Hess c_i v)_i, Hess c_i = diag(row i of G)
    G = np.zeros((qp.m, qp.n))
    rows = np.repeat(np.arange(qp.m), np.diff(qp.rowptr))
    G[rows, qp.colind] = data.hvals * problems.fn_apply(data.codes, x[qp.colind], 2)
    want = np.array([g @ (G[i] * v) for i in range(qp.m)])
    assert _rel(nlp.ghjvprod(x, g, v), want) <= 1e-14


def test_all_codes_zero_is_the_separable_quadratic_model():
    qp, data = _shape()
    zero = problems.with_function_constraints(qp, curv=0.3, seed=7, codes=np.zeros(qp.vals.size, dtype=np.uint8))
    quad = problems.with_quadratic_constraints(qp, curv=0.3, seed=7)
    assert np.array_equal(zero.hvals, quad.hvals) and _rel(zero.b, quad.b) <= 1e-14
    a, b = nlpmodels.SepFuncConModel(zero), nlpmodels.SepQuadConModel(quad)
    rng = np.random.default_rng(4)
    x, y, v, g = qp.x, rng.standard_normal(qp.m), rng.standard_normal(qp.n), rng.standard_normal(qp.n)
    # (c is a difference of O(1) sums: measured against the size of those, which is that of b)
    assert np.max(np.abs(a.cons(x) - b.cons(x))) <= 1e-14 * np.max(np.abs(quad.b))
    assert _rel(a.jac_coord(x), b.jac_coord(x)) <= 1e-14
    assert _rel(a.hprod(x, y, v), b.hprod(x, y, v)) <= 1e-14
    assert _rel(a.ghjvprod(x, g, v), b.ghjvprod(x, g, v)) <= 1e-14


def test_the_restatement_gradient_is_the_gradient_of_its_obj():
    qp, data = _shape()
    ref = SepFuncRef(data, SIGMA, 1.0, SE, 0.5, qp.xhat)
    x = qp.x
    gx = ref.objgrad(x)["gx"]
    lit = ref.grad_literal(x)
    rng = np.random.default_rng(5)
    h = 1e-6
    for _ in range(3):
        u = rng.standard_normal(qp.n)
        u /= np.linalg.norm(u)
        fd = (ref.obj(x + h * u) - ref.obj(x - h * u)) / (2 * h)
        err = abs(gx @ u - fd) / abs(fd)
        print(f"\n-ys form: {err:.2e}   literal +ys: {abs(lit @ u - fd) / abs(fd):.2e}")
        assert err <= 1e-7


@pytest.mark.parametrize("name", lg.NAMES)
def test_the_bar_tells_the_function_model_from_the_separable_one(name):
    """the same data with every code forced to 0 (same b): gx and c of the restatement move by far more than the GPU bar"""
    qp = lg.qp(name)
    data = fn_data(name)
    plain = problems.SepFuncNLP(qp, data.hvals, data.b, np.zeros_like(data.codes))
    a = SepFuncRef(data, SIGMA, 0.0, SE, 0.0, qp.xhat, kept=True).objgrad(qp.x)   # (kept: one LU of K per model)
    b = SepFuncRef(plain, SIGMA, 0.0, SE, 0.0, qp.xhat, kept=True).objgrad(qp.x)
    d_gx, d_c = _rel(b["gx"], a["gx"]), _rel(b["c"], a["c"])
    print(f"\n{name}: gx moves {d_gx:.2e}, c moves {d_c:.2e}")
    assert d_gx > 1e-3 and d_c > 1e-3


def _sigma_ratio(qp, data):
    J = nlpmodels.SepFuncConModel(data)._J(qp.x).toarray()
    sJ = np.linalg.svd(J, compute_uv=False)
    sA = np.linalg.svd(qp.scipy_csr().toarray(), compute_uv=False)
    return sJ[-1] / sA[-1], sJ[0] / sJ[-1]


@pytest.mark.parametrize("name", [n for n in lg.NAMES if n != "stride"])
def test_the_lane_group_inputs_are_well_posed(name):
    ratio, cond = _sigma_ratio(lg.qp(name), fn_data(name))
    print(f"\n{name}: sigma_min(J(x)) / sigma_min(A) = {ratio:.2f}, cond(J) = {cond:.1f}")
    assert ratio >= 0.5


ARROW_CASES = ("m640-r3-c5-param", "m640-r16-c16-stride-first", "m1500-r1-c1-shuffled", "aug2dc-N51-r2-c16-param", "rows-only",
               "cols-only")


@pytest.mark.parametrize("case", ARROW_CASES)
def test_the_arrow_inputs_are_well_posed(case):
    import test_gpu_band_arrow_nlp as arrow

    assert tuple(arrow.CASES) == ARROW_CASES
    qp, rows, cols = arrow.CASES[case][0]()
    data = fn_data_of(qp)
    ratio, cond = _sigma_ratio(qp, data)
    print(f"\n{case}: sigma_min(J(x)) / sigma_min(A) = {ratio:.2f}, cond(J) = {cond:.1f}")
    assert ratio >= 0.5
    # codes other than 0 on entries of the long columns and of the border rows
    r = np.repeat(np.arange(qp.m), np.diff(qp.rowptr))
    if cols.size:
        assert np.any(data.codes[np.isin(qp.colind, cols)] != 0)
    if rows.size:
        assert np.any(data.codes[np.isin(r, rows)] != 0)


def test_generators():
    qp = problems.pde_control_like(n=120, m=40, per_row=8, window=64, seed=3)
    data = problems.with_function_constraints(qp, curv=CURV, seed=2)
    assert data.codes.dtype == np.uint8 and set(np.unique(data.codes)) == set(range(NCODES))
    assert np.array_equal(data.hvals, problems.with_quadratic_constraints(qp, CURV, 2).hvals)
    assert np.max(np.abs(nlpmodels.SepFuncConModel(data).cons(qp.xhat))) <= 1e-12
    given = problems.with_function_constraints(qp, curv=CURV, seed=2, codes=np.full(qp.vals.size, 4))
    assert given.codes.dtype == np.uint8 and np.all(given.codes == 4)

    pen = problems.pendulum_like(200)
    q = pen.qp
    assert (q.n, q.m) == (602, 400)
    rows = np.repeat(np.arange(q.m), np.diff(q.rowptr))
    sin = pen.codes == problems.FN_SIN
    assert np.all(pen.codes[~sin] == 0)
    assert np.array_equal(np.bincount(rows[sin], minlength=q.m), np.arange(q.m) % 2)   # one in every odd row, none elsewhere
    assert np.all(q.vals[sin] == 0.0) and np.all(pen.hvals[sin] == 0.05) and np.all(pen.hvals[~sin] == 0.0)
    assert np.all(q.colind[sin] % 3 == 0)                                              # on theta_k
    nlp = nlpmodels.SepFuncConModel(pen)
    assert np.max(np.abs(pen.b)) <= 1e-14 and np.max(np.abs(nlp.cons(q.xhat))) <= 1e-14
    ctrl = (np.arange(q.n) % 3 == 2) & (np.arange(q.n) < 600)
    assert np.all(q.qdiag[ctrl] == 0.1) and np.all(q.qdiag[~ctrl] == 1.0)
    assert np.array_equal(q.d, -0.5 * q.qdiag * q.xhat)
    assert q.xhat[0] == 0.3 and 0.0 < np.max(np.abs(q.x - q.xhat)) <= 0.1


def test_host_fps_solve_on_the_pendulum_with_trunk():
    from fps_amd.fps_solve import fps_solve

    data = problems.pendulum_like(200)
    nlp = nlpmodels.SepFuncConModel(data)
    st = fps_solve(nlp, data.qp.x, atol=SE, rtol=SE, max_iter=30, subproblem_solver="trunk", qds=_SparseExtrasOracle(nlp))
    xs, lam = st.solution, st.multipliers
    primal = np.max(np.abs(nlp.cons(xs)))
    dual = np.max(np.abs(nlp.grad(xs) + nlp.jtprod(xs, lam)))
    print(f"\npendulum N=200, trunk: {st.status} in {st.iter} outer iterations, |c| {primal:.2e}, |grad f + J'lambda| {dual:.2e}, "
          f"{st.solver_specific}")
    assert st.status == "first_order"
    assert primal <= 1e-10 and dual <= 1e-6
