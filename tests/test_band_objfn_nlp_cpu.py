"""Elementwise function terms in the OBJECTIVE of the banded nonlinear model (fpsq_band_nlp_set_objective_terms,
problems.with_objective_terms), the part that needs no GPU: the declaration, the unchanged function table, the three host
models with terms against central differences and against themselves without, the movement that lets the GPU bars tell the
model from the one without terms, and a host solve of the pendulum with its potential energy and an exponential control cost."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import fps_amd  # noqa: E402,F401
import lane_group_cases as lg  # noqa: E402
import objfn_cases as oc  # noqa: E402
from coupled_quad_ref import CoupledQuadRef  # noqa: E402
from fps_amd import _lib, device_qp, nlpmodels, problems  # noqa: E402
from sepfunc_ref import SepFuncRef, fn_codes, fn_data  # noqa: E402
from sepquad_ref import SepQuadRef, _SparseExtrasOracle  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SE = float(np.sqrt(np.finfo(float).eps))
SIGMA = 1e3
ENTRY = "fpsq_band_nlp_set_objective_terms"


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def _shape():
    """the 120 x 40 shape of tests/test_band_fn_nlp_cpu.py and its function model"""
    qp = problems.pde_control_like(n=120, m=40, per_row=8, window=64, seed=3)
    return qp, problems.with_function_constraints(qp, curv=0.3, seed=7, codes=fn_codes(qp.vals.size))


def _three(qp):
    """(host class, data) for the three kinds of model on one EqQP"""
    return ((nlpmodels.SepQuadConModel, problems.with_quadratic_constraints(qp, curv=0.3, seed=7)),
            (nlpmodels.SepFuncConModel, problems.with_function_constraints(qp, curv=0.3, seed=7, codes=fn_codes(qp.vals.size))),
            (nlpmodels.CoupledQuadConModel, problems.with_coupled_constraints(qp, curv=0.3, pairs=2, seed=7)))


def test_the_entry_is_declared_typed_and_leaves_the_others_alone():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fpsq.h")).read(), flags=re.S)
    decl = re.search(rf"int {ENTRY}\(([^)]*)\);", text)
    assert decl and [p.strip() for p in decl.group(1).split(",")] == ["fpsq_band b", "fpsq_band_nlp nlp", "const double *w",
                                                                      "const uint8_t *codes"]
    typed = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    assert ENTRY in typed and len(typed[ENTRY][1]) == 4
    # one entry for every kind of model, no further create entries
    assert sorted(n for n in typed if n.startswith("fpsq_band_nlp_create")) == [
        "fpsq_band_nlp_create", "fpsq_band_nlp_create_arrow", "fpsq_band_nlp_create_coupled", "fpsq_band_nlp_create_coupled_arrow",
        "fpsq_band_nlp_create_fn"]
    # the classes: the method is the base class's, the parameter lists stay
    for cls in (device_qp.DeviceArrowBandSepQuadNLP, device_qp.DeviceBandCoupledQuadNLP, device_qp.DeviceArrowBandCoupledQuadNLP,
                device_qp.DeviceBandSepFuncNLP, device_qp.DeviceArrowBandSepFuncNLP):
        assert cls.set_objective_terms is device_qp.DeviceBandSepQuadNLP.set_objective_terms
        assert cls.objgrad is device_qp.DeviceBandSepQuadNLP.objgrad
    assert list(inspect.signature(device_qp.DeviceBandSepQuadNLP.set_objective_terms).parameters) == ["self", "w", "codes"]


def test_the_function_table_is_unchanged():
    text = open(os.path.join(ROOT, "include", "fpsq.h")).read()
    got = [(k, int(v)) for k, v in re.findall(r"FPSQ_FN_([A-Z0-9]+) = (\d+)", text)]
    assert got == [("HALFSQ", 0), ("CUBE6", 1), ("SIN", 2), ("COS", 3), ("EXP", 4), ("TANH", 5), ("COUNT", 6)]
    assert len(problems.FN_TABLE) == 6
    # the device side evaluates the objective's terms through the ONE device function of the constraint kernels
    src = open(os.path.join(ROOT, "fletcherpenaltysolver.jl_amd", "csrc", "fpsq_band_nlp.hip.h")).read()
    assert src.count("void bn_fn_eval(") == 1 and src.count("case FPSQ_FN_") == 5
    body = src[src.index("void k_bn_objfn("):]
    assert "bn_fn_eval(code[j], xv, p0, p1, p2);" in body[:body.index("\n}\n")]


def test_the_generators():
    qp, data = _shape()
    w, codes = oc.terms(qp.n)
    assert codes.dtype == np.uint8 and set(np.unique(codes[w != 0])) == set(range(6))
    assert 0.15 < np.mean(w == 0) < 0.35 and np.all((np.abs(w[w != 0]) >= 0.5) & (np.abs(w[w != 0]) < 1.5))
    assert not hasattr(data, "obj_w")
    out = problems.with_objective_terms(data, w, codes)
    assert out is not data and not hasattr(data, "obj_w") and type(out) is type(data)
    assert np.array_equal(out.obj_w, w) and np.array_equal(out.obj_codes, codes) and out.codes is data.codes and out.qp is data.qp
    assert np.all(problems.with_objective_terms(data, w).obj_codes == 0)
    bad = codes.copy()
    bad[np.flatnonzero(w == 0)[0]] = 9       # a code outside the table is harmless under w = 0 ...
    problems.with_objective_terms(data, w, bad)
    bad[np.flatnonzero(w != 0)[0]] = 6       # ... and refused under a weight
    with pytest.raises(AssertionError):
        problems.with_objective_terms(data, w, bad)
    # the positional constructions keep working
    assert isinstance(problems._sepfunc(qp, data.hvals, data.codes), problems.SepFuncNLP)
    pen, base = problems.pendulum_energy_like(200), problems.pendulum_like(200)
    q = pen.qp
    idx = np.arange(q.n)
    theta, ctrl = idx % 3 == 0, (idx % 3 == 2) & (idx < 600)
    assert (q.n, q.m) == (602, 400) and np.array_equal(pen.b, base.b) and np.array_equal(pen.codes, base.codes)
    assert np.all(pen.obj_w[theta] == -0.5) and np.all(pen.obj_codes[theta] == problems.FN_COS) and theta.sum() == 201
    assert np.all(pen.obj_w[ctrl] == 0.05) and np.all(pen.obj_codes[ctrl] == problems.FN_EXP) and ctrl.sum() == 200
    assert np.all(pen.obj_w[~(theta | ctrl)] == 0.0)
    m, m0 = nlpmodels.SepFuncConModel(pen), nlpmodels.SepFuncConModel(base)
    x = q.x
    assert abs(m.obj(x) - m0.obj(x) - (-0.5 * np.cos(x[theta]).sum() + 0.05 * np.exp(x[ctrl]).sum())) <= 1e-12


@pytest.mark.parametrize("kind", range(3), ids=["sepquad", "sepfunc", "coupled"])
def test_host_models_with_terms_against_central_differences(kind):
    """grad against central differences of obj, coordinate by coordinate, and hprod(., y = 0) against a central difference of
    grad along v.  Step 1e-6 as in tests/test_band_fn_nlp_cpu.py.  Bars: the truncation h^2/6 |f'''| <= 1e-12 is nothing; the
    rounding of a difference of two values of f is 2 eps |f| / (2 h) = 2.2e-10 |f| per coordinate, held with a factor 4 of
    room; grad has entries of size <= ~5, so its difference quotient carries ~1e-9 absolute against max|Hv| ~ 1, and the
    bar is that file's 1e-8 relative."""
    qp = _shape()[0]
    cls, data = _three(qp)[kind]
    nlp = cls(oc.with_terms(data))
    x, h = qp.x, 1e-6
    v = np.random.default_rng(4).standard_normal(qp.n)
    g = nlp.grad(x)
    fd = np.empty(qp.n)
    for j in range(qp.n):
        e = np.zeros(qp.n)
        e[j] = h
        fd[j] = (nlp.obj(x + e) - nlp.obj(x - e)) / (2 * h)
    bar = 4 * 2.2e-10 * max(abs(nlp.obj(x)), 1.0)
    print(f"\n{cls.__name__}: |f| = {abs(nlp.obj(x)):.2f}, grad - fd = {np.max(np.abs(fd - g)):.2e} (bar {bar:.1e})")
    assert np.max(np.abs(fd - g)) <= bar
    y0 = np.zeros(qp.m)
    Hv = nlp.hprod(x, y0, v)
    assert _rel(Hv, (nlp.grad(x + h * v) - nlp.grad(x - h * v)) / (2 * h)) <= 1e-8
    # obj_weight scales the objective's part alone, the constraints' curvature is untouched by the terms
    y = np.random.default_rng(5).standard_normal(qp.m)
    plain = cls(data)
    assert _rel(nlp.hprod(x, y, v, 0.0), plain.hprod(x, y, v, 0.0)) == 0.0
    assert _rel(nlp.hprod(x, y, v, 1.0) - nlp.hprod(x, y, v, 0.0), Hv) <= 1e-14
    assert np.array_equal(nlp.cons(x), plain.cons(x)) and np.array_equal(nlp.jac_coord(x), plain.jac_coord(x))


@pytest.mark.parametrize("kind", range(3), ids=["sepquad", "sepfunc", "coupled"])
def test_no_terms_and_zero_weights_give_the_old_values_and_code_0_is_a_shift_of_qdiag(kind):
    import dataclasses

    qp = _shape()[0]
    cls, data = _three(qp)[kind]
    rng = np.random.default_rng(6)
    x, y, v = qp.x.copy(), rng.standard_normal(qp.m), rng.standard_normal(qp.n)
    old = cls(data)
    # what the class computed before it knew the terms: the QP's objective, diag(q) in hprod
    assert old.obj(x) == float(x @ (0.5 * qp.qdiag * x + qp.d)) and np.array_equal(old.grad(x), qp.qdiag * x + qp.d)
    assert np.array_equal(old.hprod(x, 0 * y, v), qp.qdiag * v)
    _, codes = oc.terms(qp.n)
    x800 = x.copy()
    x800[np.flatnonzero(codes == problems.FN_EXP)[0]] = 800.0      # exp(800) = inf, never evaluated under w = 0
    zero = cls(problems.with_objective_terms(data, np.zeros(qp.n), codes))
    for at in (x, x800):
        assert zero.obj(at) == old.obj(at) and np.array_equal(zero.grad(at), old.grad(at))
        assert np.array_equal(zero.hprod(at, y, v), old.hprod(at, y, v))
    # codes all 0: w_j 1/2 x_j^2 is a shift of qdiag
    w, _ = oc.terms(qp.n)
    half = cls(problems.with_objective_terms(data, w))
    shifted = cls(dataclasses.replace(data, qp=dataclasses.replace(qp, qdiag=qp.qdiag + w)))
    assert abs(half.obj(x) - shifted.obj(x)) <= 1e-14 * abs(shifted.obj(x))
    assert _rel(half.grad(x), shifted.grad(x)) <= 1e-14 and _rel(half.hprod(x, y, v), shifted.hprod(x, y, v)) <= 1e-14


@pytest.mark.parametrize("name", lg.NAMES)
def test_the_bars_tell_the_model_from_the_one_without_terms(name):
    """the movement condition: dropping the terms moves every vector of the restatement by >= 1e-4 and fx by >= 1e-5 (relative),
    five decades and more above the GPU bars of 1e-9 and 1e-12"""
    qp = lg.qp(name)
    v = np.random.default_rng(0).standard_normal(qp.n)
    out = []
    for data in (oc.objfn_data(name), fn_data(name)):
        ref = SepFuncRef(data, SIGMA, 1.0, SE, 0.5, qp.xhat, kept=True)
        e = ref.objgrad(qp.x)
        e["Hv2"], e["Hv1"] = ref.hprod(qp.x, v, 2), ref.hprod(qp.x, v, 1)
        out.append(e)
    a, b = out
    moves = {k: _rel(b[k], a[k]) for k in ("gx", "ys", "gs", "Hv2", "Hv1")}
    moves["fx"] = abs(b["fx"] - a["fx"]) / abs(a["fx"])
    print(f"\n{name}: " + " ".join(f"{k} moves {m:.1e}" for k, m in moves.items()))
    assert np.array_equal(a["c"], b["c"])
    assert all(m >= 1e-4 for k, m in moves.items() if k != "fx") and moves["fx"] >= 1e-5


def test_the_partition_the_lane_group_cases_reach():
    """k_bn_objfn's grid and chunk on the 14 cases (the docstring of tests/test_gpu_band_objfn_nlp.py): which of them give a
    thread two entries, which reach the capped grid, which have a ragged last chunk and workgroups behind n"""
    part = {}
    for name, c in lg.CASES.items():
        grid = min(lg.tiles(c.mpad, c.lgA), lg.MAX_GRID)
        chunk = -(-c.n // grid)
        part[name] = (grid, chunk, sum(1 for b in range(grid) if b * chunk >= c.n))
    assert {k for k, (_, chunk, _) in part.items() if chunk > 256} == {"thin", "lg2"}
    assert part["thin"] == part["lg2"] == (3, 300, 0)
    assert {k for k, c in lg.CASES.items() if lg.tiles(c.mpad, c.lgA) > lg.MAX_GRID} == {"stride"}
    assert part["stride"] == (2048, 5, 248)
    assert {k for k, (_, _, empty) in part.items() if empty} >= {"m-near-n", "ragged", "both-64", "stride"}
    assert lg.CASES["m-near-n"].n % part["m-near-n"][1] == 2 and lg.CASES["ragged"].n % part["ragged"][1] == 2


def test_the_restatement_gradient_with_terms_is_the_gradient_of_its_obj():
    """on the three restatements the GPU tests use: the -ys form against central differences of obj along three directions,
    the bar of tests/test_band_fn_nlp_cpu.py"""
    qp = _shape()[0]
    refs = (SepQuadRef, SepFuncRef, CoupledQuadRef)
    for (cls, data), ref_cls in zip(_three(qp), refs):
        ref = ref_cls(oc.with_terms(data), SIGMA, 1.0, SE, 0.5, qp.xhat)
        assert getattr(ref.model.data, "obj_w", None) is not None
        gx = ref.objgrad(qp.x)["gx"]
        rng = np.random.default_rng(5)
        h = 1e-6
        for _ in range(3):
            u = rng.standard_normal(qp.n)
            u /= np.linalg.norm(u)
            fd = (ref.obj(qp.x + h * u) - ref.obj(qp.x - h * u)) / (2 * h)
            err = abs(gx @ u - fd) / abs(fd)
            print(f"\n{ref_cls.__name__}: {err:.2e}")
            assert err <= 1e-7


def test_host_fps_solve_on_the_pendulum_with_energy_terms():
    from fps_amd.fps_solve import fps_solve

    data = problems.pendulum_energy_like(200)
    nlp = nlpmodels.SepFuncConModel(data)
    st = fps_solve(nlp, data.qp.x, atol=SE, rtol=SE, max_iter=30, subproblem_solver="trunk", qds=_SparseExtrasOracle(nlp))
    xs, lam = st.solution, st.multipliers
    primal = np.max(np.abs(nlp.cons(xs)))
    dual = np.max(np.abs(nlp.grad(xs) + nlp.jtprod(xs, lam)))
    print(f"\npendulum with energy terms N=200, trunk: {st.status} in {st.iter} outer iterations, |c| {primal:.2e}, "
          f"|grad f + J'lambda| {dual:.2e}, {st.solver_specific}")
    assert st.status == "first_order"
    assert primal <= 1e-10 and dual <= 1e-6
