"""The nonlinear (separable-quadratic) equality constraints of the banded back-end (fpsq_band_nlp_*, DeviceBandSepQuadNLP) as
far as they can be checked without a GPU: the model's derivatives against central differences, the CPU restatement
(tests/sepquad_ref.py) -- its -ys gradient IS the gradient of the penalty function, the literal +ys of `grad!` is not -- and
the declarations of the header and the binding."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import fps_amd  # noqa: E402,F401
from fps_amd import _lib, device_qp, fps_solve, nlpmodels, problems  # noqa: E402
from sepquad_ref import SepQuadRef  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SE = float(np.sqrt(np.finfo(float).eps))


def test_generator_keeps_xhat_feasible_and_the_pattern():
    qp = problems.pde_control_like(n=120, m=40, per_row=8, window=64, seed=3)
    data = problems.with_quadratic_constraints(qp, curv=0.3, seed=1)
    assert data.hvals.shape == qp.vals.shape and data.b.shape == (qp.m,)
    ratio = np.abs(data.hvals / qp.vals)
    assert ratio.min() >= 0.3 * 0.5 and ratio.max() <= 0.3 * 1.5 and (data.hvals / qp.vals < 0).any()
    nlp = nlpmodels.SepQuadConModel(data)
    assert np.abs(nlp.cons(qp.xhat)).max() < 1e-13
    assert np.array_equal(nlp.meta.lcon, np.zeros(qp.m))
    again = problems.with_quadratic_constraints(qp, curv=0.3, seed=1)
    assert np.array_equal(again.hvals, data.hvals) and np.array_equal(again.b, data.b)


def test_model_derivatives_against_central_differences():
    """jac_coord, hprod (the constraint part) and ghjvprod of SepQuadConModel against central differences of cons; the
    constraints are quadratic, so a central difference of cons is exact up to rounding: |c| eps / h ~ 1e-11 at h = 1e-5."""
    qp = problems.pde_control_like(n=120, m=40, per_row=8, window=64, seed=3)
    nlp = nlpmodels.SepQuadConModel(problems.with_quadratic_constraints(qp, curv=0.3, seed=1))
    rng = np.random.default_rng(0)
    x, h = qp.x, 1e-5
    J = nlp._J(x).toarray()
    Jfd = np.column_stack([(nlp.cons(x + h * e) - nlp.cons(x - h * e)) / (2 * h) for e in np.eye(qp.n)])
    assert np.abs(J - Jfd).max() < 1e-9 * np.abs(J).max()
    v, g, y = rng.standard_normal(qp.n), rng.standard_normal(qp.n), rng.standard_normal(qp.m)
    assert np.allclose(nlp.jprod(x, v), J @ v, rtol=0, atol=1e-12 * np.abs(J @ v).max())
    assert np.allclose(nlp.jtprod(x, y), J.T @ y, rtol=0, atol=1e-12 * np.abs(J.T @ y).max())
    # d/dt J(x + t v)'y = (sum_i y_i Hess c_i) v
    hv_fd = (nlp.jtprod(x + h * v, y) - nlp.jtprod(x - h * v, y)) / (2 * h)
    hv = nlp.hprod(x, y, v, obj_weight=0.0)
    assert np.abs(hv - hv_fd).max() < 1e-9 * np.abs(hv).max()
    assert np.array_equal(nlp.hprod(x, np.zeros(qp.m), v), qp.qdiag * v)
    # (g' Hess c_i v)_i = d/dt (J(x + t v) g)_i
    gh_fd = (nlp.jprod(x + h * v, g) - nlp.jprod(x - h * v, g)) / (2 * h)
    gh = nlp.ghjvprod(x, g, v)
    assert np.abs(gh - gh_fd).max() < 1e-9 * np.abs(gh).max()
    # ... and both from cons alone: (u' Hess c_i v)_i by the mixed central second difference, exact for quadratic constraints
    # up to rounding, |c| eps / (4 h2^2) ~ 1e-9 at h2 = 1e-3, against values of order 0.1 .. 1
    h2 = 1e-3

    def mixed(u, w):
        return (nlp.cons(x + h2 * (u + w)) - nlp.cons(x + h2 * (u - w)) - nlp.cons(x - h2 * (u - w))
                + nlp.cons(x - h2 * (u + w))) / (4 * h2 * h2)

    assert np.abs(gh - mixed(g, v)).max() < 1e-6 * np.abs(gh).max()
    u = rng.standard_normal(qp.n)
    assert abs(u @ hv - y @ mixed(u, v)) < 1e-6 * np.abs(y).max() * np.abs(mixed(u, v)).max() * qp.m


PROBLEMS = {
    "pde": lambda: problems.pde_control_like(n=4000, m=400, per_row=16, window=512, seed=21),
    "aug2dc": lambda: problems.aug2dc_like(N=30),
}


@pytest.mark.parametrize("name", list(PROBLEMS))
@pytest.mark.parametrize("rho,delta", [(0.0, 0.0), (1.0, SE)])
def test_the_restatements_gradient_is_the_gradient_of_phi(name, rho, delta):
    """Directional derivatives against central differences of obj, h = 1e-4 max(1, |x|inf), three seeded unit directions:
    the -ys form agrees within 1e-8 relative (measured <= 2e-10), the literal +ys form of `grad!` (FletcherPenaltyNLP.grad)
    misses by more than 1e-3 on every direction (measured >= 3.9e-3)."""
    qp = PROBLEMS[name]()
    ref = SepQuadRef(problems.with_quadratic_constraints(qp, curv=0.3, seed=7), 1e3, rho, delta)
    x = qp.x
    g_true = ref.objgrad(x)["gx"]
    g_lit = ref.grad_literal(x).copy()
    hh = 1e-4 * max(1.0, np.abs(x).max())
    rng = np.random.default_rng(1)
    for _ in range(3):
        d = rng.standard_normal(qp.n)
        d /= np.linalg.norm(d)
        fd = (ref.obj(x + hh * d) - ref.obj(x - hh * d)) / (2 * hh)
        e_true, e_lit = abs(g_true @ d - fd) / abs(fd), abs(g_lit @ d - fd) / abs(fd)
        print(f"\n{name} rho={rho} delta={delta:.1e}: -ys {e_true:.2e}  literal {e_lit:.2e}")
        assert e_true < 1e-8
        assert e_lit > 1e-3


def test_header_and_binding_declare_the_entries():
    src = open(os.path.join(ROOT, "include", "fpsq.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    arity = {"fpsq_band_nlp_create": 7, "fpsq_band_nlp_destroy": 1, "fpsq_band_nlp_objgrad": 13, "fpsq_band_nlp_hprod": 8,
             "fpsq_band_nlp_cons": 4}
    typed = {n: a for n, _, a in _lib.SYMBOLS}
    for name, k in arity.items():
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert decl, name
        assert len(decl.group(1).split(",")) == k, name
        assert len(typed[name]) == k, name
    assert "typedef struct fpsq_band_nlp_s *fpsq_band_nlp;" in src
    # the section lies behind the fpsq_band_qp_* group
    assert src.index("fpsq_band_nlp_create") > src.index("fpsq_band_set_input_stream")
    params = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert params(device_qp.DeviceBandSepQuadNLP.objgrad) == params(device_qp.DeviceBandEqQP.objgrad)
    assert params(device_qp.DeviceBandSepQuadNLP.hprod) == params(device_qp.DeviceBandEqQP.hprod)
    assert params(device_qp.DeviceBandSepQuadNLP.__init__) == ["self", "nlp_data", "sigma", "rho", "delta", "eta", "device",
                                                              "ldlt_tol", "ldlt_r2"]
    assert device_qp.DeviceBandSepQuadNLP.nonlinear is True
    for name in ("cons", "jac_mul", "set_delta", "info", "close"):
        assert callable(getattr(device_qp.DeviceBandSepQuadNLP, name))


def test_fps_solve_device_still_takes_the_old_classes(monkeypatch):
    """The penalty wrapper is chosen by the model's `nonlinear` attribute alone: every existing class gets _DevicePenalty."""
    made = []
    monkeypatch.setattr(fps_solve, "_outer_loop", lambda pen, *a, **k: made.append(type(pen)) or "ran")
    for cls in (fps_solve._DevicePenalty, fps_solve._DeviceNLPPenalty):
        monkeypatch.setattr(cls, "__init__", lambda self, dev, torch, ha=2: None)

    class Dev:
        def set_delta(self, d):
            self.delta = d

    for cls in (device_qp.DeviceEqQP, device_qp.DeviceSparseHessianEqQP, device_qp.DeviceBandEqQP,
                device_qp.DeviceBorderedBandEqQP, device_qp.DeviceArrowBandEqQP):
        assert not getattr(cls, "nonlinear", False)
    old = Dev()
    assert fps_solve.fps_solve_device(old, None) == "ran" and made == [fps_solve._DevicePenalty]
    new = Dev()
    new.nonlinear = True
    assert fps_solve.fps_solve_device(new, None) == "ran" and made[-1] is fps_solve._DeviceNLPPenalty
    assert issubclass(fps_solve._DeviceNLPPenalty, fps_solve._DevicePenalty)
    assert "_x_at" not in vars(fps_solve._DevicePenalty)
