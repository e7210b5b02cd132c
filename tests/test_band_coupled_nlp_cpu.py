"""Coupled quadratic constraints on the banded device-resident NLP (fpsq_band_nlp_create_coupled, DeviceBandCoupledQuadNLP) as
far as they can be checked without a GPU: the host model's derivatives against central differences, the CPU restatement
(tests/coupled_quad_ref.py) -- its -ys gradient IS the gradient of the penalty function, the literal +ys of `grad!` is not --,
the numpy restatement of the device's assembly (tests/coupled_nlp_model.py) against that yardstick, the GPU cases
(tests/coupled_cases.py: the couplings must matter on each), and the declarations of the header and the binding."""
import inspect
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import fps_amd  # noqa: E402,F401
import coupled_cases as cc  # noqa: E402
from coupled_nlp_model import CoupledNLPModel, build_lists  # noqa: E402
from coupled_quad_ref import CoupledQuadRef  # noqa: E402
from fps_amd import _lib, device_qp, nlpmodels, problems  # noqa: E402
from sepquad_ref import SepQuadRef  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SE = float(np.sqrt(np.finfo(float).eps))


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def _tiny():
    qp = problems.pde_control_like(n=120, m=40, per_row=8, window=64, seed=3)
    return qp, problems.with_coupled_constraints(qp, curv=0.3, pairs=3, seed=1)


def test_generators_keep_xhat_feasible_and_the_terms_on_the_pattern():
    qp, data = _tiny()
    sep = problems.with_quadratic_constraints(qp, curv=0.3, seed=1)
    assert np.array_equal(data.hvals, sep.hvals)                      # the draw of with_quadratic_constraints
    assert data.nterms == 3 * qp.m and data.t_row.dtype == np.int32 and data.t_w.dtype == np.float64
    assert np.all(data.t_j != data.t_k)
    pattern = set(zip(np.repeat(np.arange(qp.m), np.diff(qp.rowptr)).tolist(), qp.colind.tolist()))
    assert all((r, j) in pattern and (r, k) in pattern for r, j, k in zip(data.t_row.tolist(), data.t_j.tolist(),
                                                                          data.t_k.tolist()))
    first, last = qp.colind[qp.rowptr[:-1]], qp.colind[qp.rowptr[1:] - 1]
    pairs = set(zip(data.t_row.tolist(), data.t_j.tolist(), data.t_k.tolist()))
    assert all((i, int(first[i]), int(last[i])) in pairs for i in range(qp.m))        # the row's first and last
    a = dict(zip(zip(np.repeat(np.arange(qp.m), np.diff(qp.rowptr)).tolist(), qp.colind.tolist()), qp.vals.tolist()))
    ratio = np.array([abs(w) / np.sqrt(abs(a[r, j] * a[r, k])) for r, j, k, w in zip(data.t_row.tolist(), data.t_j.tolist(),
                                                                                   data.t_k.tolist(), data.t_w.tolist())])
    assert ratio.min() >= 0.3 * 0.5 and ratio.max() <= 0.3 * 1.5 and (data.t_w < 0).any() and (data.t_w > 0).any()
    assert np.abs(nlpmodels.CoupledQuadConModel(data).cons(qp.xhat)).max() < 1e-13
    again = problems.with_coupled_constraints(qp, curv=0.3, pairs=3, seed=1)
    assert np.array_equal(again.t_w, data.t_w) and np.array_equal(again.b, data.b)
    third = problems.with_coupled_constraints(qp, curv=0.3, pairs=3, seed=1, rows=np.arange(0, qp.m, 3))
    assert set(third.t_row.tolist()) == set(range(0, qp.m, 3))
    # the real model: three entries per row, the control's entry an explicit zero, one term per row on it
    N = 50
    bil = problems.bilinear_control_like(N=N, tau=0.25, alpha=0.1)
    q = bil.qp
    assert (q.n, q.m, q.nnz, bil.nterms) == (2 * N + 1, N, 3 * N, N) and np.all(np.diff(q.rowptr) == 3)
    assert np.all(q.vals[1::3] == 0.0) and np.all(bil.hvals == 0.0)
    assert np.array_equal(bil.t_j, q.colind[0::3]) and np.array_equal(bil.t_k, q.colind[1::3]) and np.all(bil.t_w == -0.25)
    nlp = nlpmodels.CoupledQuadConModel(bil)
    assert np.abs(nlp.cons(q.xhat)).max() < 1e-13
    y, u = q.x[0::2], q.x[1::2]
    assert np.allclose(nlp.cons(q.x), y[1:] - y[:-1] + 0.25 * y[:-1] - 0.25 * u * y[:-1] - bil.b, rtol=0, atol=1e-14)


def test_model_derivatives_against_central_differences():
    """_J, hprod (the constraint part) and ghjvprod of CoupledQuadConModel against central differences of cons; the constraints
    are quadratic, so a central difference is exact up to rounding: |c| eps / h ~ 1e-11 at h = 1e-5."""
    qp, data = _tiny()
    nlp = nlpmodels.CoupledQuadConModel(data)
    rng = np.random.default_rng(0)
    x, h = qp.x, 1e-5
    J = nlp._J(x).toarray()
    Jfd = np.column_stack([(nlp.cons(x + h * e) - nlp.cons(x - h * e)) / (2 * h) for e in np.eye(qp.n)])
    assert np.abs(J - Jfd).max() < 1e-9 * np.abs(J).max()
    assert np.abs(J - nlpmodels.SepQuadConModel(cc.without_terms(data))._J(x).toarray()).max() > 1e-2     # the terms are live
    v, g, y = rng.standard_normal(qp.n), rng.standard_normal(qp.n), rng.standard_normal(qp.m)
    assert np.allclose(nlp.jprod(x, v), J @ v, rtol=0, atol=1e-12 * np.abs(J @ v).max())
    assert np.allclose(nlp.jtprod(x, y), J.T @ y, rtol=0, atol=1e-12 * np.abs(J.T @ y).max())
    # d/dt J(x + t v)'y = (sum_i y_i Hess c_i) v = (diag(H'y) + Wo(y)) v
    hv_fd = (nlp.jtprod(x + h * v, y) - nlp.jtprod(x - h * v, y)) / (2 * h)
    hv = nlp.hprod(x, y, v, obj_weight=0.0)
    assert np.abs(hv - hv_fd).max() < 1e-9 * np.abs(hv).max()
    assert np.array_equal(nlp.hprod(x, np.zeros(qp.m), v), qp.qdiag * v)
    Wo = nlp._Wo(y).toarray()
    assert np.array_equal(Wo, Wo.T) and not Wo.diagonal().any() and np.abs(Wo).max() > 1e-2
    # (g' Hess c_i v)_i = d/dt (J(x + t v) g)_i
    gh_fd = (nlp.jprod(x + h * v, g) - nlp.jprod(x - h * v, g)) / (2 * h)
    gh = nlp.ghjvprod(x, g, v)
    assert np.abs(gh - gh_fd).max() < 1e-9 * np.abs(gh).max()
    # ... and from cons alone: (u' Hess c_i v)_i by the mixed central second difference, exact for quadratic constraints up to
    # rounding, |c| eps / (4 h2^2) ~ 1e-9 at h2 = 1e-3
    h2 = 1e-3

    def mixed(u, w):
        return (nlp.cons(x + h2 * (u + w)) - nlp.cons(x + h2 * (u - w)) - nlp.cons(x - h2 * (u - w))
                + nlp.cons(x - h2 * (u + w))) / (4 * h2 * h2)

    assert np.abs(gh - mixed(g, v)).max() < 1e-6 * np.abs(gh).max()


GRAD_PROBLEMS = {
    "pde": lambda: problems.pde_control_like(n=4000, m=400, per_row=16, window=512, seed=21),
    "aug2dc": lambda: problems.aug2dc_like(N=30),
}


@pytest.mark.parametrize("name", list(GRAD_PROBLEMS))
@pytest.mark.parametrize("rho,delta", [(0.0, 0.0), (1.0, SE)])
def test_the_restatements_gradient_is_the_gradient_of_phi(name, rho, delta):
    """tests/test_band_nlp_cpu.py's check and bars on the coupled model (curv = 0.3, pairs = 2, seed 7, sigma = 1e3):
    directional derivatives against central differences of obj, h = 1e-4 max(1, |x|inf), three seeded unit directions.  The
    -ys form agrees within 1e-8 relative (measured <= 1.3e-10 on pde, <= 3.7e-11 on aug2dc), the literal +ys form of `grad!`
    misses by more than 1e-3 on every direction (measured >= 1.8e-2 on pde, >= 1.7e-2 on aug2dc)."""
    qp = GRAD_PROBLEMS[name]()
    ref = CoupledQuadRef(problems.with_coupled_constraints(qp, curv=0.3, pairs=2, seed=7), 1e3, rho, delta)
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


def _by_first_column(qp):
    """a stored order for shuffled rows: by the row's first column (what a bandwidth-reducing pass would roughly do)"""
    return np.argsort(qp.colind[qp.rowptr[:-1]], kind="stable")


ASSEMBLY = {
    # name -> (the model, the stored row order: stored row -> the caller's; None = natural)
    "natural": (lambda: problems.with_coupled_constraints(cc.small_qp(), 0.3, 2, 7), lambda qp: None),
    "row-shuffled": (lambda: problems.with_coupled_constraints(cc.shuffled(cc.small_qp(), 5), 0.3, 2, 7), _by_first_column),
    "two-chain": (lambda: problems.with_coupled_constraints(problems.aug2dc_like(N=16), 0.3, 2, 7),
                  lambda qp: np.concatenate([np.arange(0, qp.m, 2), np.arange(1, qp.m, 2)])),   # two interleaved chains
    "bilinear": (lambda: problems.bilinear_control_like(N=300), lambda qp: np.arange(qp.m)[::-1]),
}


@pytest.mark.parametrize("name", list(ASSEMBLY))
def test_the_devices_assembly_restated_in_numpy_agrees_with_the_yardstick(name):
    """tests/coupled_nlp_model.py -- the lists of csrc/fpsq_coupled.h and every sum the k_bcn_* launches form -- against
    tests/coupled_quad_ref.py within 1e-13 relative (measured <= 6e-15), delta = sqrt(eps) (the yardstick's Val(1) solves with
    tau = max(delta, 1e-14)), (rho, eta) = (0, 0) and (1, 0.5)."""
    make, order = ASSEMBLY[name]
    data = make()
    qp = data.qp
    rperm = order(qp)
    mdl = CoupledNLPModel(data, rperm)
    L = mdl.L
    # the lists themselves: every term sits at both of its stored entries, S is symmetric without a diagonal, its rows and
    # the contributors of an entry ascend
    assert sum(len(p) for p in L["partners"]) == 2 * data.nterms == sum(len(p) for p in L["t_partners"])
    srow = np.repeat(np.arange(qp.n), np.diff(L["srp"]))
    S = set(zip(srow.tolist(), L["sci"].tolist()))
    assert all((k, j) in S for j, k in S) and all(j != k for j, k in S) and len(S) == L["sci"].size
    assert all(np.all(np.diff(L["sci"][L["srp"][j]:L["srp"][j + 1]]) > 0) for j in range(qp.n))
    assert all(all(a[0] < b[0] for a, b in zip(lst, lst[1:])) for lst in L["contrib"])
    assert sum(len(lst) for lst in L["contrib"]) == 2 * data.nterms
    x, xk = qp.x, qp.xhat
    nlp = nlpmodels.CoupledQuadConModel(data)
    J = nlp._J(x)
    stored = mdl._J(mdl.vals(x))
    assert _rel(stored.toarray(), J.toarray()[mdl.rperm]) < 1e-15
    assert _rel(mdl._Jt(mdl.tvals(x)).toarray(), stored.T.toarray()) == 0.0
    v = np.random.default_rng(0).standard_normal(qp.n)
    for rho, eta in ((0.0, 0.0), (1.0, 0.5)):
        ref = CoupledQuadRef(data, cc.SIGMA, rho, SE, eta, xk)
        e = ref.objgrad(x)
        a = mdl.objgrad(x, cc.SIGMA, rho, SE, eta, xk)
        errs = {k: _rel(a[k], e[k]) for k in ("gx", "ys", "gs", "c")}
        errs["fx"] = abs(a["fx"] - e["fx"]) / abs(e["fx"])
        errs["cons"] = _rel(mdl.cons(x), e["c"])
        errs["Hv2"] = _rel(mdl.hprod(v, cc.SIGMA, rho, eta, 2), ref.hprod(x, v, 2))
        errs["Hv1"] = _rel(mdl.hprod(v, cc.SIGMA, rho, eta, 1), ref.hprod(x, v, 1))
        print(f"\n{name} rho={rho} eta={eta}: " + " ".join(f"{k}={v_:.1e}" for k, v_ in errs.items()))
        for k, err in errs.items():
            assert err < 1e-13, (k, err)
    # leaving the terms out of one list is seen: the restatement is sensitive to what it restates
    broken = CoupledNLPModel(data, rperm)
    broken.L["contrib"][0] = []
    assert _rel(broken.objgrad(x, cc.SIGMA, 1.0, SE, 0.5, xk)["gx"], e["gx"]) > 1e-9


def test_build_lists_refuses_what_the_entry_refuses():
    qp, data = _tiny()
    m, n = qp.m, qp.n
    ident = np.arange(m)
    t_perm = np.lexsort((np.repeat(ident, np.diff(qp.rowptr)), qp.colind))
    row0 = qp.colind[qp.rowptr[0]:qp.rowptr[1]]
    off = int(np.setdiff1d(np.arange(n), row0)[0])
    j0, k0 = int(row0[0]), int(row0[1])

    def build(t_row, t_j, t_k, t_w):
        return build_lists(n, m, qp.rowptr, qp.colind, ident, t_perm, t_row, t_j, t_k, t_w)

    build([0], [j0], [k0], [0.1])
    for terms, needle in ((([m], [j0], [k0], [0.1]), "out of range"), (([0], [n], [k0], [0.1]), "out of range"),
                          (([0], [j0], [-1], [0.1]), "out of range"), (([0], [j0], [j0], [0.1]), "j = k"),
                          (([0, 0], [j0, k0], [k0, j0], [0.1, 0.2]), "listed twice"),
                          (([0], [off], [k0], [0.1]), "not an entry"), (([0], [j0], [off], [0.1]), "not an entry")):
        with pytest.raises(ValueError, match=needle):
            build(*terms)


def _compiler():
    for c in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    raise RuntimeError("no host C++ compiler found")


def _flat(lists):
    """a list of (index, w) lists as (ptr, index, w) arrays"""
    ptr = np.concatenate([[0], np.cumsum([len(p) for p in lists])])
    return ptr, np.array([c for p in lists for c, _ in p]), np.array([w for p in lists for _, w in p])


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_the_host_builder_gives_the_lists_of_its_numpy_restatement(tmp_path, flags):
    """csrc/fpsq_coupled.h through the stand-alone tests/host/coupled_check.cpp (no GPU, no library; plain and under the
    address / undefined-behaviour sanitizers) against coupled_nlp_model.build_lists on a shuffled pattern with a stored row
    order of its own, entry by entry and bit by bit; and it refuses what the restatement refuses."""
    inc = os.path.join(ROOT, "fletcherpenaltysolver.jl_amd", "csrc")
    exe = str(tmp_path / "coupled_check")
    build = subprocess.run([_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", inc, "-o", exe,
                            os.path.join(ROOT, "tests", "host", "coupled_check.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    text = open(os.path.join(inc, "fpsq_coupled.h")).read()
    for word in ("hip", "dalloc", "getenv"):                    # plain host code: what makes it testable here
        assert word not in re.sub(r"//.*", "", text).lower(), word

    def run(mdl, t_row, t_j, t_k, t_w):
        qp = mdl.qp
        rinv = np.empty(qp.m, dtype=np.int64)
        rinv[mdl.rperm] = np.arange(qp.m)
        path = tmp_path / "problem.txt"
        with open(path, "w") as f:
            f.write(f"{qp.n} {qp.m} {mdl.t_perm.size} {len(t_w)}\n")
            for a in (mdl.rp, mdl.ci, rinv, mdl.t_perm):
                f.write(" ".join(str(int(v)) for v in a) + "\n")
            for r, j, k, w in zip(t_row, t_j, t_k, t_w):
                f.write(f"{int(r)} {int(j)} {int(k)} {float(w)!r}\n")
        out = subprocess.run([exe, str(path)], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        if out.stdout.startswith("error"):
            return out.stdout
        got = {}
        for line in out.stdout.splitlines():
            name, count, *items = line.split()
            got[name] = np.array([float(v) for v in items])
            assert len(items) == int(count)
        return got

    data = problems.with_coupled_constraints(cc.shuffled(problems.pde_control_like(n=300, m=60, per_row=8, window=64, seed=3), 5),
                                             0.3, 3, 7)
    mdl = CoupledNLPModel(data, _by_first_column(data.qp))
    got = run(mdl, data.t_row, data.t_j, data.t_k, data.t_w)
    L = mdl.L
    want = dict(zip(("pptr", "pcol", "pw"), _flat(L["partners"])))
    want.update(zip(("tpptr", "tpcol", "tpw"), _flat(L["t_partners"])))
    want.update(zip(("cptr", "crow", "cw"), _flat(L["contrib"])))
    want.update(tcol=L["tcol"], srp=L["srp"], sci=L["sci"])
    assert set(got) == set(want)
    for name, w in want.items():
        assert np.array_equal(got[name], np.asarray(w, dtype=float)), name
    qp = data.qp
    row0 = qp.colind[qp.rowptr[0]:qp.rowptr[1]]
    off = int(np.setdiff1d(np.arange(qp.n), row0)[0])
    j0, k0 = int(row0[0]), int(row0[1])
    for terms, needle in ((([qp.m], [j0], [k0], [0.1]), "out of range"), (([0], [j0], [qp.n], [0.1]), "out of range"),
                          (([0], [j0], [j0], [0.1]), "j = k"), (([0, 0], [j0, k0], [k0, j0], [0.1, 0.2]), "listed twice"),
                          (([0], [off], [k0], [0.1]), "not an entry"), (([0], [j0], [off], [0.1]), "not an entry")):
        msg = run(mdl, *terms)
        assert isinstance(msg, str) and needle in msg, (terms, msg)
    assert isinstance(run(mdl, [], [], [], []), dict)            # no terms: empty lists, no error


@pytest.mark.parametrize("case", list(cc.CASES))
def test_the_couplings_matter_on_every_gpu_case(case):
    """On each case of tests/test_gpu_band_coupled_nlp.py, at delta = sqrt(eps), (rho, eta) = (1, 0.5): dropping the terms
    (tests/sepquad_ref.py on the same a, h, b) moves the reference gx and Hv by more than 1e-3 relative, so the 1e-9 bar of the
    GPU tests tells the models apart; and Val(1) differs from Val(2) by more than 1e-6.  Measured (gx, Hv2, Hv1, |Hv1 - Hv2|):
      small 1.1e+0 1.3e-1 1.3e-1 2.6e-2        row-shuffled 5.0e-1 1.1e-1 1.1e-1 3.0e-2     aug2dc 3.7e+0 4.4e-1 4.4e-1 3.8e-2
      m-multiple-of-128 4.8e-1 5.3e-2 5.2e-2 1.9e-2   bilinear 3.2e+0 3.9e-1 4.0e-1 1.9e-2  sparse-terms 3.8e-1 7.9e-2 8.3e-2 2.8e-2
      hub 1.4e+0 7.3e-2 8.0e-2 2.8e-2"""
    data = cc.data(case)
    qp = data.qp
    x, xk = qp.x, qp.xhat
    v = np.random.default_rng(0).standard_normal(qp.n)
    ref = CoupledQuadRef(data, cc.SIGMA, 1.0, SE, 0.5, xk, keep_factors=True)
    sep = SepQuadRef(cc.without_terms(data), cc.SIGMA, 1.0, SE, 0.5, xk)
    e, e0 = ref.objgrad(x), sep.objgrad(x)
    H2, H1 = ref.hprod(x, v, 2), ref.hprod(x, v, 1)
    moved = {"gx": _rel(e0["gx"], e["gx"]), "Hv2": _rel(sep.hprod(x, v, 2), H2), "Hv1": _rel(sep.hprod(x, v, 1), H1)}
    print(f"\n{case}: " + " ".join(f"{k}={v_:.1e}" for k, v_ in moved.items()) + f" |Hv1-Hv2|={_rel(H1, H2):.1e}")
    for k, d in moved.items():
        assert d > 1e-3, (k, d)
    assert _rel(H1, H2) > 1e-6


def test_header_and_binding_declare_the_entry():
    src = open(os.path.join(ROOT, "include", "fpsq.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decl = re.search(r"\bint\s+fpsq_band_nlp_create_coupled\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert decl and len(decl.group(1).split(",")) == 12
    typed = {n: a for n, _, a in _lib.SYMBOLS}
    assert len(typed["fpsq_band_nlp_create_coupled"]) == 12
    cls = device_qp.DeviceBandCoupledQuadNLP
    assert issubclass(cls, device_qp.DeviceBandSepQuadNLP) and cls.nonlinear is True
    assert cls._model_entry == "fpsq_band_nlp_create_coupled" and cls._create_entry == "fpsq_band_create"
    params = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert params(cls.__init__) == params(device_qp.DeviceBandSepQuadNLP.__init__)
    for name in ("objgrad", "hprod", "cons"):
        assert getattr(cls, name) is getattr(device_qp.DeviceBandSepQuadNLP, name)
    assert issubclass(nlpmodels.CoupledQuadConModel, nlpmodels.SepQuadConModel)
    assert issubclass(problems.CoupledQuadNLP, problems.SepQuadNLP)
