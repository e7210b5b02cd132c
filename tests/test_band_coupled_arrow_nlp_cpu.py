"""Coupling terms on bordered and arrow band handles (fpsq_band_nlp_create_coupled_arrow, DeviceArrowBandCoupledQuadNLP) as far as
they can be checked without a GPU: the declarations, the generator of the real model (problems.free_final_time_like), the
cases of tests/coupled_arrow_cases.py (their term counts, what the symbolic phase makes of them, and that the terms the plain
coupled entry cannot state matter on each), the numpy restatement of the new lists and sums (tests/coupled_arrow_nlp_model.py)
against the yardstick tests/coupled_quad_ref.py, and the extended host builder of csrc/fpsq_coupled.h through the stand-alone
tests/host/coupled_arrow_check.cpp, plain and under the address / undefined-behaviour sanitizers."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import fps_amd  # noqa: E402,F401
import coupled_arrow_cases as ca  # noqa: E402
from coupled_arrow_nlp_model import CoupledArrowNLPModel  # noqa: E402
from coupled_nlp_model import CoupledNLPModel  # noqa: E402
from coupled_quad_ref import CoupledQuadRef  # noqa: E402
from fps_amd import _lib, device_qp, nlpmodels, problems, qdsolver  # noqa: E402
from test_band_coupled_nlp_cpu import _by_first_column, _compiler, _flat  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SE = ca.SE
# The restatement against the yardstick: both are exact up to rounding (sparse LU solves of the same KKT system), so they agree
# to a small multiple of eps times the conditioning of K; 1e-12 is three decades under the device's 1e-9 bar, the margin
# tests/test_lane_groups_cpu.py holds the yardstick's own residual to.
BAR_RESTATEMENT = 1e-12


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def test_header_binding_and_class_declare_the_entry():
    src = open(os.path.join(ROOT, "include", "fpsq.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    new = re.search(r"\bint\s+fpsq_band_nlp_create_coupled_arrow\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    old = re.search(r"\bint\s+fpsq_band_nlp_create_coupled\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    squeeze = lambda s: re.sub(r"\s+", " ", s).strip()  # noqa: E731
    assert new and old and squeeze(new.group(1)) == squeeze(old.group(1))           # the parameter list of the coupled entry
    typed = {n: a for n, _, a in _lib.SYMBOLS}
    assert typed["fpsq_band_nlp_create_coupled_arrow"] == typed["fpsq_band_nlp_create_coupled"]
    cls = device_qp.DeviceArrowBandCoupledQuadNLP
    assert issubclass(cls, device_qp.DeviceBandCoupledQuadNLP) and cls.nonlinear is True
    assert cls._model_entry == "fpsq_band_nlp_create_coupled_arrow" and cls._create_entry == "fpsq_band_create_arrow"
    params = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert params(cls.__init__) == params(device_qp.DeviceArrowBandSepQuadNLP.__init__)
    for name in ("objgrad", "hprod", "cons", "jac_mul", "_model_extra"):
        assert getattr(cls, name) is getattr(device_qp.DeviceBandCoupledQuadNLP, name)
    text = re.sub(r"//.*", "", open(os.path.join(ROOT, "fletcherpenaltysolver.jl_amd", "csrc", "fpsq_coupled.h")).read()).lower()
    for word in ("hip", "dalloc", "getenv"):                    # the lists stay plain host code
        assert word not in text, word


def test_the_free_final_time_generator():
    N, tau, a, beta = 40, 0.25, 1.0, 1.0
    d = problems.free_final_time_like(N, tau=tau, a=a, beta=beta)
    q = d.qp
    th = q.n - 1
    assert (q.n, q.m, q.nnz, d.nterms) == (2 * N + 2, N + 1, 5 * N, 2 * N)
    k = np.arange(N)
    assert np.array_equal(np.diff(q.rowptr), np.concatenate([np.full(N, 4), [N]]))
    body = q.colind[:4 * N].reshape(N, 4)
    assert np.array_equal(body, np.stack([2 * k, 2 * k + 1, 2 * k + 2, np.full(N, th)], axis=1))
    assert np.array_equal(q.vals[:4 * N].reshape(N, 4), np.tile([-1.0, 0.0, 1.0, 0.0], (N, 1)))     # explicit zeros under the terms
    assert np.array_equal(q.colind[4 * N:], 2 * k + 1) and np.all(q.vals[4 * N:] == 0.0)
    assert np.all(d.hvals[:4 * N] == 0.0) and np.all(d.hvals[4 * N:] == 1.0 / N)                  # curvature in the long row
    terms = set(zip(d.t_row.tolist(), d.t_j.tolist(), d.t_k.tolist(), d.t_w.tolist()))
    assert terms == {(i, 2 * i, th, tau * a) for i in range(N)} | {(i, 2 * i + 1, th, -tau * beta) for i in range(N)}
    nlp = nlpmodels.CoupledQuadConModel(d)
    assert np.abs(nlp.cons(q.xhat)).max() < 1e-13
    x = q.x
    y, u, theta = x[0:th:2], x[1:th:2], x[th]
    want = np.concatenate([y[1:] - y[:-1] + tau * theta * (a * y[:-1] - beta * u), [np.sum(u * u) / (2 * N)]]) - d.b
    assert np.allclose(nlp.cons(x), want, rtol=0, atol=1e-14)
    assert q.qdiag[th] == 1.0 and q.d[th] == -1.0 and 0.8 < q.xhat[th] < 1.2                      # (theta - theta_hat)^2
    # the symbolic phase: at N = 2000 the arrow keeps the band at one block where the plain band needs many
    big = problems.free_final_time_like(2000).qp
    arrow = qdsolver.band_analysis_arrow(nlpmodels.EqQPModel(big), border=16, cols=16)
    plain = qdsolver.band_analysis_arrow(nlpmodels.EqQPModel(big), border=0, cols=0)
    print(f"\nfree_final_time_like(2000): arrow {arrow}\n plain {plain}")
    assert (arrow["border_rows"], arrow["border_cols"], arrow["bandwidth_blocks"]) == (1, 1, 1)
    assert (plain["border_rows"], plain["border_cols"]) == (0, 0) and plain["bandwidth_blocks"] > 8


@pytest.mark.parametrize("name", ca.NAMES)
def test_the_cases_are_what_their_table_says(name):
    d, rows, cols = ca.problem(name)
    assert ca.counts(name) == ca.COUNTS[name]
    border, ncols = ca.limits(name)
    info = qdsolver.band_analysis_arrow(nlpmodels.EqQPModel(d.qp), border=border, cols=ncols)
    for key, want in ca.want_info(name).items():
        assert info[key] == want, (key, info)
    assert (info["border_rows"], info["border_cols"]) == (rows.size, cols.size)
    assert np.abs(nlpmodels.CoupledQuadConModel(d).cons(d.qp.xhat)).max() < 1e-12


@pytest.mark.parametrize("name", ca.NAMES)
def test_the_terms_the_plain_entry_cannot_state_matter(name):
    """Dropping ONLY the terms that touch a long column or lie in a border row moves the reference gx and Hv Val(2) by more than
    1e-3 relative on every case (measured 2.4e-2 .. 2.3e-1 and 3.7e-3 .. 3.0e-1), at (rho, eta) = (1, 0.5): the 1e-9 bar of the
    GPU tests tells the two models apart."""
    d, _, _ = ca.problem(name)
    qp = d.qp
    e = ca.expected(name)[(1.0, 0.5)]
    less = ca.without_special_terms(name)
    assert less.nterms < d.nterms
    # (b stays: the same constraint functions minus the terms, evaluated at the same point)
    ref = CoupledQuadRef(less, ca.SIGMA, 1.0, ca.delta(name), 0.5, qp.xhat, keep_factors=True)
    moved = {"gx": _rel(ref.objgrad(qp.x)["gx"], e["gx"]), "Hv2": _rel(ref.hprod(qp.x, ca.v_of(qp), 2), e["Hv2"])}
    print(f"\n{name}: " + " ".join(f"{k}={v:.1e}" for k, v in moved.items()))
    assert moved["gx"] > 1e-3 and moved["Hv2"] > 1e-3


@pytest.mark.parametrize("name", ca.NAMES)
def test_the_restated_lists_and_sums_agree_with_the_yardstick(name):
    """tests/coupled_arrow_nlp_model.py on the case's long columns -- the split S, the long-row sums, the virtual transposed
    entries -- against tests/coupled_quad_ref.py; and without the long-row sums it misses wherever a long row has an entry."""
    d, rows, cols = ca.problem(name)
    qp = d.qp
    x, xk, v = qp.x, qp.xhat, ca.v_of(qp)
    rperm = _by_first_column(qp) if name == "m1500-r1-c1-shuffled" else None
    mdl = CoupledArrowNLPModel(d, cols, rperm)
    A = mdl.A
    # the lists: the long columns' rows are empty in the CSR and stand behind it, in order; together they are S
    nb = int(A["srp"][-1])
    assert all(A["srp"][c] == A["srp"][c + 1] for c in cols) and A["lrp"][0] == nb and A["lrp"][-1] == A["sci"].size
    assert A["sci"].size == len(A["contrib"]) and sum(len(c) for c in A["contrib"]) == 2 * d.nterms
    long_len = np.diff(A["lrp"])
    assert (long_len.max() if cols.size else 0) == (ca.COUNTS[name][4] if ca.COUNTS[name][1] else 0)
    if name == "m640-r3-c5-param":
        assert np.count_nonzero(long_len == 0) == 4             # long columns without terms
    tv = mdl.dev_tvals(x)
    virtual = mdl.dev_t_perm == mdl.ci.size
    assert np.count_nonzero(virtual) == 3 * cols.size and np.all(tv[virtual] == 1.0)
    assert np.array_equal(tv[~virtual], mdl.vals(x)[mdl.dev_t_perm[~virtual]])
    delta = ca.delta(name)
    for rho, eta in ca.RHO_ETA:
        e = ca.expected(name)[(rho, eta)]
        a = mdl.objgrad(x, ca.SIGMA, rho, delta, eta, xk)
        errs = {k: _rel(a[k], e[k]) for k in ("gx", "ys", "gs", "c")}
        errs["fx"] = abs(a["fx"] - e["fx"]) / abs(e["fx"])
        errs["cons"] = _rel(mdl.cons(x), e["c"])
        errs["Hv2"] = _rel(mdl.hprod(v, ca.SIGMA, rho, eta, 2), e["Hv2"])
        if delta > 0.0:      # (at delta = 0 the yardstick's Val(1) solves with tau = 1e-14, the restatement with 0)
            errs["Hv1"] = _rel(mdl.hprod(v, ca.SIGMA, rho, eta, 1), e["Hv1"])
        if cols.size:
            errs.update({f"{k}[L]": _rel(a[k][cols], e[k][cols]) for k in ("gx", "gs")})
        print(f"\n{name} rho={rho} eta={eta}: " + " ".join(f"{k}={v_:.1e}" for k, v_ in errs.items()))
        for k, err in errs.items():
            assert err < BAR_RESTATEMENT, (k, err)
    if long_len.sum() > 0:
        broken = CoupledArrowNLPModel(d, cols, rperm, long_rows=False)
        got = broken.objgrad(x, ca.SIGMA, 1.0, delta, 0.5, xk)["gx"]
        assert _rel(got[cols], e["gx"][cols]) > 1e-9


def _arrow_input():
    """a small pattern with three long columns: the last is coupled to the first entry of every row (with_coupled_constraints),
    the second and the third are coupled to each other in every row (a term between two long columns), the first has no term"""
    base = problems.with_long_columns(problems.pde_control_like(n=300, m=60, per_row=8, window=64, seed=3), 3)
    d = problems.with_coupled_constraints(base, 0.3, 3, 7)
    m, n = base.m, base.n
    rows = np.arange(m, dtype=np.int32)
    cat = lambda a, b: np.concatenate([a, np.asarray(b, dtype=a.dtype)])  # noqa: E731
    return problems._coupled(base, d.hvals, cat(d.t_row, rows), cat(d.t_j, np.full(m, n - 2)), cat(d.t_k, np.full(m, n - 1)),
                             cat(d.t_w, 0.05 * (1.0 + rows % 3))), np.array([n - 3, n - 2, n - 1])


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_the_extended_host_builder_gives_the_lists_of_its_restatement(tmp_path, flags):
    """coupled_build with the list of long columns through tests/host/coupled_arrow_check.cpp (its own main; no GPU, nothing
    loaded into Python) against coupled_arrow_nlp_model.build_lists_arrow, entry by entry: a transposed structure with virtual
    entries, a long column without terms, a term between two long columns, a stored row order of its own.  Without the list
    (nlong = 0) the same input gives the unsplit S of tests/coupled_nlp_model.py."""
    inc = os.path.join(ROOT, "fletcherpenaltysolver.jl_amd", "csrc")
    exe = str(tmp_path / "coupled_arrow_check")
    build = subprocess.run([_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", inc, "-o", exe,
                            os.path.join(ROOT, "tests", "host", "coupled_arrow_check.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    data, lcols = _arrow_input()
    qp = data.qp
    mdl = CoupledArrowNLPModel(data, lcols, _by_first_column(qp), vgrid=2)
    both = (np.isin(data.t_j, lcols) & np.isin(data.t_k, lcols)).sum()
    assert both == qp.m and not np.isin(lcols[0], np.concatenate([data.t_j, data.t_k]))
    assert np.count_nonzero(mdl.dev_t_perm == qp.nnz) == 2 * lcols.size

    def run(cols, t_row, t_j, t_k, t_w):
        rinv = np.empty(qp.m, dtype=np.int64)
        rinv[mdl.rperm] = np.arange(qp.m)
        path = tmp_path / "problem.txt"
        with open(path, "w") as f:
            f.write(f"{qp.n} {qp.m} {mdl.dev_t_perm.size} {len(t_w)} {len(cols)}\n")
            for a in (mdl.rp, mdl.ci, rinv, mdl.dev_t_perm, cols):
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

    terms = (data.t_row, data.t_j, data.t_k, data.t_w)
    got = run(lcols, *terms)
    A = mdl.A
    want = dict(zip(("pptr", "pcol", "pw"), _flat(A["partners"])))
    want.update(zip(("tpptr", "tpcol", "tpw"), _flat(A["t_partners"])))
    want.update(zip(("cptr", "crow", "cw"), _flat(A["contrib"])))
    want.update(tcol=A["tcol"], srp=A["srp"], sci=A["sci"], lrp=A["lrp"])
    assert set(got) == set(want)
    for name, w in want.items():
        assert np.array_equal(got[name], np.asarray(w, dtype=float)), name
    firsts = np.unique(qp.colind[qp.rowptr[:-1]]).size            # (rows that share their first column share the entry of S)
    assert np.diff(A["lrp"]).tolist() == [0, 1, firsts + 1]       # no term; the third column; the second and every row's first
    assert max(len(c) for c in A["contrib"]) == qp.m              # the entry between the two long columns: every row contributes
    # without the list: S whole (the parent's lists on the real entries), the virtual entries still empty
    plain = run([], *terms)
    L = CoupledNLPModel(data, _by_first_column(qp)).L
    assert np.array_equal(plain["srp"], L["srp"]) and np.array_equal(plain["sci"], L["sci"])
    assert np.array_equal(plain["cptr"], _flat(L["contrib"])[0]) and plain["lrp"].tolist() == [float(L["sci"].size)]
    assert np.array_equal(plain["tpptr"], got["tpptr"]) and np.array_equal(plain["tcol"], got["tcol"])
    # the checks stay, and a list of long columns that does not ascend is refused
    row0 = mdl.ci[mdl.rp[0]:mdl.rp[1]]
    r0 = int(mdl.rperm[0])
    msg = run(lcols, [r0], [int(row0[0])], [int(row0[0])], [0.1])
    assert isinstance(msg, str) and "j = k" in msg
    msg = run(lcols[::-1], *terms)
    assert isinstance(msg, str) and "ascending" in msg
    assert isinstance(run(lcols, [], [], [], []), dict)            # no terms: empty lists, no error
