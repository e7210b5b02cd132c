"""Every lane-group width and the second trip of the grid-stride loops of the banded evaluation kernels (k_bq_*, k_bqb_*,
k_bn_*): each case of tests/lane_group_cases.py -- whose docstring names, per WITH_LANE_GROUP site, the case that reaches each
width -- through every entry that dispatches on a lane group, on the linear model with a diagonal and with a sparse Hessian
(DeviceBandEqQP) and on the nonlinear model (DeviceBandSepQuadNLP).

The yardsticks are the exact restatements the older band tests use (oracle.exact_qp_objgrad / exact_qp_hprod,
tests/sparse_hessian_ref.py, tests/sepquad_ref.py, scipy for jac_mul) at the bars those tests hold the entries to:
max|a - b| / max|b| < 1e-9 per vector, |fx - fx_ref| <= 1e-9 |fx_ref|, jac_mul 1e-13; a column of a block entry against the
single-vector entry at the block tests' 1e-9.  On `thin` and `lg2` the gradient rows of the empty columns of A must equal
q_j x_j + d_j (+ eta (x_j - xk_j)) to the bit (each multiply-add rounded twice or fused): they receive no product term.  On
`stride` host and device arguments must give the same bits, fx included (its four sums come from the partials of capped grids).

MEASURED on the MI355X, worst relative error per model over every case, delta and (rho, eta) (the case it occurs on):
  linear, diagonal Hessian   gx 6.1e-14 (both-64)  ys 8.6e-14 (stride)  gs 6.0e-14 (both-64)  fx 1.2e-15 (both-64-shuffled)
                             Hv 4.1e-14 (wide-rows)  jac_mul A 7.5e-16 (ragged)  A' 6.7e-16 (stride)
    blocks, k = 1 and 11     HV 5.2e-14  GX 7.4e-14  GS 7.7e-14 (wide-rows)  YS 4.2e-14  P1 4.2e-14  Q1 5.5e-14  P2 4.0e-14
                             Q2 3.3e-14 (stride)  FX 1.8e-15 (both-64-shuffled); a column against the single entry <= 2.1e-15
  linear, sparse Hessian     gx 2.3e-14  ys 3.1e-14  gs 2.2e-14  fx 1.1e-15 (both-64)  Hv 4.4e-15 (lgT-8); blocks HV 7.7e-15
                             (lgT-16)  GX 3.0e-14  YS 3.5e-14  GS 3.1e-14  FX 1.3e-15 (both-64); on m-near-n the worst figure
                             is 2.6e-14 .. 2.9e-14 (ys) at every lgR
  nonlinear                  gx 8.3e-14  gs 8.1e-14  c 1.2e-14 (ragged-shuffled)  ys 7.0e-14 (stride)  fx 1.4e-15 (both-64)
                             Hv2 2.7e-14  Hv1 2.7e-14 (wide-rows)  jac_mul J 6.7e-16  J' 7.3e-16 (stride)
  per case, the worst of all its figures (linear / nonlinear): wide-rows 7.7e-14 / 3.0e-14, m-near-n 2.7e-14 / 1.5e-14,
  both-64 6.1e-14 / 3.9e-14, lgT-16 1.8e-14 / 3.1e-14, lgT-8 1.3e-14 / 1.5e-14, thin 2.1e-15 / 6.3e-15, lg2 1.9e-15 / 3.1e-15,
  ragged 5.9e-14 / 7.7e-14, stride 8.6e-14 / 7.0e-14, lg4-2 2.2e-15 / 4.0e-15, lg8-4 4.3e-15 / 1.4e-14,
  lg16-2 3.2e-15 / 4.6e-15, both-64-shuffled 3.9e-14 / 3.1e-14, ragged-shuffled 4.6e-14 / 8.3e-14.
No case failed: the kernels are right at every width.  Each test prints its figures (LANE-GROUPS lines, pytest -s).

THAT THE TESTS BITE: three arithmetic-only mutations of the kernels (no index, bound or launch changed), this file run on each:
  k_bn_epilogue, the shuffle loop started at LG / 4          -> test_nonlinear_model fails on the 12 cases with lgT >= 2
                                                                 (gx off by 0.9 .. 3.0 relative), passes on thin and lg2 (lgT = 1)
  k_bq_prologue, red[] zeroed at the top of every tile       -> test_linear_model_with_a_diagonal_hessian[stride] alone fails, in
                                                                 fx alone (3.1e-4; gx, ys, gs stay under 1e-13)
  k_bn_prologue, lanes l >= 32 scaled by 1 + 1e-6            -> test_nonlinear_model fails on wide-rows, both-64,
                                                                 both-64-shuffled and stride (lgA = 64; vectors off by ~1e-5)
and everything else passes under each."""
import fractions
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import fps_amd  # noqa: E402,F401
from fps_amd import nlpmodels  # noqa: E402
from fps_amd.device_qp import DeviceBandEqQP, DeviceBandSepQuadNLP  # noqa: E402
import lane_group_cases as L  # noqa: E402

pytestmark = pytest.mark.gpu

SE, SIGMA = L.SE, L.SIGMA
BAR, BAR_JAC = 1e-9, 1e-13
PAIRS = ((0.0, 0.0), (1.0, 0.5))          # (rho, eta)
KMAX = 11


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def _deltas(name):
    return (SE,) if name == "stride" else (0.0, SE)


def _ks(name):
    return (KMAX,) if name == "stride" else (1, KMAX)


def _report(name, what, errs):
    """one line per (case, entry group): the figures the summary of a run is made of"""
    print(f"\nLANE-GROUPS {name} {what}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))


def _hold(errs, bars=None):
    for k, v in errs.items():
        assert v < (bars or {}).get(k, BAR), (k, v)


def _objgrad(dev, x, xk, on=None):
    """one evaluation with every output; `on`: a torch device to run it on device tensors, None: numpy arrays"""
    qp = dev.qp
    if on is None:
        gx, ys, gs = np.empty(qp.n), np.empty(qp.m), np.empty(qp.n)
        fx, rc = dev.objgrad(x, gx=gx, ys=ys, gs=gs, xk=xk)
        return fx, rc, gx, ys, gs
    import torch

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(on)  # noqa: E731
    gx, ys, gs = (torch.empty(k, dtype=torch.float64, device=on) for k in (qp.n, qp.m, qp.n))
    fx, rc = dev.objgrad(t(x), gx=gx, ys=ys, gs=gs, xk=t(xk))
    return fx, rc, gx.cpu().numpy(), ys.cpu().numpy(), gs.cpu().numpy()


def _objgrad_errs(got, e):
    fx, rc, gx, ys, gs = got
    assert rc == 0
    errs = {"gx": _rel(gx, e["gx"]), "ys": _rel(ys, e["ys"]), "gs": _rel(gs, e["gs"]), "fx": abs(fx - e["fx"]) / abs(e["fx"])}
    assert abs(fx - e["fx"]) <= 1e-9 * abs(e["fx"]), errs
    return errs


def _info_as_pinned(dev, name):
    info = dev.info()
    for k, v in L.CASES[name].band.items():
        assert info[k] == v, (k, info)
    assert info["border_rows"] == 0 and info["border_cols"] == 0


def _fl(fr):
    return fr.numerator / fr.denominator   # (int / int is correctly rounded)


def _rows_without_a_product(qp, eta, xk):
    """{j: the fp64 values q_j x_j + d_j (+ eta (x_j - xk_j)) can take} for the empty columns j of A: each multiply-add either
    rounded twice or fused, nothing else -- such a row receives no term of a product, and a sum over NO entries is exact"""
    F = fractions.Fraction
    cols = np.flatnonzero(np.bincount(qp.colind, minlength=qp.n) == 0)
    out = {}
    for j in cols:
        q, x, d = float(qp.qdiag[j]), float(qp.x[j]), float(qp.d[j])
        g = {q * x + d, _fl(F(q) * F(x) + F(d))}
        if eta > 0.0:
            dx = x - float(xk[j])
            g = {v for u in g for v in (u + eta * dx, _fl(F(u) + F(eta) * F(dx)))}
        out[int(j)] = g
    return out


def _check_rows_without_a_product(name, qp, gx, gs, eta, xk):
    want_gs, want_gx = _rows_without_a_product(qp, 0.0, None), _rows_without_a_product(qp, eta, xk)
    assert len(want_gs) == L.CASES[name].cols[0] > 100
    for j in want_gs:
        assert float(gs[j]) in want_gs[j], (j, gs[j], want_gs[j])
        assert float(gx[j]) in want_gx[j], (j, gx[j], want_gx[j])


@pytest.mark.parametrize("name", L.NAMES)
def test_linear_model_with_a_diagonal_hessian(oracle, name):
    """DeviceBandEqQP on every case: objgrad, hprod, jac_mul and the three block entries.  The single-vector entries go
    against oracle.exact_qp_objgrad / exact_qp_hprod -- on `stride` against the same formulae on ONE kept factor of K
    (lane_group_cases.exact_linear), as do the columns of the block entries everywhere."""
    qp = L.qp(name)
    x, xk = qp.x, qp.xhat
    A = qp.scipy_csr()
    rng = np.random.default_rng(0)
    v, u = rng.standard_normal(qp.n), rng.standard_normal(qp.m)
    dev = DeviceBandEqQP(qp, sigma=SIGMA, rho=0.0, delta=_deltas(name)[0], eta=0.0)
    _info_as_pinned(dev, name)
    for delta in _deltas(name):
        dev.set_delta(delta)
        ref = L.exact_linear(name, delta)
        for rho, eta in PAIRS:
            dev.rho, dev.eta = rho, eta
            got = _objgrad(dev, x, xk)
            e = ref.objgrad(x, SIGMA, rho, eta, xk) if name == "stride" else oracle.exact_qp_objgrad(qp, x, SIGMA, rho, delta, eta,
                                                                                                  xk)
            errs = _objgrad_errs(got, e)
            Hv2, Hv1 = np.empty(qp.n), np.empty(qp.n)
            assert dev.hprod(v, Hv2, 2) == 0 and dev.hprod(v, Hv1, 1) == 0
            errs["Hv"] = _rel(Hv2, ref.hprod(v, SIGMA, rho, eta) if name == "stride" else
                              oracle.exact_qp_hprod(qp, v, SIGMA, rho, delta, eta))
            _report(name, f"linear delta={delta:.1e} rho={rho} eta={eta}", errs)
            _hold(errs)
            assert np.array_equal(Hv1, Hv2)
            if name in ("thin", "lg2"):
                _check_rows_without_a_product(name, qp, got[2], got[4], eta, xk)
    assert dev.info()["factorizations"] == len(_deltas(name))
    # y = alpha op(A) x + beta y: lane_group(nnz, m) lanes for A, lane_group(nnz, n) for A'
    y0, z0 = rng.standard_normal(qp.m), rng.standard_normal(qp.n)
    y, z = y0.copy(), z0.copy()
    assert dev.jac_mul(0, -0.5, x, 2.0, y) == 0 and dev.jac_mul(1, -0.5, u, 2.0, z) == 0
    errs = {"A": _rel(y, -0.5 * (A @ x) + 2.0 * y0), "At": _rel(z, -0.5 * (A.T @ u) + 2.0 * z0)}
    _report(name, "linear jac_mul", errs)
    _hold(errs, {"A": BAR_JAC, "At": BAR_JAC})
    if name == "stride":   # all four partial sums live, over capped grids: host arguments against device arguments
        import torch

        host, devt = _objgrad(dev, x, xk), _objgrad(dev, x, xk, on=torch.device("cuda", 0))
        for a, b in zip(host, devt):
            assert np.array_equal(a, b)
    _block_entries(dev, name, L.exact_linear(name, SE), "linear")
    dev.close()


def _block_entries(dev, name, ref, what):
    """hprod_block, objgrad_block and solve_two_least_squares_block on a handle at delta = sqrt(eps), (rho, eta) = (1, 0.5):
    every column against the exact evaluation of that column, and against the single-vector entry where there is one"""
    qp = dev.qp
    rho, eta = dev.rho, dev.eta
    rng = np.random.default_rng(4321)
    V, X, XK, D = (rng.standard_normal((KMAX, qp.n)) for _ in range(4))
    B = rng.standard_normal((KMAX, qp.m))
    for k in _ks(name):
        HV = np.full((k, qp.n), np.nan)
        assert dev.hprod_block(np.ascontiguousarray(V[:k]), HV, 2) == 0
        single = np.empty(qp.n)
        errs = {"HV": 0.0, "HV-single": 0.0}
        for j in range(k):
            assert dev.hprod(V[j], single, 2) == 0
            errs["HV"] = max(errs["HV"], _rel(HV[j], ref.hprod(V[j], SIGMA, rho, eta)))
            errs["HV-single"] = max(errs["HV-single"], _rel(HV[j], single))
        # k = 11: the linear term and the right-hand side of each column its own; k = 1: the model's
        own = k == 1
        args = dict(XK=np.ascontiguousarray(XK[:k]), D=None if own else np.ascontiguousarray(D[:k]),
                    B=None if own else np.ascontiguousarray(B[:k]))
        GX, YS, GS = np.full((k, qp.n), np.nan), np.full((k, qp.m), np.nan), np.full((k, qp.n), np.nan)
        fx, rc = dev.objgrad_block(np.ascontiguousarray(X[:k]), GX=GX, YS=YS, GS=GS, **args)
        assert rc == 0 and fx.shape == (k,)
        worst = {"GX": 0.0, "YS": 0.0, "GS": 0.0, "FX": 0.0}
        for j in range(k):
            e = (ref if own else L.exact_linear_with(ref, D[j], B[j])).objgrad(X[j], SIGMA, rho, eta, XK[j])
            col = _objgrad_errs((fx[j], 0, GX[j], YS[j], GS[j]), e)
            worst = {a: max(worst[a], col[a.lower()]) for a in worst}
        errs.update(worst)
        if own:   # the single entry evaluates the model's own d and b
            sfx, src, sgx, sys_, sgs = _objgrad(dev, X[0], XK[0])
            errs.update({"GX-single": _rel(GX[0], sgx), "YS-single": _rel(YS[0], sys_), "GS-single": _rel(GS[0], sgs),
                         "FX-single": abs(fx[0] - sfx) / abs(sfx)})
        if not qp.has_sparse_hessian:
            P1, P2 = np.full((k, qp.n), np.nan), np.full((k, qp.n), np.nan)
            Q1, Q2 = np.full((k, qp.m), np.nan), np.full((k, qp.m), np.nan)
            assert dev.solve_two_least_squares_block(np.ascontiguousarray(V[:k]), np.ascontiguousarray(X[:k]), p1=P1, q1=Q1,
                                                     p2=P2, q2=Q2) == 0
            zero = np.zeros(qp.m)
            for j in range(k):
                (p1, q1), (p2, q2) = ref._solve(V[j], zero), ref._solve(X[j], zero)
                for a, got, want in (("P1", P1, p1), ("Q1", Q1, q1), ("P2", P2, p2), ("Q2", Q2, q2)):
                    errs[a] = max(errs.get(a, 0.0), _rel(got[j], want))
        _report(name, f"{what} blocks k={k}", errs)
        _hold(errs)


@pytest.mark.parametrize("base,hw", list(L.HESS_CASES), ids=[f"{b}-hw{h}" for b, h in L.HESS_CASES])
def test_linear_model_with_a_sparse_hessian(base, hw):
    """The rows of R = Q - diag(Q) at every lane-group width (k_bq_pack_sq, k_bq_jacmul on R and their block forms) on
    `m-near-n`, and the Hessian forms of the A and A' kernels (k_bq_epilogue_sq, the block kernels' flags) at every width of
    theirs, against tests/sparse_hessian_ref.py."""
    qp = L.hess_qp(base, hw)
    lgr = L.HESS_CASES[base, hw]
    assert L.hessian_lanes(qp) == lgr
    name = f"{base}/hw{hw}-lgR{lgr}"
    x, xk = qp.x, qp.xhat
    v = np.random.default_rng(0).standard_normal(qp.n)
    dev = DeviceBandEqQP(qp, sigma=SIGMA, rho=0.0, delta=0.0, eta=0.0)
    _info_as_pinned(dev, base)
    for delta in (0.0, SE):
        dev.set_delta(delta)
        ref = L.exact_linear(base, delta, hw)
        for rho, eta in PAIRS:
            dev.rho, dev.eta = rho, eta
            errs = _objgrad_errs(_objgrad(dev, x, xk), ref.objgrad(x, SIGMA, rho, eta, xk))
            Hv2, Hv1 = np.empty(qp.n), np.empty(qp.n)
            assert dev.hprod(v, Hv2, 2) == 0 and dev.hprod(v, Hv1, 1) == 0
            errs["Hv"] = _rel(Hv2, ref.hprod(v, SIGMA, rho, eta))
            _report(name, f"sparse-hessian delta={delta:.1e} rho={rho} eta={eta}", errs)
            _hold(errs)
            assert np.array_equal(Hv1, Hv2)
    assert dev.info()["factorizations"] == 2
    _block_entries(dev, name, L.exact_linear(base, SE, hw), "sparse-hessian")
    dev.close()


@pytest.mark.parametrize("name", L.NAMES)
def test_nonlinear_model(name):
    """DeviceBandSepQuadNLP on every case: cons, objgrad, hprod Val(2) and Val(1) against tests/sepquad_ref.py (its factors
    kept: lane_group_cases.exact_nonlinear), jac_mul against J(x) afterwards, one factorisation per objgrad."""
    qp, data = L.qp(name), L.nlp_data(name)
    x, xk = qp.x, qp.xhat
    rng = np.random.default_rng(0)
    v, u = rng.standard_normal(qp.n), rng.standard_normal(qp.m)
    dev = DeviceBandSepQuadNLP(data, sigma=SIGMA, rho=0.0, delta=_deltas(name)[0], eta=0.0)
    _info_as_pinned(dev, name)
    c = np.empty(qp.m)
    assert dev.cons(x, c) == 0
    nobj = 0
    for delta in _deltas(name):
        dev.set_delta(delta)
        ref = L.exact_nonlinear(name, delta)
        for rho, eta in PAIRS:
            dev.rho, dev.eta = rho, eta
            ref.pen.rho, ref.pen.eta = rho, eta
            got = _objgrad(dev, x, xk)
            nobj += 1
            e = ref.objgrad(x)
            errs = _objgrad_errs(got, e)
            errs["c"] = _rel(c, e["c"])
            Hv2, Hv1 = np.empty(qp.n), np.empty(qp.n)
            assert dev.hprod(v, Hv2, 2) == 0 and dev.hprod(v, Hv1, 1) == 0
            errs["Hv2"] = _rel(Hv2, ref.hprod(x, v, 2))
            errs["Hv1"] = _rel(Hv1, ref.hprod(x, v, 1))
            _report(name, f"nonlinear delta={delta:.1e} rho={rho} eta={eta}", errs)
            _hold(errs)
            assert _rel(Hv1, Hv2) > 1e-6          # the terms that vanish on the linear model are live
            if name in ("thin", "lg2"):
                _check_rows_without_a_product(name, qp, got[2], got[4], eta, xk)
        ref.pen.rho, ref.pen.eta = 0.0, 0.0
    assert dev.info()["factorizations"] == nobj
    # the handle's values are J(x) now
    J = nlpmodels.SepQuadConModel(data)._J(x)
    y0, z0 = rng.standard_normal(qp.m), rng.standard_normal(qp.n)
    y, z = y0.copy(), z0.copy()
    assert dev.jac_mul(0, -0.5, v, 2.0, y) == 0 and dev.jac_mul(1, -0.5, u, 2.0, z) == 0
    errs = {"J": _rel(y, -0.5 * (J @ v) + 2.0 * y0), "Jt": _rel(z, -0.5 * (J.T @ u) + 2.0 * z0)}
    _report(name, "nonlinear jac_mul", errs)
    _hold(errs, {"J": BAR_JAC, "Jt": BAR_JAC})
    if name == "stride":
        import torch

        on = torch.device("cuda", 0)
        host, devt = _objgrad(dev, x, xk), _objgrad(dev, x, xk, on=on)
        for a, b in zip(host, devt):
            assert np.array_equal(a, b)
        cd = torch.empty(qp.m, dtype=torch.float64, device=on)
        assert dev.cons(torch.from_numpy(x.copy()).to(on), cd) == 0
        assert np.array_equal(cd.cpu().numpy(), c)
        assert dev.info()["factorizations"] == nobj + 2
    dev.close()
