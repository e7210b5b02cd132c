"""Long Jacobian columns on the banded back-end (fpsq_band_create_bordered_cols, DeviceBorderedBandEqQP(cols=...)): a few
columns that touch rows all over the range are taken out of the band, M = A A' + delta I = B + U U', and every M-solve is the
sweeps on the band B plus the correction w = S^-1 (U'y), u = y - Z w (include/fpsq.h "LONG COLUMNS").

Yardstick: a DENSE fp64 solve of K = [I A'; A -delta I] (scipy.linalg.lu_factor, once per shape, shared) and the closed forms
of objgrad / hprod of include/fpsq.h (tests/sparse_hessian_ref.py, on that dense factor), at the bar the existing banded tests
hold each entry to: max|a - b| / max|b| < 1e-9 per vector, |phi - phi_exact| <= 1e-9 |phi_exact|, 1e-13 for A x / A'y (the
rows of the long columns included).  A numpy model of the scheme (tests/long_columns_model.py) loses 2e-15 .. 6e-14 on these
shapes, so the bars leave four digits: a case that needs more is a defect.  Every call must return 0.

Shapes: the band parts of tests/test_gpu_band_border.py, the smallest at which a border can exist at all (the rule needs >= 5
blocks, two chains need m >= 2560); s = 1, 5, 16 columns of either kind; delta = 0 and sqrt(eps); long columns last, first and
in the middle of the caller's column order; all rows shuffled (reverse Cuthill-McKee on the band rows)."""
import ctypes as C
import dataclasses
import functools
import os
import sys

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(__file__))
import fps_amd  # noqa: E402,F401
import conditioning_cases as cc  # noqa: E402
import kkt_truth as kt  # noqa: E402
from fps_amd import _lib, problems  # noqa: E402
from fps_amd.device_qp import DeviceBorderedBandEqQP  # noqa: E402
from long_columns_model import LongColumnsModel  # noqa: E402
from sparse_hessian_ref import SparseHessianRef  # noqa: E402

pytestmark = pytest.mark.gpu

SE = float(np.sqrt(np.finfo(float).eps))
SIGMA = 1e3
BAR = 1e-9


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def _columns_moved(qp, new_of_old):
    """column c of qp becomes column new_of_old[c]"""
    A = qp.scipy_csr().tocoo()
    B = sp.csr_matrix((A.data, (A.row, new_of_old[A.col])), shape=A.shape)
    B.sort_indices()
    inv = np.argsort(new_of_old)
    return dataclasses.replace(qp, rowptr=B.indptr.astype(np.int32), colind=B.indices.astype(np.int32), vals=B.data.copy(),
                               qdiag=qp.qdiag[inv], d=qp.d[inv], xhat=qp.xhat[inv], x=qp.x[inv])


def _rows_shuffled(qp, seed):
    order = np.random.default_rng(seed).permutation(qp.m)
    A = sp.csr_matrix(qp.scipy_csr()[order])
    A.sort_indices()
    return dataclasses.replace(qp, rowptr=A.indptr.astype(np.int32), colind=A.indices.astype(np.int32), vals=A.data.copy(),
                               b=qp.b[order])


def _placed(qp0, s, kind, where, shuffle, seed=9):
    """qp0 with s long columns; `where` they sit in the caller's column order.  Returns (qp, indices of the long columns)"""
    qp = problems.with_long_columns(qp0, s, kind=kind, seed=seed)
    n0 = qp0.n
    at = {"last": n0, "first": 0, "middle": n0 // 2}[where]
    if where != "last":
        qp = _columns_moved(qp, np.concatenate([np.arange(at), np.arange(at + s, qp.n), at + np.arange(s)]))
    if shuffle:
        qp = _rows_shuffled(qp, seed)
    return qp, at + np.arange(s)


def _p640():
    return problems.pde_control_like(n=3000, m=640, per_row=12, window=256, seed=5)


def _p1500():
    return problems.pde_control_like(n=3600, m=1500, per_row=12, window=256, seed=6)


# name: (band part, s, kind, where, rows shuffled, delta, expected info of the handle)
CASES = {
    "m640-s5-param-delta0": (_p640, 5, "param", "last", False, 0.0, {"nblocks": 5, "chains": 1}),
    "m640-s16-stride-first": (_p640, 16, "stride", "first", False, SE, {"nblocks": 5, "chains": 1}),
    "m1500-s1-middle": (_p1500, 1, "param", "middle", False, SE, {"nblocks": 12, "chains": 1}),
    # (all rows shuffled: the natural band of the 1500 rows is full, 11 blocks; 2 only after reverse Cuthill-McKee)
    "m1500-s5-stride-shuffled-delta0": (_p1500, 5, "stride", "last", True, 0.0,
                                        {"nblocks": 12, "chains": 1, "bandwidth_blocks": 2, "reordered": 1}),
    "aug2dc-two-chains-s16-param": (lambda: problems.aug2dc_like(N=51), 16, "param", "last", False, SE,
                                    {"nblocks": 21, "chains": 2}),
}
KMAX = 9


@functools.lru_cache(maxsize=None)
def _qp(case, model="diag"):
    make, s, kind, where, shuffle, _, _ = CASES[case]
    qp, cols = _placed(make(), s, kind, where, shuffle)
    if model != "diag":
        qp = problems.with_sparse_hessian(qp, 2, 11)
    return qp, cols


class DenseRef(SparseHessianRef):
    """the closed forms of tests/sparse_hessian_ref.py on a DENSE LU factorisation of K = [I A'; A -delta I]"""

    def __init__(self, qp, lu):
        self.qp, self.n, self.m = qp, qp.n, qp.m
        self.A = qp.scipy_csr()
        self.Q = qp.hess_csr()
        self._dense = lu

    def _solve(self, top, bottom):
        sol = sla.lu_solve(self._dense, np.concatenate([top, bottom]))
        return sol[:self.n], sol[self.n:]


def _dense_lu_of(qp, delta):
    A = qp.scipy_csr().toarray()
    K = np.block([[np.eye(qp.n), A.T], [A, -float(delta) * np.eye(qp.m)]])
    return sla.lu_factor(K, overwrite_a=True, check_finite=False)


@functools.lru_cache(maxsize=None)
def _dense_lu(case):
    return _dense_lu_of(_qp(case)[0], CASES[case][5])


def _ref(case, model="diag"):
    return DenseRef(_qp(case, model)[0], _dense_lu(case))


@functools.lru_cache(maxsize=None)
def _blocks(case):
    qp, _ = _qp(case)
    rng = np.random.default_rng(1234)
    V, W = rng.standard_normal((KMAX, qp.n)), rng.standard_normal((KMAX, qp.n))
    V.setflags(write=False)
    W.setflags(write=False)
    return V, W


def _device(case, model="diag", rho=1.0, eta=0.5, cols=16, **kw):
    qp, _ = _qp(case, model)
    dev = DeviceBorderedBandEqQP(qp, border=0, cols=cols, sigma=SIGMA, rho=rho, delta=CASES[case][5], eta=eta, **kw)
    info = dev.info()
    assert info["border_rows"] == 0
    if cols:
        assert info["border_cols"] == CASES[case][1], info
        for k, v in CASES[case][6].items():
            assert info[k] == v, (k, info)
    else:
        assert info["border_cols"] == 0
    return dev


def _objgrad(dev, x, xk):
    qp = dev.qp
    gx, ys, gs = np.full(qp.n, np.nan), np.full(qp.m, np.nan), np.full(qp.n, np.nan)
    fx, rc = dev.objgrad(x, gx=gx, ys=ys, gs=gs, xk=xk)
    assert rc == 0
    return fx, gx, ys, gs


def _two_on(lib, h, qp, name, rhs1, rhs2):
    p1, q1, p2, q2 = np.full(qp.n, np.nan), np.full(qp.m, np.nan), np.full(qp.n, np.nan), np.full(qp.m, np.nan)
    rc = getattr(lib, f"fpsq_band_{name}")(h, rhs1.ctypes.data, rhs2.ctypes.data, p1.ctypes.data, q1.ctypes.data,
                                           p2.ctypes.data, q2.ctypes.data)
    assert rc == 0, lib.fpsq_band_last_error(h)
    return p1, q1, p2, q2


def _two(dev, name, rhs1, rhs2):
    """fpsq_band_solve_two_mixed / _least_squares on the object's handle"""
    assert dev._factor() == 0
    return _two_on(dev._lib, dev._h, dev.qp, name, rhs1, rhs2)


def _hprod_block(dev, V):
    HV = np.full(V.shape, np.nan)
    assert dev.hprod_block(np.ascontiguousarray(V), HV) == 0
    return HV


def _solve_block(dev, R1, R2):
    k, qp = R1.shape[0], dev.qp
    out = {"p1": np.full((k, qp.n), np.nan), "q1": np.full((k, qp.m), np.nan), "p2": np.full((k, qp.n), np.nan),
           "q2": np.full((k, qp.m), np.nan)}
    assert dev.solve_two_least_squares_block(np.ascontiguousarray(R1), np.ascontiguousarray(R2), **out) == 0
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_every_entry_on_a_handle_with_long_columns_matches_the_dense_kkt_solve(case):
    qp, cols = _qp(case)
    ref = _ref(case)
    V, W = _blocks(case)
    dev = _device(case)
    errs = {}
    # the two solve entries: K [p1; q1] = [rhs1; 0] and K [p2; q2] = [0; rhs2] (mixed) resp. [rhs2; 0] (least squares)
    c = np.random.default_rng(7).standard_normal(qp.m)
    got = _two(dev, "solve_two_mixed", V[0].copy(), c)
    want = ref._solve(V[0], np.zeros(qp.m)) + ref._solve(np.zeros(qp.n), c)
    errs["mixed"] = max(_rel(a, b) for a, b in zip(got, want))
    got = _two(dev, "solve_two_least_squares", V[1].copy(), W[1].copy())
    want = ref._solve(V[1], np.zeros(qp.m)) + ref._solve(W[1], np.zeros(qp.m))
    errs["lsq"] = max(_rel(a, b) for a, b in zip(got, want))
    # the evaluations, both QP models
    for model in ("diag", "hw2"):
        d = dev if model == "diag" else _device(case, model)
        r = ref if model == "diag" else _ref(case, model)
        for rho, eta in ((0.0, 0.0), (1.0, 0.5)):
            d.rho, d.eta = rho, eta
            fx, gx, ys, gs = _objgrad(d, d.qp.x, d.qp.xhat)
            e = r.objgrad(d.qp.x, SIGMA, rho, eta, d.qp.xhat)
            errs[f"{model} objgrad rho={rho}"] = max(_rel(gx, e["gx"]), _rel(ys, e["ys"]), _rel(gs, e["gs"]))
            errs[f"{model} phi rho={rho}"] = abs(fx - e["fx"]) / abs(e["fx"])
        Hv = np.full(qp.n, np.nan)
        assert d.hprod(V[2].copy(), Hv) == 0
        errs[f"{model} hprod"] = _rel(Hv, r.hprod(V[2], SIGMA, 1.0, 0.5))
        HV = _hprod_block(d, V)
        errs[f"{model} hprod_block"] = max(_rel(HV[j], r.hprod(V[j], SIGMA, 1.0, 0.5)) for j in (0, 7, 8))
        if d is not dev:
            d.close()
    out = _solve_block(dev, V[:3], W[:3])
    for j in range(3):
        want = ref._solve(V[j], np.zeros(qp.m)) + ref._solve(W[j], np.zeros(qp.m))
        errs[f"solve_block[{j}]"] = max(_rel(out[k][j], w) for k, w in zip(("p1", "q1", "p2", "q2"), want))
    # A x and A'y in the caller's order, the rows of the long columns among those of A'y and on their own
    A = qp.scipy_csr()
    u = np.random.default_rng(2).standard_normal(qp.m)
    y, z = np.zeros(qp.m), np.empty(qp.n)
    assert dev.jac_mul(0, 1.0, qp.x, 0.0, y) == 0 and dev.jac_mul(1, 1.0, u, 0.0, z) == 0
    Atu = A.T @ u
    errs["jac_mul"] = max(_rel(y, A @ qp.x), _rel(z, Atu), _rel(z[cols], Atu[cols])) * (BAR / 1e-13)   # (held to 1e-13)
    z2 = np.array(z)
    assert dev.jac_mul(1, -0.5, u, 2.0, z2) == 0                          # alpha, beta on the same rows
    errs["jac_mul alpha beta"] = _rel(z2, 2.0 * z - 0.5 * Atu) * (BAR / 1e-13)
    info = dev.info()
    print(f"\n{case}: long columns {info['border_cols']}, last_border_ms {info['last_border_ms']:.3f}, pivot ratio "
          f"{info['border_pivot_ratio']:.3g}, worst {max(errs.values()):.2e}: {errs}")
    assert info["last_border_ms"] > 0.0 and info["regularized_pivots"] == 0 and info["factorizations"] == 1
    assert info["border_pivot_ratio"] >= 1.0
    assert max(errs.values()) < BAR, errs
    dev.close()


def _scaled_aug2dc():
    qp0 = problems.aug2dc_like(N=51)
    qp = problems.with_long_columns(qp0, 4, kind="param", seed=9)
    vals = np.where(qp.colind >= qp0.n, 30.0, 1.0) * qp.vals
    A = sp.csr_matrix((vals, qp.colind, qp.rowptr), shape=(qp.m, qp.n))
    return dataclasses.replace(qp, vals=vals, b=A @ qp.xhat), qp0.n + np.arange(4)


def test_the_documented_loss_where_the_long_columns_dominate():
    """aug2dc_like(51), delta = 0, 4 all-row columns scaled by 30: cond(B) = 1e3, cond(M) = 2e5, cond(S) = 9e3, and the scheme
    itself loses digits (numpy model 1e-10 where a Cholesky of M gives 1e-13).  Each of p1, q1, p2, q2 of both solve entries is
    held to conditioning_cases.sensitive_bar = 8 x max(fp64 LAPACK Cholesky of M, the numpy model of the scheme), both computed
    here on the same inputs against the longdouble truth of tests/kkt_truth.py; border_pivot_ratio must say so."""
    qp, cols = _scaled_aug2dc()
    A = qp.scipy_csr()
    model = LongColumnsModel(A, 0.0, cols)
    M = cc.gram64(A, 0.0)
    dev = DeviceBorderedBandEqQP(qp, border=0, cols=16, sigma=SIGMA, delta=0.0)
    assert dev.info()["border_cols"] == 4 and dev.info()["chains"] == 2
    rng = np.random.default_rng(11)
    r1, r2, c = rng.standard_normal(qp.n), rng.standard_normal(qp.n), rng.standard_normal(qp.m)
    failed = []
    for name, second, mixed in (("solve_two_mixed", c, True), ("solve_two_least_squares", r2, False)):
        truth = (kt.truth_two_mixed if mixed else kt.truth_two_least_squares)(A, 0.0, r1, second)
        lapack = cc.errors(cc.lapack_solve(A, M, r1, second, mixed, np.arange(qp.m)), truth)
        mod = cc.errors(model.solve(r1, second, mixed), truth)
        bar = cc.sensitive_bar(lapack, mod)
        kt.check_uncertainty(truth[4], bar, name)
        got = cc.errors(_two(dev, name, r1.copy(), second.copy()), truth)
        print(f"\n{name}: device {got}, model {mod}, LAPACK {lapack}, bar {bar}")
        if not np.all(got <= bar):
            failed.append((name, got, bar))
    info = dev.info()
    print(f"border_pivot_ratio {info['border_pivot_ratio']:.4g}, numpy's {model.pivot_ratio:.4g}")
    assert info["regularized_pivots"] == 0
    assert model.pivot_ratio / 8.0 <= info["border_pivot_ratio"] <= 8.0 * model.pivot_ratio
    assert not failed, failed
    dev.close()


class Raw:
    """a handle through the C entries themselves, no regularisation.  entry: "plain" (fpsq_band_create[_coo]), ("bordered",
    max_border) or ("cols", max_border, max_cols); coo: the COO entries with the triplets (rows, cols, vals), 0-based"""

    def __init__(self, qp, entry, coo=None):
        self.lib, self.qp, self.coo = _lib.load(), qp, coo
        h = C.c_void_p()
        if coo is None:
            rp = np.ascontiguousarray(qp.rowptr, dtype=np.int32)
            ci = np.ascontiguousarray(qp.colind, dtype=np.int32)
            head = (C.byref(h), qp.n, qp.m, rp.ctypes.data, ci.ctypes.data)
            fn = {"plain": self.lib.fpsq_band_create, "bordered": self.lib.fpsq_band_create_bordered,
                  "cols": self.lib.fpsq_band_create_bordered_cols}
        else:
            r, c = np.ascontiguousarray(coo[0], dtype=np.int64), np.ascontiguousarray(coo[1], dtype=np.int64)
            head = (C.byref(h), qp.n, qp.m, r.size, r.ctypes.data, c.ctypes.data, 0)
            fn = {"plain": self.lib.fpsq_band_create_coo, "bordered": self.lib.fpsq_band_create_coo_bordered,
                  "cols": self.lib.fpsq_band_create_coo_bordered_cols}
        kind, extra = (entry, ()) if entry == "plain" else (entry[0], tuple(int(v) for v in entry[1:]))
        rc = fn[kind](*head, *extra, 0)
        assert rc == 0, self.lib.fpsq_band_last_error(None)
        self.h, self.q = h, None

    def factorize(self, delta):
        pivot = C.c_int32(-7)
        if self.coo is None:
            vals = np.ascontiguousarray(self.qp.vals)
            return self.lib.fpsq_band_factorize(self.h, vals.ctypes.data, float(delta), C.byref(pivot)), pivot.value
        vals = np.ascontiguousarray(self.coo[2], dtype=np.float64)
        return self.lib.fpsq_band_factorize_coo(self.h, vals.ctypes.data, float(delta), C.byref(pivot)), pivot.value

    def model(self):
        q, qp = C.c_void_p(), self.qp
        assert self.lib.fpsq_band_qp_create(self.h, qp.qdiag.ctypes.data, qp.d.ctypes.data, qp.b.ctypes.data, C.byref(q)) == 0
        self.q = q

    def objgrad(self, x, rho=1.0, eta=0.5):
        qp = self.qp
        fx = C.c_double()
        gx, ys, gs = np.full(qp.n, np.nan), np.full(qp.m, np.nan), np.full(qp.n, np.nan)
        rc = self.lib.fpsq_band_qp_objgrad(self.h, self.q, x.ctypes.data, SIGMA, rho, eta, qp.xhat.ctypes.data, C.byref(fx),
                                           gx.ctypes.data, ys.ctypes.data, gs.ctypes.data)
        return rc, fx.value, gx, ys, gs

    def hprod_block(self, V):
        HV = np.full(V.shape, np.nan)
        V = np.ascontiguousarray(V)
        rc = self.lib.fpsq_band_qp_hprod_block(self.h, self.q, V.shape[0], V.ctypes.data, SIGMA, 1.0, 0.5, 2, HV.ctypes.data)
        return rc, HV

    def two(self, name, rhs1, rhs2):
        return _two_on(self.lib, self.h, self.qp, name, rhs1, rhs2)

    def info(self):
        i = _lib.BandInfo()
        assert self.lib.fpsq_band_get_info(self.h, C.byref(i)) == 0
        return i.as_dict()

    def close(self):
        if self.q:
            self.lib.fpsq_band_qp_destroy(self.q)
        assert self.lib.fpsq_band_destroy(self.h) == 0


def _triplets(qp):
    return np.repeat(np.arange(qp.m, dtype=np.int64), np.diff(qp.rowptr)), qp.colind.astype(np.int64), qp.vals


def test_max_cols_zero_through_the_new_entries_is_bitwise_the_existing_entries():
    """on the problem WITH long columns (a wide band, as the existing entries store it) and on one without; the CSR and the
    COO entry (fpsq_band_analyze_bordered_cols is compared on the host, tests/test_band_long_columns_cpu.py)"""
    keys = ("nblocks", "bandwidth_blocks", "factor_bytes", "reordered", "chains", "nnz", "border_rows", "border_cols",
            "border_pivot_ratio", "regularized_pivots")
    for qp in (_qp("m640-s5-param-delta0")[0], _p640()):
        V = np.random.default_rng(5).standard_normal((9, qp.n))
        c = np.random.default_rng(6).standard_normal(qp.m)
        for coo in (None, _triplets(qp)):
            outs = []
            for entry in ("plain", ("cols", 0, 0)):
                r = Raw(qp, entry, coo)
                assert r.factorize(SE) == (0, 0)
                r.model()
                rc, fx, gx, ys, gs = r.objgrad(qp.x)
                rc2, HV = r.hprod_block(V)
                assert rc == 0 and rc2 == 0
                solves = r.two("solve_two_mixed", V[0].copy(), c) + r.two("solve_two_least_squares", V[1].copy(), V[2].copy())
                i = r.info()
                assert i["border_cols"] == 0 and i["border_pivot_ratio"] == 1.0 and i["last_border_ms"] == 0.0
                outs.append(((np.float64(fx), gx, ys, gs, HV) + solves, {k: i[k] for k in keys}))
                r.close()
            for a, b in zip(outs[0][0], outs[1][0]):
                assert np.array_equal(a, b)
            assert outs[0][1] == outs[1][1]


def test_repeat_calls_and_block_columns_are_bitwise_stable():
    case = "m1500-s5-stride-shuffled-delta0"
    qp, _ = _qp(case)
    V, W = _blocks(case)
    dev = _device(case)
    first, again = _objgrad(dev, qp.x, qp.xhat), _objgrad(dev, qp.x, qp.xhat)
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    s1 = _two(dev, "solve_two_least_squares", V[0].copy(), W[0].copy())
    s2 = _two(dev, "solve_two_least_squares", V[0].copy(), W[0].copy())
    for a, b in zip(s1, s2):
        assert np.array_equal(a, b)
    # a column's bits: whatever k (1, 8, 9: the ninth column is a tile of its own), its position and its neighbours
    H9 = _hprod_block(dev, V)
    assert np.array_equal(H9, _hprod_block(dev, V))
    assert np.array_equal(_hprod_block(dev, V[:1])[0], H9[0])
    assert np.array_equal(_hprod_block(dev, V[:8]), H9[:8])
    moved = np.ascontiguousarray(V[[8, 3, 0]])                           # column 0 of V last, the ninth first
    Hm = _hprod_block(dev, moved)
    assert np.array_equal(Hm[2], H9[0]) and np.array_equal(Hm[0], H9[8]) and np.array_equal(Hm[1], H9[3])
    other = np.array(V[:8])
    other[1:] = np.random.default_rng(99).standard_normal((7, qp.n)) * 1e3   # other neighbours
    assert np.array_equal(_hprod_block(dev, other)[0], H9[0])
    S9 = _solve_block(dev, V, W)
    S1 = _solve_block(dev, V[4:5], W[4:5])
    S8 = _solve_block(dev, V[1:9], W[1:9])
    for k in ("p1", "q1", "p2", "q2"):
        assert np.array_equal(S1[k][0], S9[k][4]) and np.array_equal(S8[k], S9[k][1:9])
    # objgrad_block: a column's bits whatever k and position
    X = np.ascontiguousarray(qp.x[None, :] + 0.01 * V)
    G9 = np.full(X.shape, np.nan)
    f9, rc = dev.objgrad_block(X, GX=G9)
    G2 = np.full((2, qp.n), np.nan)
    f2, rc2 = dev.objgrad_block(np.ascontiguousarray(X[[8, 0]]), GX=G2)
    assert rc == 0 and rc2 == 0
    assert np.array_equal(f2, f9[[8, 0]]) and np.array_equal(G2, G9[[8, 0]])
    e = _ref(case).objgrad(X[8], SIGMA, 1.0, 0.5, None)
    assert _rel(G9[8], e["gx"]) < BAR and abs(f9[8] - e["fx"]) <= BAR * abs(e["fx"])
    dev.close()


def test_refactorisation_follows_new_values_and_delta_like_a_fresh_handle():
    import torch

    case = "m640-s16-stride-first"
    qp, _ = _qp(case)
    on = torch.device("cuda", 0)
    dev = _device(case)
    before = _objgrad(dev, qp.x, qp.xhat)
    ratio_before = dev.info()["border_pivot_ratio"]
    new_vals = qp.vals * (1.0 + 0.25 * np.cos(np.arange(qp.nnz)))
    big = torch.rand(2048, 2048, dtype=torch.float64, device=on)
    for _ in range(3):                                                    # the values are still being produced at the call
        big = big @ big * 1e-3
    dev.set_jacobian_values(torch.from_numpy(new_vals).to(on) * 1.0)
    dev.set_delta(1e-3)
    after = _objgrad(dev, qp.x, qp.xhat)
    assert dev.info()["factorizations"] == 2 and not np.array_equal(after[1], before[1])
    assert dev.info()["border_pivot_ratio"] != ratio_before
    fresh_qp = dataclasses.replace(qp, vals=new_vals)
    fresh = DeviceBorderedBandEqQP(fresh_qp, border=0, cols=16, sigma=SIGMA, rho=1.0, delta=1e-3, eta=0.5)
    want = _objgrad(fresh, qp.x, qp.xhat)
    for a, b in zip(after, want):
        assert np.array_equal(a, b)
    assert fresh.info()["border_pivot_ratio"] == dev.info()["border_pivot_ratio"]
    e = DenseRef(fresh_qp, _dense_lu_of(fresh_qp, 1e-3)).objgrad(qp.x, SIGMA, 1.0, 0.5, qp.xhat)
    assert _rel(after[1], e["gx"]) < BAR and _rel(after[2], e["ys"]) < BAR and abs(after[0] - e["fx"]) <= BAR * abs(e["fx"])
    fresh.close()
    dev.close()


def test_device_tensors_on_a_registered_stream_give_the_bits_of_host_arrays():
    import torch

    case = "m1500-s1-middle"
    qp, _ = _qp(case)
    on = torch.device("cuda", 0)
    dev = _device(case)
    host = _objgrad(dev, qp.x, qp.xhat)
    t = lambda a: torch.from_numpy(np.array(a)).to(on)  # noqa: E731  (a copy: the shared blocks are read-only)
    gx, ys, gs = (torch.empty(k, dtype=torch.float64, device=on) for k in (qp.n, qp.m, qp.n))
    fx, rc = dev.objgrad(t(qp.x), gx=gx, ys=ys, gs=gs, xk=t(qp.xhat))
    assert rc == 0 and fx == host[0]
    for a, b in zip((gx, ys, gs), host[1:]):
        assert np.array_equal(a.cpu().numpy(), b)
    V, _ = _blocks(case)
    HV = torch.empty((3, qp.n), dtype=torch.float64, device=on)
    assert dev.hprod_block(t(V[:3]), HV) == 0
    assert np.array_equal(HV.cpu().numpy(), _hprod_block(dev, V[:3]))
    u = np.random.default_rng(2).standard_normal(qp.m)
    z_host, z_dev = np.empty(qp.n), torch.empty(qp.n, dtype=torch.float64, device=on)
    assert dev.jac_mul(1, 1.0, u, 0.0, z_host) == 0 and dev.jac_mul(1, 1.0, t(u), 0.0, z_dev) == 0
    assert np.array_equal(z_dev.cpu().numpy(), z_host)
    dev.close()


def test_the_per_step_sweeps_take_the_same_correction(monkeypatch):
    """FPSQ_TRSV_CHAIN=0 (one launch per step of the sweeps) on a handle with long columns: the same algebra, another
    summation order"""
    case = "aug2dc-two-chains-s16-param"
    qp, _ = _qp(case)
    dev = _device(case)
    chain = _objgrad(dev, qp.x, qp.xhat)
    dev.close()
    monkeypatch.setenv("FPSQ_TRSV_CHAIN", "0")
    steps = _device(case)
    other = _objgrad(steps, qp.x, qp.xhat)
    steps.close()
    assert abs(other[0] - chain[0]) <= 1e-12 * abs(chain[0])
    for a, b in zip(other[1:], chain[1:]):
        assert _rel(a, b) < 1e-12


def test_fps_solve_device_on_a_handle_with_long_columns_agrees_with_the_wide_band_handle():
    import torch

    from fps_amd.fps_solve import fps_solve_device

    case = "m640-s5-param-delta0"
    qp, _ = _qp(case)
    on = torch.device("cuda", 0)
    res = {}
    for name, cols in (("cols", 16), ("wide", 0)):
        dev = DeviceBorderedBandEqQP(qp, border=0, cols=cols)
        assert dev.info()["border_cols"] == (5 if cols else 0)
        stats = fps_solve_device(dev, torch.from_numpy(qp.x).to(on), max_time=120)
        res[name] = (stats.status, stats.solution.cpu().numpy(), stats.multipliers.cpu().numpy())
        dev.close()
    dist = np.linalg.norm(res["cols"][1] - res["wide"][1]) / np.linalg.norm(res["wide"][1])
    print(f"\n{case}: {res['cols'][0]} / {res['wide'][0]}, |dx|/|x| = {dist:.2e}")
    assert res["cols"][0] == res["wide"][0] == "first_order"
    assert dist <= 1e-6


def test_the_coo_entry_behind_the_qdsolver_seam_takes_the_same_columns():
    """HIPBandedDirectQDSolver(cols=16) (fpsq_band_create_coo_bordered_cols, fpsq_band_factorize_coo) behind FletcherPenaltyNLP
    against fpsq_band_qp_objgrad on the CSR entry: the same columns and factor, other summation orders in the products --
    1e-12 relative, the bar of the existing seam test."""
    from fps_amd import nlpmodels
    from fps_amd.penalty_nlp import FletcherPenaltyNLP
    from fps_amd.qdsolver import HIPBandedDirectQDSolver

    case = "m1500-s5-stride-shuffled-delta0"
    qp, _ = _qp(case)
    model = nlpmodels.EqQPModel(qp)
    qds = HIPBandedDirectQDSolver(model, 0.0, cols=16)
    assert qds.info()["border_cols"] == 5 and qds.info()["nblocks"] == 12 and qds.info()["bandwidth_blocks"] == 2
    fp = FletcherPenaltyNLP(model, SIGMA, 1.0, 0.0, 2, qds=qds)
    f_seam, g_seam = fp.objgrad(qp.x)
    dev = _device(case, rho=1.0, eta=0.0)
    fx, gx, ys, gs = _objgrad(dev, qp.x, None)
    assert abs(fx - f_seam) <= 1e-12 * abs(f_seam)
    assert _rel(gx, g_seam) < 1e-12 and _rel(ys, fp.ys) < 1e-12 and _rel(gs, fp.gs) < 1e-12
    plain = HIPBandedDirectQDSolver(model, 0.0)
    assert plain.info()["border_cols"] == 0
    plain.close()
    qds.close()
    dev.close()


@pytest.mark.parametrize("form", ["by-columns", "by-row-pairs"])
def test_a_pattern_with_duplicates_through_the_coo_entry(form, monkeypatch):
    """every third triplet split into two halves (the long columns' among them), summed on the device into the CSR slots;
    FPSQ_BAND_FORM=1 sends the formation through k_band_form (row pairs, the CSR of the other columns alone) instead of
    k_band_form_t: both must form B, not M"""
    case = "m640-s5-param-delta0"
    qp, _ = _qp(case)
    if form == "by-row-pairs":
        monkeypatch.setenv("FPSQ_BAND_FORM", "1")
    r, c, v = _triplets(qp)
    split = np.arange(v.size) % 3 == 0
    v1 = np.where(split, 0.5 * v, v)
    order = np.random.default_rng(4).permutation(v.size + int(split.sum()))
    coo = (np.concatenate([r, r[split]])[order], np.concatenate([c, c[split]])[order], np.concatenate([v1, 0.5 * v[split]])[order])
    h = Raw(qp, ("cols", 0, 16), coo)
    assert h.info()["border_cols"] == 5 and h.info()["nblocks"] == 5 and h.info()["nnz"] == qp.nnz
    assert h.factorize(0.0) == (0, 0)
    ref = _ref(case)
    V, W = _blocks(case)
    got = h.two("solve_two_least_squares", V[1].copy(), W[1].copy())
    want = ref._solve(V[1], np.zeros(qp.m)) + ref._solve(W[1], np.zeros(qp.m))
    err = max(_rel(a, b) for a, b in zip(got, want))
    print(f"\n{case} with duplicates, formation {form}: {err:.2e}")
    assert h.info()["regularized_pivots"] == 0 and h.info()["last_border_ms"] > 0.0
    assert err < BAR
    h.close()
