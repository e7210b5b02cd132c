"""Border rows AND long columns on one banded handle (fpsq_band_create_arrow, DeviceArrowBandEqQP): a few long constraint rows
are eliminated last as a border, a few long columns are taken out as a low-rank term, M = M_r + U U' with M_r the bordered
band, and every M-solve is the sweeps on the band plus the two corrections, fused into one reduction and one update (include/
fpsq.h "ARROW BAND").

Yardstick: a DENSE fp64 solve of K = [I A'; A -delta I] (scipy.linalg.lu_factor, once per shape, shared) and the closed forms
of objgrad / hprod of include/fpsq.h (tests/sparse_hessian_ref.py, on that dense factor), at the bars the existing banded tests
hold each entry to: max|a - b| / max|b| < 1e-9 per vector, |phi - phi_exact| <= 1e-9 |phi_exact|, 1e-13 for A x / A'y (the
rows of the long columns and the border rows included).  A numpy model of the scheme (tests/arrow_model.py) loses 2e-15 ..
5e-15 on shapes like these, so the bars leave five digits: a case that needs more is a defect.  Every call must return 0.

Shapes: the band parts of tests/test_gpu_band_long_columns.py, the smallest at which the selection takes both kinds (checked
on the host with fpsq_band_analyze_arrow, tests/test_band_arrow_cpu.py)."""
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
from arrow_model import ArrowModel  # noqa: E402
from fps_amd import _lib, problems  # noqa: E402
from fps_amd.device_qp import DeviceArrowBandEqQP, DeviceBandEqQP  # noqa: E402
from sparse_hessian_ref import SparseHessianRef  # noqa: E402

pytestmark = pytest.mark.gpu

SE = float(np.sqrt(np.finfo(float).eps))
SIGMA = 1e3
BAR = 1e-9
BAR_PRODUCT = 1e-13


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
    """Returns (qp with row p = row order[p] of the argument, order)"""
    order = np.random.default_rng(seed).permutation(qp.m)
    A = sp.csr_matrix(qp.scipy_csr()[order])
    A.sort_indices()
    return dataclasses.replace(qp, rowptr=A.indptr.astype(np.int32), colind=A.indices.astype(np.int32), vals=A.data.copy(),
                               b=qp.b[order]), order


def _placed(qp0, s_r, s_c, kind, where, shuffle, seed=9):
    """qp0 with s_r mean rows and s_c long columns that reach them; `where` the columns sit in the caller's column order.
    Returns (qp, the long rows, the long columns), both ascending in the caller's numbering"""
    qp = problems.with_arrow(qp0, s_r, s_c, col_kind=kind, seed=seed)
    at = {"last": qp0.n, "first": 0}[where]
    if where != "last":
        qp = _columns_moved(qp, np.concatenate([np.arange(at), np.arange(at + s_c, qp.n), at + np.arange(s_c)]))
    rows = qp0.m + np.arange(s_r)
    if shuffle:
        qp, order = _rows_shuffled(qp, seed)
        rows = np.sort(np.nonzero(order >= qp0.m)[0])
    return qp, rows, at + np.arange(s_c)


def _p640():
    return problems.pde_control_like(n=3000, m=640, per_row=12, window=256, seed=5)


def _p1500():
    return problems.pde_control_like(n=3600, m=1500, per_row=12, window=256, seed=6)


# name: (band part, s_r, s_c, column kind, where the columns sit, rows shuffled, delta, expected info of the handle)
CASES = {
    # (640 band rows fill 5 blocks exactly: the border rows open a block of padding behind them; mpad = 768)
    "m640-r3-c5-param-delta0": (_p640, 3, 5, "param", "last", False, 0.0, {"nblocks": 5, "chains": 1, "reordered": 0}),
    "m640-r16-c16-stride-first": (_p640, 16, 16, "stride", "first", False, SE, {"nblocks": 5, "chains": 1}),
    # (all rows shuffled: reverse Cuthill-McKee runs on the band rows; 1500 band rows: the border row sits in the padding of
    # the last block)
    "m1500-r1-c1-shuffled": (_p1500, 1, 1, "param", "last", True, SE, {"nblocks": 12, "chains": 1, "reordered": 1}),
    "aug2dc-two-chains-r2-c16-param": (lambda: problems.aug2dc_like(N=51), 2, 16, "param", "last", False, SE,
                                       {"nblocks": 21, "chains": 2}),
}
KMAX = 9


@functools.lru_cache(maxsize=None)
def _qp(case, model="diag"):
    make, s_r, s_c, kind, where, shuffle, _, _ = CASES[case]
    qp, rows, cols = _placed(make(), s_r, s_c, kind, where, shuffle)
    if model != "diag":
        qp = problems.with_sparse_hessian(qp, 2, 11)
    return qp, rows, cols


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
    return _dense_lu_of(_qp(case)[0], CASES[case][6])


def _ref(case, model="diag"):
    return DenseRef(_qp(case, model)[0], _dense_lu(case))


@functools.lru_cache(maxsize=None)
def _blocks(case):
    qp = _qp(case)[0]
    rng = np.random.default_rng(1234)
    V, W = rng.standard_normal((KMAX, qp.n)), rng.standard_normal((KMAX, qp.n))
    V.setflags(write=False)
    W.setflags(write=False)
    return V, W


def _device(case, model="diag", rho=1.0, eta=0.5, **kw):
    qp = _qp(case, model)[0]
    dev = DeviceArrowBandEqQP(qp, sigma=SIGMA, rho=rho, delta=CASES[case][6], eta=eta, **kw)
    info = dev.info()
    assert (info["border_rows"], info["border_cols"]) == CASES[case][1:3], info
    for k, v in CASES[case][7].items():
        assert info[k] == v, (k, info)
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


def _objgrad_block(dev, X, XK):
    k, qp = X.shape[0], dev.qp
    out = {"GX": np.full((k, qp.n), np.nan), "YS": np.full((k, qp.m), np.nan), "GS": np.full((k, qp.n), np.nan)}
    f, rc = dev.objgrad_block(np.ascontiguousarray(X), XK=np.ascontiguousarray(XK), **out)
    assert rc == 0
    return f, out


@functools.lru_cache(maxsize=None)
def _expected(case, model):
    """everything the dense LU says about a case, computed once: the block tests at k = 1, 8, 9 compare columns of it"""
    qp = _qp(case, model)[0]
    r = _ref(case, model)
    V, W = _blocks(case)
    X = qp.x[None, :] + 0.01 * V
    e = {"hprod": [r.hprod(V[j], SIGMA, 1.0, 0.5) for j in range(KMAX)],
         "og": [r.objgrad(X[j], SIGMA, 1.0, 0.5, qp.xhat) for j in range(KMAX)]}
    if model == "diag":
        e["lsq"] = [r._solve(V[j], np.zeros(qp.m)) + r._solve(W[j], np.zeros(qp.m)) for j in range(KMAX)]
    return e


@pytest.mark.parametrize("case", list(CASES))
def test_every_entry_on_an_arrow_handle_matches_the_dense_kkt_solve(case):
    qp, rows, cols = _qp(case)
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
    errs["lsq"] = max(_rel(a, b) for a, b in zip(got, _expected(case, "diag")["lsq"][1]))
    # the evaluations, both QP models; the block entries at k = 1, 8, 9 (the ninth column is a tile of its own)
    for model in ("diag", "hw2"):
        d = dev if model == "diag" else _device(case, model)
        r = ref if model == "diag" else _ref(case, model)
        exp = _expected(case, model)
        for rho, eta in ((0.0, 0.0), (1.0, 0.5)):
            d.rho, d.eta = rho, eta
            fx, gx, ys, gs = _objgrad(d, d.qp.x, d.qp.xhat)
            e = r.objgrad(d.qp.x, SIGMA, rho, eta, d.qp.xhat)
            errs[f"{model} objgrad rho={rho}"] = max(_rel(gx, e["gx"]), _rel(ys, e["ys"]), _rel(gs, e["gs"]))
            errs[f"{model} phi rho={rho}"] = abs(fx - e["fx"]) / abs(e["fx"])
        Hv = np.full(qp.n, np.nan)
        assert d.hprod(V[2].copy(), Hv) == 0
        errs[f"{model} hprod"] = _rel(Hv, exp["hprod"][2])
        X = np.ascontiguousarray(d.qp.x[None, :] + 0.01 * V)
        XK = np.ascontiguousarray(np.tile(d.qp.xhat, (KMAX, 1)))
        for k in (1, 8, 9):
            HV = _hprod_block(d, V[:k])
            errs[f"{model} hprod_block k={k}"] = max(_rel(HV[j], exp["hprod"][j]) for j in range(k))
            f, out = _objgrad_block(d, X[:k], XK[:k])
            errs[f"{model} objgrad_block k={k}"] = max(
                max(_rel(out["GX"][j], exp["og"][j]["gx"]), _rel(out["YS"][j], exp["og"][j]["ys"]),
                    _rel(out["GS"][j], exp["og"][j]["gs"]), abs(f[j] - exp["og"][j]["fx"]) / abs(exp["og"][j]["fx"]))
                for j in range(k))
        if d is not dev:
            d.close()
    for k in (1, 8, 9):
        out = _solve_block(dev, V[:k], W[:k])
        errs[f"solve_block k={k}"] = max(_rel(out[key][j], w) for j in range(k)
                                         for key, w in zip(("p1", "q1", "p2", "q2"), _expected(case, "diag")["lsq"][j]))
    # A x and A'y in the caller's order, the rows of the long columns and the border rows among them and on their own
    A = qp.scipy_csr()
    u = np.random.default_rng(2).standard_normal(qp.m)
    y, z = np.zeros(qp.m), np.empty(qp.n)
    assert dev.jac_mul(0, 1.0, qp.x, 0.0, y) == 0 and dev.jac_mul(1, 1.0, u, 0.0, z) == 0
    Ax, Atu = A @ qp.x, A.T @ u
    scale = BAR / BAR_PRODUCT                                              # (held to 1e-13)
    errs["jac_mul"] = max(_rel(y, Ax), _rel(y[rows], Ax[rows]), _rel(z, Atu), _rel(z[cols], Atu[cols])) * scale
    z2 = np.array(z)
    assert dev.jac_mul(1, -0.5, u, 2.0, z2) == 0                          # alpha, beta on the same rows
    errs["jac_mul alpha beta"] = _rel(z2, 2.0 * z - 0.5 * Atu) * scale
    info = dev.info()
    print(f"\n{case}: border rows {info['border_rows']}, long columns {info['border_cols']}, last_border_ms "
          f"{info['last_border_ms']:.3f}, pivot ratio {info['border_pivot_ratio']:.3g}, worst {max(errs.values()):.2e}: {errs}")
    assert info["last_border_ms"] > 0.0 and info["regularized_pivots"] == 0 and info["factorizations"] == 1
    assert info["border_pivot_ratio"] >= 1.0
    assert max(errs.values()) < BAR, errs
    dev.close()


def test_the_fused_and_the_nested_correction_both_meet_the_bar(monkeypatch):
    """FPSQ_ARROW_FUSED=0 (read at create): the row border's two launches, then the long columns' two, instead of the fused
    pair.  Another summation order: the two agree to rounding, and each is held to the dense LU on its own."""
    case = "m640-r16-c16-stride-first"
    qp = _qp(case)[0]
    V, W = _blocks(case)
    ref = _ref(case)
    e = ref.objgrad(qp.x, SIGMA, 1.0, 0.5, qp.xhat)
    want = _expected(case, "diag")
    got = {}
    for form in ("fused", "nested"):
        if form == "nested":
            monkeypatch.setenv("FPSQ_ARROW_FUSED", "0")
        dev = _device(case)
        fx, gx, ys, gs = _objgrad(dev, qp.x, qp.xhat)
        HV = _hprod_block(dev, V)
        lsq = _two(dev, "solve_two_least_squares", V[1].copy(), W[1].copy())
        dev.close()
        err = max(_rel(gx, e["gx"]), _rel(ys, e["ys"]), _rel(gs, e["gs"]), abs(fx - e["fx"]) / abs(e["fx"]),
                  max(_rel(HV[j], want["hprod"][j]) for j in range(KMAX)),
                  max(_rel(a, b) for a, b in zip(lsq, want["lsq"][1])))
        print(f"\n{case}, {form}: worst {err:.2e}")
        assert err < BAR
        got[form] = (gx, ys, gs, HV) + lsq
    assert not all(np.array_equal(a, b) for a, b in zip(got["fused"], got["nested"]))   # (the switch did switch)


class Raw:
    """a handle through the C entries themselves, no regularisation.  entry: "plain" (fpsq_band_create[_coo]), ("bordered",
    max_border), ("cols", max_border, max_cols) or ("arrow", max_border, max_cols); coo: the COO entries with the triplets
    (rows, cols, vals), 0-based"""

    def __init__(self, qp, entry, coo=None):
        self.lib, self.qp, self.coo = _lib.load(), qp, coo
        h = C.c_void_p()
        if coo is None:
            rp = np.ascontiguousarray(qp.rowptr, dtype=np.int32)
            ci = np.ascontiguousarray(qp.colind, dtype=np.int32)
            head = (C.byref(h), qp.n, qp.m, rp.ctypes.data, ci.ctypes.data)
            fn = {"plain": self.lib.fpsq_band_create, "bordered": self.lib.fpsq_band_create_bordered,
                  "cols": self.lib.fpsq_band_create_bordered_cols, "arrow": self.lib.fpsq_band_create_arrow}
        else:
            r, c = np.ascontiguousarray(coo[0], dtype=np.int64), np.ascontiguousarray(coo[1], dtype=np.int64)
            head = (C.byref(h), qp.n, qp.m, r.size, r.ctypes.data, c.ctypes.data, 0)
            fn = {"plain": self.lib.fpsq_band_create_coo, "bordered": self.lib.fpsq_band_create_coo_bordered,
                  "cols": self.lib.fpsq_band_create_coo_bordered_cols, "arrow": self.lib.fpsq_band_create_coo_arrow}
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


def test_a_zero_maximum_through_the_arrow_entries_gives_the_bits_of_the_existing_entries():
    """max_cols = 0 is the bordered entry, max_border = 0 the long-column entry, both 0 the plain one -- on the problem that
    has both kinds (one kind is then left in the band, as the existing entries leave it), CSR and COO entry"""
    keys = ("nblocks", "bandwidth_blocks", "factor_bytes", "reordered", "chains", "nnz", "border_rows", "border_cols",
            "border_pivot_ratio", "regularized_pivots")
    qp = _qp("m640-r3-c5-param-delta0")[0]
    V = np.random.default_rng(5).standard_normal((9, qp.n))
    c = np.random.default_rng(6).standard_normal(qp.m)
    pairs = ((("bordered", 16), ("arrow", 16, 0)), (("cols", 0, 16), ("arrow", 0, 16)), ("plain", ("arrow", 0, 0)))
    for coo in (None, _triplets(qp)):
        for pair in pairs:
            outs = []
            for entry in pair:
                r = Raw(qp, entry, coo)
                assert r.factorize(SE) == (0, 0)
                r.model()
                rc, fx, gx, ys, gs = r.objgrad(qp.x)
                rc2, HV = r.hprod_block(V)
                assert rc == 0 and rc2 == 0
                solves = r.two("solve_two_mixed", V[0].copy(), c) + r.two("solve_two_least_squares", V[1].copy(), V[2].copy())
                i = r.info()
                outs.append(((np.float64(fx), gx, ys, gs, HV) + solves, {k: i[k] for k in keys}))
                r.close()
            for a, b in zip(outs[0][0], outs[1][0]):
                assert np.array_equal(a, b), pair
            assert outs[0][1] == outs[1][1], pair


def test_repeat_calls_and_block_columns_are_bitwise_stable():
    case = "m1500-r1-c1-shuffled"
    qp = _qp(case)[0]
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
    other[1:] *= 1e300                                                    # neighbours that overflow: a column reads its own only
    with np.errstate(all="ignore"):
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
    dev.close()


def test_refactorisation_follows_new_values_and_delta_like_a_fresh_handle():
    case = "m640-r16-c16-stride-first"
    qp = _qp(case)[0]
    dev = _device(case)
    before = _objgrad(dev, qp.x, qp.xhat)
    ratio_before = dev.info()["border_pivot_ratio"]
    new_vals = qp.vals * (1.0 + 0.25 * np.cos(np.arange(qp.nnz)))
    dev.set_jacobian_values(new_vals)
    dev.set_delta(1e-3)
    after = _objgrad(dev, qp.x, qp.xhat)
    assert dev.info()["factorizations"] == 2 and not np.array_equal(after[1], before[1])
    assert dev.info()["border_pivot_ratio"] != ratio_before
    fresh_qp = dataclasses.replace(qp, vals=new_vals)
    fresh = DeviceArrowBandEqQP(fresh_qp, sigma=SIGMA, rho=1.0, delta=1e-3, eta=0.5)
    want = _objgrad(fresh, qp.x, qp.xhat)
    for a, b in zip(after, want):
        assert np.array_equal(a, b)
    assert fresh.info()["border_pivot_ratio"] == dev.info()["border_pivot_ratio"]
    e = DenseRef(fresh_qp, _dense_lu_of(fresh_qp, 1e-3)).objgrad(qp.x, SIGMA, 1.0, 0.5, qp.xhat)
    assert _rel(after[1], e["gx"]) < BAR and _rel(after[2], e["ys"]) < BAR and abs(after[0] - e["fx"]) <= BAR * abs(e["fx"])
    fresh.close()
    dev.close()


def test_the_per_step_sweeps_take_the_same_correction(monkeypatch):
    """FPSQ_TRSV_CHAIN=0 (one launch per step of the sweeps) on an arrow handle: the same algebra, another summation order"""
    case = "aug2dc-two-chains-r2-c16-param"
    qp = _qp(case)[0]
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


def _exactly_singular():
    """The construction of tests/test_gpu_band_border.py with a long column added: band rows with four entries +-1 in columns
    of their own (B = 4 I: exact in fp64), ONE long row, at index 100, that is the sum of all band rows -- S_r = D - C'Z_r =
    2560 - 640 * 4 * 1 is an EXACT zero -- and one column of ones that touches every row and belongs to U, not to S_r."""
    mb, at = 640, 100
    n = 4 * mb
    sign = np.where((np.arange(n) * 7) % 3 == 0, -1.0, 1.0)
    A = sp.vstack([sp.csr_matrix((sign, (np.repeat(np.arange(mb), 4), np.arange(n))), shape=(mb, n)),
                   sp.csr_matrix(sign[None, :])]).tocsr()
    order = np.concatenate([np.arange(at), [mb], np.arange(at, mb)])
    A = sp.csr_matrix(sp.hstack([A[order], sp.csr_matrix(np.ones((mb + 1, 1)))]))
    A.sort_indices()
    xhat = np.linspace(-1.0, 1.0, n + 1)
    return problems.EqQP("exactly-singular-arrow", n + 1, mb + 1, A.indptr.astype(np.int32), A.indices.astype(np.int32),
                         A.data.copy(), np.linspace(1.0, 2.0, n + 1), np.ones(n + 1), A @ xhat, xhat + 0.1, xhat), at


def test_singular_border_without_regularisation_reports_the_border_row():
    qp, at = _exactly_singular()
    r = Raw(qp, ("arrow", 1, 1))
    assert (r.info()["border_rows"], r.info()["border_cols"], r.info()["bandwidth_blocks"]) == (1, 1, 0)
    rc, pivot = r.factorize(0.0)
    assert (rc, pivot) == (1, at + 1)                                     # soft code, the row 1-based in the caller's order
    r.model()
    assert r.objgrad(qp.x)[0] == -3                                       # FPSQ_ERR_STATE
    assert r.factorize(1e-3) == (0, 0)                                    # delta > 0: positive definite again
    assert r.objgrad(qp.x)[0] == 0
    r.close()


def test_singular_border_with_the_default_regularisation_is_regularised():
    qp, _ = _exactly_singular()
    dev = DeviceArrowBandEqQP(qp, border=1, cols=1, sigma=SIGMA, rho=1.0, delta=0.0)
    fx, gx, ys, gs = _objgrad(dev, qp.x, None)
    i = dev.info()
    assert (i["border_rows"], i["border_cols"]) == (1, 1) and i["regularized_pivots"] >= 1
    assert np.isfinite(fx) and all(np.all(np.isfinite(a)) for a in (gx, ys, gs))
    Hv = np.full(qp.n, np.nan)
    assert dev.hprod(qp.x, Hv) == 0 and np.all(np.isfinite(Hv))
    dev.close()


def test_fps_solve_device_on_an_arrow_handle_agrees_with_the_wide_band_handle():
    import torch

    from fps_amd.fps_solve import fps_solve_device

    case = "m640-r3-c5-param-delta0"
    qp = _qp(case)[0]
    on = torch.device("cuda", 0)
    res = {}
    for name, cls in (("arrow", DeviceArrowBandEqQP), ("wide", DeviceBandEqQP)):
        dev = cls(qp)
        assert (dev.info()["border_rows"], dev.info()["border_cols"]) == ((3, 5) if name == "arrow" else (0, 0))
        stats = fps_solve_device(dev, torch.from_numpy(qp.x).to(on), max_time=120)
        res[name] = (stats.status, stats.solution.cpu().numpy(), stats.multipliers.cpu().numpy())
        dev.close()
    dist = np.linalg.norm(res["arrow"][1] - res["wide"][1]) / np.linalg.norm(res["wide"][1])
    print(f"\n{case}: {res['arrow'][0]} / {res['wide'][0]}, |dx|/|x| = {dist:.2e}")
    assert res["arrow"][0] == res["wide"][0] == "first_order"
    assert dist <= 1e-6


def test_the_coo_entry_behind_the_qdsolver_seam_takes_the_same_rows_and_columns():
    """HIPArrowBandedDirectQDSolver (fpsq_band_create_coo_arrow, fpsq_band_factorize_coo) behind FletcherPenaltyNLP against
    fpsq_band_qp_objgrad on the CSR entry: the same rows, columns and factor, other summation orders in the products -- 1e-12
    relative, the bar of the existing seam test."""
    from fps_amd import nlpmodels
    from fps_amd.penalty_nlp import FletcherPenaltyNLP
    from fps_amd.qdsolver import HIPArrowBandedDirectQDSolver, qdsolver_correspondence

    assert qdsolver_correspondence["hip_ldlt_arrow"] is HIPArrowBandedDirectQDSolver
    case = "m1500-r1-c1-shuffled"
    qp = _qp(case)[0]
    model = nlpmodels.EqQPModel(qp)
    qds = HIPArrowBandedDirectQDSolver(model, 0.0)
    dev = _device(case, rho=1.0, eta=0.0)
    for k in ("border_rows", "border_cols", "nblocks", "bandwidth_blocks", "chains", "reordered"):
        assert qds.info()[k] == dev.info()[k], k
    fp = FletcherPenaltyNLP(model, SIGMA, 1.0, CASES[case][6], 2, qds=qds)
    f_seam, g_seam = fp.objgrad(qp.x)
    fx, gx, ys, gs = _objgrad(dev, qp.x, None)
    assert abs(fx - f_seam) <= 1e-12 * abs(f_seam)
    assert _rel(gx, g_seam) < 1e-12 and _rel(ys, fp.ys) < 1e-12 and _rel(gs, fp.gs) < 1e-12
    qds.close()
    dev.close()


@pytest.mark.parametrize("form", ["by-columns", "by-row-pairs"])
def test_a_pattern_with_duplicates_through_the_coo_entry(form, monkeypatch):
    """every third triplet split into two halves (the long columns' and the border rows' among them), summed on the device
    into the CSR slots; FPSQ_BAND_FORM=1 sends the formation through k_band_form (row pairs, the CSR of the other columns
    alone) instead of k_band_form_t: both must form B on the band rows and the other columns, not M"""
    case = "m640-r3-c5-param-delta0"
    qp = _qp(case)[0]
    if form == "by-row-pairs":
        monkeypatch.setenv("FPSQ_BAND_FORM", "1")
    r, c, v = _triplets(qp)
    split = np.arange(v.size) % 3 == 0
    v1 = np.where(split, 0.5 * v, v)
    order = np.random.default_rng(4).permutation(v.size + int(split.sum()))
    coo = (np.concatenate([r, r[split]])[order], np.concatenate([c, c[split]])[order], np.concatenate([v1, 0.5 * v[split]])[order])
    h = Raw(qp, ("arrow", 16, 16), coo)
    i = h.info()
    assert (i["border_rows"], i["border_cols"], i["nblocks"], i["nnz"]) == (3, 5, 5, qp.nnz)
    assert h.factorize(0.0) == (0, 0)
    V, W = _blocks(case)
    got = h.two("solve_two_least_squares", V[1].copy(), W[1].copy())
    err = max(_rel(a, b) for a, b in zip(got, _expected(case, "diag")["lsq"][1]))
    print(f"\n{case} with duplicates, formation {form}: {err:.2e}")
    assert h.info()["regularized_pivots"] == 0 and h.info()["last_border_ms"] > 0.0
    assert err < BAR
    h.close()


def test_the_numpy_model_explains_the_device_on_the_643_row_case():
    """the second yardstick: the device's q1 / q2 against tests/arrow_model.py (nested and fused algebra) on the same inputs;
    all three against the dense LU.  Prints the figures of profiles/band_arrow.md."""
    case = "m640-r3-c5-param-delta0"
    qp, rows, cols = _qp(case)
    V, W = _blocks(case)
    model = ArrowModel(qp.scipy_csr(), 0.0, rows, cols)
    want = _expected(case, "diag")["lsq"][1]
    dev = _device(case)
    got = _two(dev, "solve_two_least_squares", V[1].copy(), W[1].copy())
    ratio = dev.info()["border_pivot_ratio"]
    dev.close()
    e_dev = max(_rel(a, b) for a, b in zip(got, want))
    e_nested = max(_rel(a, b) for a, b in zip(model.solve(V[1], W[1], False), want))
    e_fused = max(_rel(a, b) for a, b in zip(model.solve(V[1], W[1], False, fused=True), want))
    print(f"\n{case}: device {e_dev:.2e}, numpy nested {e_nested:.2e}, numpy fused {e_fused:.2e}; pivot ratio {ratio:.4g}, "
          f"numpy's {model.pivot_ratio:.4g}")
    assert e_nested < 1e-12 and e_fused < 1e-12 and e_dev < BAR
