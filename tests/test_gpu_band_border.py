"""Bordered band on the device (fpsq_band_create_bordered, DeviceBorderedBandEqQP): a few long constraint rows are eliminated
last, M = [B C; C' D], and every M-solve is the sweeps on the band B plus the correction w = S^-1 (t - C'y), u = y - Z w.

Yardstick: a DENSE fp64 solve of K = [I A'; A -delta I] (scipy.linalg.lu_factor, once per shape, shared) and the closed forms
of objgrad / hprod of include/fpsq.h (tests/sparse_hessian_ref.py, on that dense factor), at the bar the existing banded tests
hold each entry to: max|a - b| / max|b| < 1e-9 per vector, |phi - phi_exact| <= 1e-9 |phi_exact|, 1e-13 for A x / A'y.
Every call must return 0: a non-zero code is how a raised error word of the sweeps shows.

Shapes.  The selection rule takes a border only when the band of the other rows is at most a quarter as wide in blocks, and
the bands here are 1 - 2 blocks wide, so the smallest band parts at which a border exists at all have 5 blocks (one chain)
and 21 blocks (two chains need m >= 2560): mb = 640 (a multiple of 128), 1500 and 2601 (not multiples); s = 1, 5, 16;
delta = 0 and sqrt(eps); border rows first, last, in the middle of the caller's order and scattered by a shuffle of all rows
(which also makes the symbolic phase reorder the band rows by reverse Cuthill-McKee)."""
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
from fps_amd import _lib, problems  # noqa: E402
from fps_amd.device_qp import DeviceBandEqQP, DeviceBorderedBandEqQP  # noqa: E402
from sparse_hessian_ref import SparseHessianRef  # noqa: E402

pytestmark = pytest.mark.gpu

SE = float(np.sqrt(np.finfo(float).eps))
SIGMA = 1e3
BAR = 1e-9


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def _reordered(qp, order):
    """row p of the result = row order[p] of qp"""
    A = sp.csr_matrix(qp.scipy_csr()[order])
    A.sort_indices()
    return dataclasses.replace(qp, rowptr=A.indptr.astype(np.int32), colind=A.indices.astype(np.int32), vals=A.data.copy(),
                               b=qp.b[order])


def _placed(qp0, s, where, seed=9):
    """qp0 with s mean-value rows; `where` they sit in the caller's order.  Returns (qp, indices of the long rows)"""
    qp = problems.with_border_rows(qp0, s, kind="mean", seed=seed)
    m0 = qp0.m
    if where == "last":
        order = np.arange(qp.m)
    elif where == "first":
        order = np.concatenate([np.arange(m0, qp.m), np.arange(m0)])
    elif where == "middle":
        order = np.concatenate([np.arange(m0 // 2), np.arange(m0, qp.m), np.arange(m0 // 2, m0)])
    else:
        order = np.random.default_rng(seed).permutation(qp.m)
    return _reordered(qp, order), np.sort(np.nonzero(order >= m0)[0])


def _p640():
    return problems.pde_control_like(n=3000, m=640, per_row=12, window=256, seed=5)


def _p1500():
    return problems.pde_control_like(n=3600, m=1500, per_row=12, window=256, seed=6)


# name: (band part, s, where, delta, expected info of the bordered handle)
CASES = {
    "mb640-s5-first-delta0": (_p640, 5, "first", 0.0, {"nblocks": 5, "chains": 1}),
    "mb640-s16-last": (_p640, 16, "last", SE, {"nblocks": 5, "chains": 1}),
    "mb1500-s1-middle": (_p1500, 1, "middle", SE, {"nblocks": 12, "chains": 1}),
    # (all rows shuffled: the natural band of the 1500 band rows is full, 11 blocks; 2 only after reverse Cuthill-McKee)
    "mb1500-s5-shuffled-delta0": (_p1500, 5, "shuffled", 0.0, {"nblocks": 12, "chains": 1, "bandwidth_blocks": 2}),
    "aug2dc-two-chains-s16": (lambda: problems.aug2dc_like(N=51), 16, "last", SE, {"nblocks": 21, "chains": 2}),
}
KMAX = 9


@functools.lru_cache(maxsize=None)
def _qp(case, model="diag"):
    make, s, where, _, _ = CASES[case]
    qp, rows = _placed(make(), s, where)
    if model != "diag":
        qp = problems.with_sparse_hessian(qp, 2, 11)
    return qp, rows


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


@functools.lru_cache(maxsize=None)
def _dense_lu(case, delta):
    qp, _ = _qp(case)
    A = qp.scipy_csr().toarray()
    K = np.block([[np.eye(qp.n), A.T], [A, -float(delta) * np.eye(qp.m)]])
    return sla.lu_factor(K, overwrite_a=True, check_finite=False)


def _ref(case, model="diag", delta=None):
    delta = CASES[case][3] if delta is None else delta
    return DenseRef(_qp(case, model)[0], _dense_lu(case, delta))


@functools.lru_cache(maxsize=None)
def _blocks(case):
    qp, _ = _qp(case)
    rng = np.random.default_rng(1234)
    V, W = rng.standard_normal((KMAX, qp.n)), rng.standard_normal((KMAX, qp.n))
    V.setflags(write=False)
    W.setflags(write=False)
    return V, W


def _device(case, model="diag", rho=1.0, eta=0.5, border=16, **kw):
    qp, _ = _qp(case, model)
    dev = DeviceBorderedBandEqQP(qp, border=border, sigma=SIGMA, rho=rho, delta=CASES[case][3], eta=eta, **kw)
    info = dev.info()
    if border:
        assert info["border_rows"] == CASES[case][1], info
        for k, v in CASES[case][4].items():
            assert info[k] == v, (k, info)
    else:
        assert info["border_rows"] == 0
    return dev


def _objgrad(dev, x, xk):
    qp = dev.qp
    gx, ys, gs = np.full(qp.n, np.nan), np.full(qp.m, np.nan), np.full(qp.n, np.nan)
    fx, rc = dev.objgrad(x, gx=gx, ys=ys, gs=gs, xk=xk)
    assert rc == 0
    return fx, gx, ys, gs


def _two(dev, name, rhs1, rhs2):
    """fpsq_band_solve_two_mixed / _least_squares on the object's handle"""
    qp = dev.qp
    assert dev._factor() == 0
    p1, q1, p2, q2 = np.full(qp.n, np.nan), np.full(qp.m, np.nan), np.full(qp.n, np.nan), np.full(qp.m, np.nan)
    rc = getattr(dev._lib, f"fpsq_band_{name}")(dev._h, rhs1.ctypes.data, rhs2.ctypes.data, p1.ctypes.data, q1.ctypes.data,
                                                p2.ctypes.data, q2.ctypes.data)
    assert rc == 0, dev._lib.fpsq_band_last_error(dev._h)
    return p1, q1, p2, q2


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
def test_every_entry_on_a_bordered_handle_matches_the_dense_kkt_solve(case):
    qp, rows = _qp(case)
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
    # A x and A'y in the caller's row order
    A = qp.scipy_csr()
    u = np.random.default_rng(2).standard_normal(qp.m)
    y, z = np.zeros(qp.m), np.empty(qp.n)
    assert dev.jac_mul(0, 1.0, qp.x, 0.0, y) == 0 and dev.jac_mul(1, 1.0, u, 0.0, z) == 0
    errs["jac_mul"] = max(_rel(y, A @ qp.x), _rel(z, A.T @ u)) * (BAR / 1e-13)   # (held to 1e-13)
    info = dev.info()
    print(f"\n{case}: border {info['border_rows']}, last_border_ms {info['last_border_ms']:.3f}, "
          f"worst {max(errs.values()):.2e}: {errs}")
    assert info["last_border_ms"] > 0.0 and info["regularized_pivots"] == 0 and info["factorizations"] == 1
    assert max(errs.values()) < BAR, errs
    dev.close()


class Raw:
    """a handle through the C entries themselves: `entry` = "plain" (fpsq_band_create) or a max_border
    (fpsq_band_create_bordered); no regularisation unless `reg`"""

    def __init__(self, qp, entry, reg=None):
        self.lib, self.qp = _lib.load(), qp
        rp = np.ascontiguousarray(qp.rowptr, dtype=np.int32)
        ci = np.ascontiguousarray(qp.colind, dtype=np.int32)
        h = C.c_void_p()
        if entry == "plain":
            rc = self.lib.fpsq_band_create(C.byref(h), qp.n, qp.m, rp.ctypes.data, ci.ctypes.data, 0)
        else:
            rc = self.lib.fpsq_band_create_bordered(C.byref(h), qp.n, qp.m, rp.ctypes.data, ci.ctypes.data, int(entry), 0)
        assert rc == 0, self.lib.fpsq_band_last_error(None)
        self.h, self.q = h, None
        if reg is not None:
            assert self.lib.fpsq_band_set_regularization(h, reg[0], reg[1]) == 0

    def factorize(self, delta, vals=None):
        pivot = C.c_int32(-7)
        vals = np.ascontiguousarray(self.qp.vals if vals is None else vals)
        return self.lib.fpsq_band_factorize(self.h, vals.ctypes.data, float(delta), C.byref(pivot)), pivot.value

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

    def info(self):
        i = _lib.BandInfo()
        assert self.lib.fpsq_band_get_info(self.h, C.byref(i)) == 0
        return i.as_dict()

    def close(self):
        if self.q:
            self.lib.fpsq_band_qp_destroy(self.q)
        assert self.lib.fpsq_band_destroy(self.h) == 0


def test_max_border_zero_through_the_new_entries_is_bitwise_the_existing_entries():
    """on the problem WITH long rows (a wide band, as the existing entries store it) and on one without"""
    for qp in (_qp("mb640-s5-first-delta0")[0], _p640()):
        V = np.random.default_rng(5).standard_normal((9, qp.n))
        outs = []
        for entry in ("plain", 0):
            r = Raw(qp, entry)
            assert r.factorize(SE) == (0, 0)
            r.model()
            rc, fx, gx, ys, gs = r.objgrad(qp.x)
            rc2, HV = r.hprod_block(V)
            assert rc == 0 and rc2 == 0
            i = r.info()
            assert i["border_rows"] == 0 and i["last_border_ms"] == 0.0
            outs.append((np.float64(fx), gx, ys, gs, HV, {k: i[k] for k in ("nblocks", "bandwidth_blocks", "factor_bytes",
                                                                           "reordered", "chains", "nnz")}))
            r.close()
        for a, b in zip(outs[0][:5], outs[1][:5]):
            assert np.array_equal(a, b)
        assert outs[0][5] == outs[1][5]


def test_repeat_calls_and_block_columns_are_bitwise_stable():
    case = "mb1500-s5-shuffled-delta0"
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
    dev.close()


def _exactly_singular():
    """Band rows with four entries +-1 in columns of their own (B = 4 I: the factor, its inverse and every sum below are exact
    in fp64) and ONE long row that is the sum of all band rows: M is singular and S = D - C'Z = 2560 - 640 * 4 * 1 is an EXACT
    zero, not a rounding residue of either sign.  (A copy of a single band row would be as narrow as that row and never be a
    border candidate; a dependent row has to be long to end up in the border.)  The long row sits at index 100."""
    mb, at = 640, 100
    n = 4 * mb
    sign = np.where((np.arange(n) * 7) % 3 == 0, -1.0, 1.0)
    A = sp.vstack([sp.csr_matrix((sign, (np.repeat(np.arange(mb), 4), np.arange(n))), shape=(mb, n)),
                   sp.csr_matrix(sign[None, :])]).tocsr()
    order = np.concatenate([np.arange(at), [mb], np.arange(at, mb)])
    A = sp.csr_matrix(A[order])
    A.sort_indices()
    xhat = np.linspace(-1.0, 1.0, n)
    return problems.EqQP("exactly-singular", n, mb + 1, A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy(),
                         np.linspace(1.0, 2.0, n), np.ones(n), A @ xhat, xhat + 0.1, xhat), at


def test_singular_border_without_regularisation_reports_the_border_row():
    qp, at = _exactly_singular()
    r = Raw(qp, 1)
    assert r.info()["border_rows"] == 1 and r.info()["bandwidth_blocks"] == 0
    rc, pivot = r.factorize(0.0)
    assert (rc, pivot) == (1, at + 1)                                     # soft code, the row 1-based in the caller's order
    r.model()
    assert r.objgrad(qp.x)[0] == -3                                       # FPSQ_ERR_STATE
    assert r.hprod_block(np.ones((2, qp.n)))[0] == -3
    p = np.empty(qp.n)
    q = np.empty(qp.m)
    assert r.lib.fpsq_band_solve_two_least_squares(r.h, qp.x.ctypes.data, qp.x.ctypes.data, p.ctypes.data, q.ctypes.data,
                                                   p.ctypes.data, q.ctypes.data) == -3
    assert b"no valid factorisation" in r.lib.fpsq_band_last_error(r.h)
    assert r.factorize(1e-3) == (0, 0)                                    # delta > 0: positive definite again
    assert r.objgrad(qp.x)[0] == 0
    r.close()


def test_singular_border_with_the_default_regularisation_is_regularised():
    qp, _ = _exactly_singular()
    dev = DeviceBorderedBandEqQP(qp, border=1, sigma=SIGMA, rho=1.0, delta=0.0)
    fx, gx, ys, gs = _objgrad(dev, qp.x, None)
    i = dev.info()
    assert i["border_rows"] == 1 and i["regularized_pivots"] >= 1
    assert np.isfinite(fx) and all(np.all(np.isfinite(a)) for a in (gx, ys, gs))
    Hv = np.full(qp.n, np.nan)
    assert dev.hprod(qp.x, Hv) == 0 and np.all(np.isfinite(Hv))
    dev.close()


def test_refactorisation_follows_new_values_and_delta_like_a_fresh_handle():
    import torch

    case = "mb640-s16-last"
    qp, _ = _qp(case)
    on = torch.device("cuda", 0)
    dev = _device(case)
    before = _objgrad(dev, qp.x, qp.xhat)
    new_vals = qp.vals * (1.0 + 0.25 * np.cos(np.arange(qp.nnz)))
    big = torch.rand(2048, 2048, dtype=torch.float64, device=on)
    for _ in range(3):                                                    # the values are still being produced at the call
        big = big @ big * 1e-3
    dev.set_jacobian_values(torch.from_numpy(new_vals).to(on) * 1.0)
    dev.set_delta(1e-3)
    after = _objgrad(dev, qp.x, qp.xhat)
    assert dev.info()["factorizations"] == 2 and not np.array_equal(after[1], before[1])
    fresh_qp = dataclasses.replace(qp, vals=new_vals)
    fresh = DeviceBorderedBandEqQP(fresh_qp, border=16, sigma=SIGMA, rho=1.0, delta=1e-3, eta=0.5)
    want = _objgrad(fresh, qp.x, qp.xhat)
    for a, b in zip(after, want):
        assert np.array_equal(a, b)
    e = DenseRef(fresh_qp, _dense_lu_of(fresh_qp, 1e-3)).objgrad(qp.x, SIGMA, 1.0, 0.5, qp.xhat)
    assert _rel(after[1], e["gx"]) < BAR and _rel(after[2], e["ys"]) < BAR and abs(after[0] - e["fx"]) <= BAR * abs(e["fx"])
    fresh.close()
    dev.close()


def _dense_lu_of(qp, delta):
    A = qp.scipy_csr().toarray()
    K = np.block([[np.eye(qp.n), A.T], [A, -float(delta) * np.eye(qp.m)]])
    return sla.lu_factor(K, overwrite_a=True, check_finite=False)


def test_device_tensors_on_a_registered_stream_give_the_bits_of_host_arrays():
    import torch

    case = "mb1500-s1-middle"
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
    dev.close()


def test_the_per_step_sweeps_take_the_same_correction(monkeypatch):
    """FPSQ_TRSV_CHAIN=0 (one launch per step of the sweeps) on a bordered handle: the same algebra, another summation order"""
    case = "aug2dc-two-chains-s16"
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


def test_fps_solve_device_on_a_bordered_handle_agrees_with_the_wide_band_handle():
    import torch

    from fps_amd.fps_solve import fps_solve_device

    case = "mb640-s5-first-delta0"
    qp, _ = _qp(case)
    on = torch.device("cuda", 0)
    res = {}
    for name, border in (("bordered", 16), ("wide", 0)):
        dev = DeviceBorderedBandEqQP(qp, border=border)
        assert dev.info()["border_rows"] == (5 if border else 0)
        stats = fps_solve_device(dev, torch.from_numpy(qp.x).to(on), max_time=120)
        res[name] = (stats.status, stats.solution.cpu().numpy(), stats.multipliers.cpu().numpy())
        dev.close()
    print(f"\n{case}: {res['bordered'][0]} / {res['wide'][0]}, |dx|/|x| = "
          f"{np.linalg.norm(res['bordered'][1] - res['wide'][1]) / np.linalg.norm(res['wide'][1]):.2e}")
    assert res["bordered"][0] == res["wide"][0] == "first_order"
    ref = SparseHessianRef(qp, 0.0)
    xstar, lam = ref.kkt_point()
    for name in res:                                                      # the bounds of the existing banded outer-loop tests
        assert np.linalg.norm(res[name][1] - xstar) <= 1e-6 * np.linalg.norm(xstar), name
        assert np.linalg.norm(res[name][2] - lam) <= 1e-5 * max(1.0, np.linalg.norm(lam)), name
    assert np.linalg.norm(res["bordered"][1] - res["wide"][1]) <= 2e-6 * np.linalg.norm(xstar)


def test_the_coo_entry_behind_the_qdsolver_seam_takes_the_same_border():
    """HIPBandedDirectQDSolver(border=16) (fpsq_band_create_coo_bordered, fpsq_band_factorize_coo) behind FletcherPenaltyNLP
    against fpsq_band_qp_objgrad on the CSR entry: the same border and factor, other summation orders in the products --
    1e-12 relative, the bar of the existing seam test."""
    from fps_amd import nlpmodels
    from fps_amd.penalty_nlp import FletcherPenaltyNLP
    from fps_amd.qdsolver import HIPBandedDirectQDSolver

    case = "mb1500-s5-shuffled-delta0"
    qp, _ = _qp(case)
    model = nlpmodels.EqQPModel(qp)
    qds = HIPBandedDirectQDSolver(model, 0.0, border=16)
    assert qds.info()["border_rows"] == 5 and qds.info()["nblocks"] == 12
    fp = FletcherPenaltyNLP(model, SIGMA, 1.0, 0.0, 2, qds=qds)
    f_seam, g_seam = fp.objgrad(qp.x)
    dev = _device(case, rho=1.0, eta=0.0)
    fx, gx, ys, gs = _objgrad(dev, qp.x, None)
    assert abs(fx - f_seam) <= 1e-12 * abs(f_seam)
    assert _rel(gx, g_seam) < 1e-12 and _rel(ys, fp.ys) < 1e-12 and _rel(gs, fp.gs) < 1e-12
    plain = HIPBandedDirectQDSolver(model, 0.0)
    assert plain.info()["border_rows"] == 0
    plain.close()
    qds.close()
    dev.close()
