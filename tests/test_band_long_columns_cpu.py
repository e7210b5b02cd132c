"""The symbolic phase of the band with long columns (fpsq_band_analyze_bordered_cols: host only, no device), the generator of
long columns and a numpy restatement of the low-rank scheme.  A variable that appears in constraints all over the row range
is a long column of A and makes M = A A' + delta I structurally dense; the entries with max_cols take such columns out of the
band, M = B + U U' (include/fpsq.h "LONG COLUMNS")."""
import ctypes as C
import dataclasses
import inspect
import os
import sys

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(__file__))
import fps_amd  # noqa: E402,F401
from fps_amd import _lib, nlpmodels, problems, qdsolver  # noqa: E402
from long_columns_model import LongColumnsModel  # noqa: E402


def _analyze(qp, max_cols, max_border=0, entry="cols"):
    lib = _lib.load()
    rp = np.ascontiguousarray(qp.rowptr, dtype=np.int32)
    ci = np.ascontiguousarray(qp.colind, dtype=np.int32)
    perm = np.full(qp.m, -1, dtype=np.int32)
    long_cols = np.full(16, -7, dtype=np.int32)
    info = _lib.BandInfo()
    if entry == "cols":
        rc = lib.fpsq_band_analyze_bordered_cols(qp.n, qp.m, rp.ctypes.data, ci.ctypes.data, max_border, max_cols,
                                                 perm.ctypes.data, long_cols.ctypes.data, C.byref(info))
    else:
        rc = lib.fpsq_band_analyze(qp.n, qp.m, rp.ctypes.data, ci.ctypes.data, perm.ctypes.data, C.byref(info))
    return rc, perm, long_cols, info.as_dict()


BASES = {
    "pde": lambda: problems.pde_control_like(n=20000, m=2000, per_row=40, window=1024, seed=3),
    "aug2dc": lambda: problems.aug2dc_like(N=51),
}
SHAPE = ("bandwidth_blocks", "nblocks", "chains", "reordered", "factor_bytes")


def _columns_moved(qp, new_of_old):
    """column c of qp becomes column new_of_old[c]"""
    A = qp.scipy_csr().tocoo()
    B = sp.csr_matrix((A.data, (A.row, new_of_old[A.col])), shape=A.shape)
    B.sort_indices()
    inv = np.argsort(new_of_old)
    return dataclasses.replace(qp, rowptr=B.indptr.astype(np.int32), colind=B.indices.astype(np.int32), vals=B.data.copy(),
                               qdiag=qp.qdiag[inv], d=qp.d[inv], xhat=qp.xhat[inv], x=qp.x[inv])


@pytest.mark.parametrize("kind", ["param", "stride"])
@pytest.mark.parametrize("s", [1, 5, 16])
@pytest.mark.parametrize("base", list(BASES))
def test_long_columns_are_detected_and_the_band_is_the_one_without_them(base, s, kind):
    qp0 = BASES[base]()
    qp = problems.with_long_columns(qp0, s, kind=kind, seed=7)
    rc0, perm0, _, i0 = _analyze(qp0, 0, entry="plain")
    rc, perm, lc, i = _analyze(qp, 16)
    assert rc0 == 0 and rc == 0
    assert i["border_cols"] == s and i["border_rows"] == 0 and i["border_pivot_ratio"] == 1.0
    assert np.array_equal(lc[:s], qp0.n + np.arange(s)) and np.all(lc[s:] == -1)     # the appended columns, ascending
    for k in SHAPE:
        assert i[k] == i0[k], (k, i, i0)
    assert (i["n"], i["m"], i["nnz"]) == (qp.n, qp.m, qp.nnz)
    assert np.array_equal(perm, perm0)                                    # the ordering of the rows on the other columns
    # with max_cols = 0 a column that couples rows all over the range keeps the band at least half the matrix wide
    rc, _, lc, full = _analyze(qp, 0)
    assert rc == 0 and full["border_cols"] == 0 and np.all(lc == -1)
    assert full["bandwidth_blocks"] >= max((full["nblocks"] - 1) // 2, 4 * i["bandwidth_blocks"])


def test_nothing_to_take_is_the_plain_handle():
    qp0 = BASES["pde"]()

    def same_as_plain(qp, max_cols):
        rc_a, perm_a, _, info_a = _analyze(qp, 0, entry="plain")
        rc, perm, lc, info = _analyze(qp, max_cols)
        assert rc == 0 and rc_a == 0 and info["border_cols"] == 0 and np.all(lc == -1)
        assert info == info_a and np.array_equal(perm, perm_a)
        return info

    same_as_plain(qp0, 16)                                                # a base problem without long columns
    same_as_plain(problems.pde_control_like(n=30000, m=7700, per_row=12, window=600, seed=11), 16)   # two chains, reordered
    # 17 long columns with max_cols = 16: no prefix of the candidates narrows the band, so NOTHING is taken, not a part
    full = same_as_plain(problems.with_long_columns(qp0, 17, seed=4), 16)
    assert full["bandwidth_blocks"] >= (full["nblocks"] - 1) // 2
    same_as_plain(problems.with_long_columns(qp0, 5, seed=4), 4)          # fewer candidates than long columns
    # rule (a): a row whose only entry lies in a long column would leave B structurally singular
    qp = problems.with_long_columns(qp0, 1, seed=4)
    A = qp.scipy_csr().tolil()
    A[700, :qp0.n] = 0.0
    A = sp.csr_matrix(A)
    A.eliminate_zeros()
    A.sort_indices()
    assert A[700].nnz == 1 and A[700].indices[0] == qp0.n
    lonely = dataclasses.replace(qp, rowptr=A.indptr.astype(np.int32), colind=A.indices.astype(np.int32), vals=A.data.copy())
    same_as_plain(lonely, 16)


@pytest.mark.parametrize("where", ["first", "middle"])
def test_long_columns_anywhere_in_the_callers_order_are_found_by_index(where):
    qp0 = BASES["aug2dc"]()
    s = 5
    qp = problems.with_long_columns(qp0, s, kind="stride", seed=2)
    at = 0 if where == "first" else qp0.n // 2
    new_of_old = np.concatenate([np.arange(at), np.arange(at + s, qp.n), at + np.arange(s)])   # old column -> new
    moved = _columns_moved(qp, new_of_old)
    assert np.allclose(moved.scipy_csr() @ moved.xhat, moved.b, rtol=0, atol=1e-12)
    _, perm0, _, i0 = _analyze(qp0, 0, entry="plain")
    rc, perm, lc, i = _analyze(moved, 8)
    assert rc == 0 and i["border_cols"] == s
    assert np.array_equal(lc[:s], at + np.arange(s)) and np.all(lc[s:] == -1)
    assert np.array_equal(perm, perm0) and all(i[k] == i0[k] for k in SHAPE)


def test_bad_max_cols_and_both_borders_are_argument_errors():
    qp = BASES["aug2dc"]()
    lib = _lib.load()
    h = C.c_void_p()
    rp = np.ascontiguousarray(qp.rowptr, dtype=np.int32)
    ci = np.ascontiguousarray(qp.colind, dtype=np.int32)
    rows = np.zeros(1, dtype=np.int64)
    for max_border, max_cols in ((0, -1), (0, 17), (1, 1), (16, 16)):
        rc, _, _, _ = _analyze(qp, max_cols, max_border)
        assert rc == -1 and b"max_cols" in lib.fpsq_band_last_error(None)
        # (refused before a device is looked for)
        assert lib.fpsq_band_create_bordered_cols(C.byref(h), qp.n, qp.m, rp.ctypes.data, ci.ctypes.data, max_border, max_cols,
                                                  0) == -1
        assert b"max_cols" in lib.fpsq_band_last_error(None)
        assert lib.fpsq_band_create_coo_bordered_cols(C.byref(h), qp.n, qp.m, 1, rows.ctypes.data, rows.ctypes.data, 0,
                                                      max_border, max_cols, 0) == -1
        assert b"max_cols" in lib.fpsq_band_last_error(None)
    rc, _, _, _ = _analyze(qp, 16, 16)
    assert b"one kind" in lib.fpsq_band_last_error(None)


@pytest.mark.parametrize("kind", ["param", "stride"])
def test_with_long_columns_appends_columns_and_keeps_xhat_feasible(kind):
    qp0 = problems.pde_control_like(n=4000, m=400, per_row=16, window=512, seed=21)
    for s in (1, 5, 16):
        qp = problems.with_long_columns(qp0, s, kind=kind, seed=5)
        assert (qp.n, qp.m) == (qp0.n + s, qp0.m) and qp.rowptr.shape == (qp.m + 1,)
        for a in (qp.qdiag, qp.d, qp.xhat, qp.x):
            assert a.shape == (qp.n,)
        assert qp.rowptr.dtype == np.int32 and qp.colind.dtype == np.int32 and qp.vals.dtype == np.float64
        assert qp.rowptr[0] == 0 and qp.rowptr[-1] == qp.colind.size == qp.vals.size
        A = qp.scipy_csr()
        assert np.allclose(A @ qp.xhat, qp.b, rtol=0, atol=1e-12)
        assert (abs(A[:, :qp0.n] - qp0.scipy_csr())).nnz == 0             # the base columns are untouched
        for a, a0 in ((qp.qdiag, qp0.qdiag), (qp.d, qp0.d), (qp.xhat, qp0.xhat), (qp.x, qp0.x)):
            assert np.array_equal(a[:qp0.n], a0)
        idx = qp0.n + np.arange(s)
        assert np.array_equal(qp.qdiag[qp0.n:], 1.0 + 9.0 * problems.uniform01(5, idx, 1))
        assert np.array_equal(qp.xhat[qp0.n:], 2.0 * problems.uniform01(5, idx, 3) - 1.0)
        for r in range(qp.m):                                             # sorted, distinct columns in range
            c = qp.colind[qp.rowptr[r]:qp.rowptr[r + 1]]
            assert c.size > 0 and c.min() >= 0 and c.max() < qp.n and np.all(np.diff(c) > 0)
        Ac = A.tocsc()
        for j in range(s):
            col = Ac[:, qp0.n + j]
            want = np.arange(qp.m) if kind == "param" else np.arange(j % 4, qp.m, 4)
            assert np.array_equal(np.sort(col.indices), want)
            v = np.asarray(col.todense()).ravel()[want]
            assert np.array_equal(v, (0.5 + problems.uniform01(5, j * qp.m + want, 41)) / np.sqrt(want.size))
        again = problems.with_long_columns(qp0, s, kind=kind, seed=5)
        assert np.array_equal(again.vals, qp.vals) and np.array_equal(again.colind, qp.colind) and np.array_equal(again.b, qp.b)
    with pytest.raises(ValueError):
        problems.with_long_columns(qp0, 1, kind="dense")


def test_python_surface_forwards_cols():
    from fps_amd.device_qp import DeviceBandEqQP, DeviceBorderedBandEqQP

    assert DeviceBandEqQP.cols == 0 and DeviceBandEqQP.border == 0
    params = inspect.signature(DeviceBorderedBandEqQP.__init__).parameters
    assert list(params)[1:4] == ["qp", "border", "cols"] and params["border"].default == 16 and params["cols"].default == 0
    assert inspect.signature(qdsolver.HIPBandedDirectQDSolver.__init__).parameters["cols"].default == 0
    assert inspect.signature(qdsolver.band_analysis).parameters["cols"].default == 0
    fields = [f for f, _ in _lib.BandInfo._fields_]
    assert fields[-2:] == ["border_cols", "border_pivot_ratio"]
    qp0 = BASES["aug2dc"]()
    model = nlpmodels.EqQPModel(problems.with_long_columns(qp0, 3, seed=1))
    plain, taken = qdsolver.band_analysis(model), qdsolver.band_analysis(model, cols=16)
    base = qdsolver.band_analysis(nlpmodels.EqQPModel(qp0))
    assert plain["border_cols"] == 0 and plain["bandwidth_blocks"] >= (plain["nblocks"] - 1) // 2
    assert taken["border_cols"] == 3 and taken["bandwidth_blocks"] == base["bandwidth_blocks"]
    assert qdsolver.band_analysis(model, border=16, cols=16) is None      # one kind per handle


def test_the_numpy_restatement_of_the_scheme_meets_the_dense_kkt_solve():
    """pins the algebra before any kernel runs: M^-1 r = y - Z w with the long columns' rows of A'q taken as w, against a dense
    LU of K = [I A'; A -delta I], on the 640-row shape of the device tests (s = 5 all-row columns, delta = 0)"""
    qp0 = problems.pde_control_like(n=3000, m=640, per_row=12, window=256, seed=5)
    qp = problems.with_long_columns(qp0, 5, kind="param", seed=9)
    A = qp.scipy_csr()
    Ad = A.toarray()
    lu = sla.lu_factor(np.block([[np.eye(qp.n), Ad.T], [Ad, np.zeros((qp.m, qp.m))]]), check_finite=False)
    model = LongColumnsModel(A, 0.0, qp0.n + np.arange(5))
    assert model.pivot_ratio >= 1.0
    rng = np.random.default_rng(7)
    r1, r2, c = rng.standard_normal(qp.n), rng.standard_normal(qp.n), rng.standard_normal(qp.m)
    rel = lambda a, b: float(np.max(np.abs(a - b)) / np.max(np.abs(b)))  # noqa: E731
    worst = 0.0
    for mixed, second in ((True, c), (False, r2)):
        got = model.solve(r1, second, mixed)
        s1 = sla.lu_solve(lu, np.concatenate([r1, np.zeros(qp.m)]))
        s2 = sla.lu_solve(lu, np.concatenate([np.zeros(qp.n), second] if mixed else [second, np.zeros(qp.m)]))
        # K [p; q] = [r; 0] gives q = M^-1 A r;  K [p; q] = [0; c] gives q = -M^-1 c, the mixed entry's q2
        want = (s1[:qp.n], s1[qp.n:], s2[:qp.n], s2[qp.n:])
        worst = max(worst, max(rel(a, b) for a, b in zip(got, want)))
    print(f"\nnumpy model of the long-column scheme against the dense LU: worst relative error {worst:.2e}")
    assert worst < 1e-12
