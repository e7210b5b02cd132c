"""The symbolic phase of the ARROW band (fpsq_band_analyze_arrow: host only, no device): border rows and long columns on one
handle, the selection rule of include/fpsq.h "ARROW BAND" with its four reductions to the existing entries, the generator
`problems.with_arrow` and the numpy restatement of the scheme (tests/arrow_model.py)."""
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
from arrow_model import ArrowModel  # noqa: E402
from fps_amd import _lib, nlpmodels, problems, qdsolver  # noqa: E402

ENTRIES = {"arrow": "fpsq_band_analyze_arrow", "cols": "fpsq_band_analyze_bordered_cols"}


def _analyze(qp, max_border, max_cols, entry="arrow"):
    lib = _lib.load()
    rp = np.ascontiguousarray(qp.rowptr, dtype=np.int32)
    ci = np.ascontiguousarray(qp.colind, dtype=np.int32)
    perm = np.full(qp.m, -1, dtype=np.int32)
    long_cols = np.full(16, -7, dtype=np.int32)
    info = _lib.BandInfo()
    if entry == "plain":
        rc = lib.fpsq_band_analyze(qp.n, qp.m, rp.ctypes.data, ci.ctypes.data, perm.ctypes.data, C.byref(info))
        long_cols[:] = -1
    elif entry == "bordered":
        rc = lib.fpsq_band_analyze_bordered(qp.n, qp.m, rp.ctypes.data, ci.ctypes.data, max_border, perm.ctypes.data,
                                            C.byref(info))
        long_cols[:] = -1
    else:
        rc = getattr(lib, ENTRIES[entry])(qp.n, qp.m, rp.ctypes.data, ci.ctypes.data, max_border, max_cols, perm.ctypes.data,
                                          long_cols.ctypes.data, C.byref(info))
    return rc, perm, long_cols, info.as_dict()


BASES = {
    "pde": lambda: problems.pde_control_like(n=20000, m=2000, per_row=40, window=1024, seed=3),
    "aug2dc": lambda: problems.aug2dc_like(N=51),
}
SHAPE = ("bandwidth_blocks", "nblocks", "chains", "reordered", "factor_bytes")


def _small():
    """the 640-row band part of the device tests: 5 blocks, the fewest at which either rule can take anything"""
    return problems.pde_control_like(n=3000, m=640, per_row=12, window=256, seed=5)


def _columns_moved(qp, new_of_old):
    """column c of qp becomes column new_of_old[c]"""
    A = qp.scipy_csr().tocoo()
    B = sp.csr_matrix((A.data, (A.row, new_of_old[A.col])), shape=A.shape)
    B.sort_indices()
    inv = np.argsort(new_of_old)
    return dataclasses.replace(qp, rowptr=B.indptr.astype(np.int32), colind=B.indices.astype(np.int32), vals=B.data.copy(),
                               qdiag=qp.qdiag[inv], d=qp.d[inv], xhat=qp.xhat[inv], x=qp.x[inv])


def _rows_shuffled(qp, order):
    """row p of the result is row order[p] of qp"""
    A = sp.csr_matrix(qp.scipy_csr()[order])
    A.sort_indices()
    return dataclasses.replace(qp, rowptr=A.indptr.astype(np.int32), colind=A.indices.astype(np.int32), vals=A.data.copy(),
                               b=qp.b[order])


def _same(a, b):
    """two analyses, bit for bit: the code, row_perm, long_cols and every field of info"""
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]


@pytest.mark.parametrize("kind", ["param", "stride"])
@pytest.mark.parametrize("s_rows,s_cols", [(1, 1), (3, 5), (16, 16)])
@pytest.mark.parametrize("base", list(BASES))
def test_both_kinds_are_detected_and_the_band_is_the_one_without_them(base, s_rows, s_cols, kind):
    qp0 = BASES[base]()
    qp = problems.with_arrow(qp0, s_rows, s_cols, col_kind=kind, seed=7)
    rc0, perm0, _, i0 = _analyze(qp0, 0, 0, "plain")
    rc, perm, lc, i = _analyze(qp, 16, 16)
    assert rc0 == 0 and rc == 0
    assert i["border_rows"] == s_rows and i["border_cols"] == s_cols and i["border_pivot_ratio"] == 1.0
    assert np.array_equal(lc[:s_cols], qp0.n + np.arange(s_cols)) and np.all(lc[s_cols:] == -1)   # the appended columns
    assert np.array_equal(np.sort(perm), np.arange(qp.m))                 # a permutation ...
    assert np.array_equal(perm[-s_rows:], qp0.m + np.arange(s_rows))      # ... with the appended rows last, ascending ...
    assert np.array_equal(perm[:qp0.m], perm0)                            # ... behind the base problem's own ordering
    for k in SHAPE:
        assert i[k] == i0[k], (k, i, i0)
    assert (i["n"], i["m"], i["nnz"]) == (qp.n, qp.m, qp.nnz)
    if (s_rows, s_cols) != (3, 5):                                        # (once per base and kind is enough)
        return
    # either kind alone leaves the band at least half the matrix wide: the existing entries gain nothing on this pattern
    for entry, mb, mc in (("bordered", 16, 0), ("cols", 0, 16)):
        rc, _, _, one = _analyze(qp, mb, mc, entry)
        assert rc == 0 and one["border_rows"] == 0 and one["border_cols"] == 0
        assert one["bandwidth_blocks"] >= max((one["nblocks"] - 1) // 2, 4 * i["bandwidth_blocks"])


@pytest.mark.parametrize("where", ["first", "middle"])
@pytest.mark.parametrize("base", list(BASES))
def test_long_columns_anywhere_in_the_column_order_and_all_rows_shuffled(base, where):
    qp0 = BASES[base]()
    s_rows, s_cols = 3, 5
    qp = problems.with_arrow(qp0, s_rows, s_cols, col_kind="stride", seed=2)
    at = 0 if where == "first" else qp0.n // 2
    new_of_old = np.concatenate([np.arange(at), np.arange(at + s_cols, qp.n), at + np.arange(s_cols)])   # old column -> new
    moved = _columns_moved(qp, new_of_old)
    assert np.allclose(moved.scipy_csr() @ moved.xhat, moved.b, rtol=0, atol=1e-12)
    _, perm0, _, i0 = _analyze(qp0, 0, 0, "plain")
    rc, perm, lc, i = _analyze(moved, 16, 16)
    assert rc == 0 and (i["border_rows"], i["border_cols"]) == (s_rows, s_cols)
    assert np.array_equal(lc[:s_cols], at + np.arange(s_cols)) and np.all(lc[s_cols:] == -1)
    assert np.array_equal(perm[-s_rows:], qp0.m + np.arange(s_rows)) and np.array_equal(perm[:qp0.m], perm0)
    assert all(i[k] == i0[k] for k in SHAPE), (i, i0)
    # all rows shuffled, the long ones among them: the band is the one of the base problem's rows shuffled the same way
    order = np.random.default_rng(3).permutation(qp.m)
    shuffled = _rows_shuffled(moved, order)
    where_long = np.sort(np.nonzero(order >= qp0.m)[0])                   # the long rows in the shuffled numbering
    base_rows = order[order < qp0.m]                                      # the band rows in the order the shuffle leaves them
    _, _, _, ib = _analyze(_rows_shuffled(qp0, base_rows), 0, 0, "plain")
    rc, perm, lc, i = _analyze(shuffled, 16, 16)
    assert rc == 0 and (i["border_rows"], i["border_cols"]) == (s_rows, s_cols) and i["reordered"] == 1
    assert np.array_equal(np.sort(perm), np.arange(qp.m)) and np.array_equal(perm[-s_rows:], where_long)
    assert np.array_equal(lc[:s_cols], at + np.arange(s_cols))
    assert all(i[k] == ib[k] for k in SHAPE), (i, ib)


def test_the_four_reductions_are_the_existing_analyses_bit_for_bit():
    qp0 = _small()
    both = problems.with_arrow(qp0, 3, 5, seed=4)
    only_rows = problems.with_border_rows(qp0, 3, seed=4)
    only_cols = problems.with_long_columns(qp0, 5, seed=4)
    two_chains = problems.pde_control_like(n=30000, m=7700, per_row=12, window=600, seed=11)   # two chains, reordered
    for qp in (both, only_rows, only_cols, qp0):
        # a zero maximum is the corresponding existing entry, whatever the pattern holds
        assert _same(_analyze(qp, 0, 16), _analyze(qp, 0, 16, "cols"))
        assert _same(_analyze(qp, 16, 0), _analyze(qp, 16, 0, "bordered"))
        assert _same(_analyze(qp, 0, 0), _analyze(qp, 0, 0, "plain"))
    # only long rows: L is empty, the result is the bordered entry's
    got = _analyze(only_rows, 16, 16)
    assert got[3]["border_rows"] == 3 and got[3]["border_cols"] == 0 and _same(got, _analyze(only_rows, 16, 0, "bordered"))
    # only long columns: R is empty, the result is the long-column entry's
    got = _analyze(only_cols, 16, 16)
    assert got[3]["border_rows"] == 0 and got[3]["border_cols"] == 5 and _same(got, _analyze(only_cols, 0, 16, "cols"))
    # neither: the plain handle
    for qp in (qp0, two_chains):
        got = _analyze(qp, 16, 16)
        assert got[3]["border_rows"] == 0 and got[3]["border_cols"] == 0 and _same(got, _analyze(qp, 0, 0, "plain"))


def test_more_long_rows_or_columns_than_allowed_take_nothing():
    qp0 = _small()

    def nothing(qp, max_border, max_cols):
        got = _analyze(qp, max_border, max_cols)
        assert got[0] == 0 and got[3]["border_rows"] == 0 and got[3]["border_cols"] == 0
        assert _same(got, _analyze(qp, 0, 0, "plain"))
        assert got[3]["bandwidth_blocks"] >= (got[3]["nblocks"] - 1) // 2
        return got

    nothing(problems.with_arrow(qp0, 17, 5, seed=4), 16, 16)              # 17 long rows with 16 allowed: NOTHING, not a part
    nothing(problems.with_arrow(qp0, 3, 17, seed=4), 16, 16)              # 17 long columns with 16 allowed
    nothing(problems.with_arrow(qp0, 3, 5, seed=4), 2, 16)                # fewer row candidates than long rows
    nothing(problems.with_arrow(qp0, 3, 5, seed=4), 16, 4)                # fewer column candidates than long columns


def test_a_row_left_without_an_ordinary_entry_takes_no_columns():
    """rule (a), checked over ALL rows: a row whose only entries lie in long columns would leave B structurally singular"""
    qp0 = BASES["pde"]()
    qp = problems.with_arrow(qp0, 2, 1, seed=4)
    A = qp.scipy_csr().tolil()
    A[700, :qp0.n] = 0.0
    A = sp.csr_matrix(A)
    A.eliminate_zeros()
    A.sort_indices()
    assert A[700].nnz == 1 and A[700].indices[0] == qp0.n
    lonely = dataclasses.replace(qp, rowptr=A.indptr.astype(np.int32), colind=A.indices.astype(np.int32), vals=A.data.copy())
    got = _analyze(lonely, 16, 16)
    assert got[0] == 0 and got[3]["border_cols"] == 0 and np.all(got[2] == -1)
    assert _same(got, _analyze(lonely, 16, 0, "bordered"))                # L empty: the row border's rule alone


def test_bad_maxima_are_argument_errors_and_the_old_entries_still_refuse_both():
    qp = BASES["aug2dc"]()
    lib = _lib.load()
    h = C.c_void_p()
    rp = np.ascontiguousarray(qp.rowptr, dtype=np.int32)
    ci = np.ascontiguousarray(qp.colind, dtype=np.int32)
    rows = np.zeros(1, dtype=np.int64)
    for max_border, max_cols, word in ((-1, 0, b"max_border"), (17, 0, b"max_border"), (0, -1, b"max_cols"), (0, 17, b"max_cols"),
                                       (16, 17, b"max_cols"), (17, 16, b"max_border")):
        rc, _, _, _ = _analyze(qp, max_border, max_cols)
        assert rc == -1 and word in lib.fpsq_band_last_error(None)
        # (refused before a device is looked for)
        assert lib.fpsq_band_create_arrow(C.byref(h), qp.n, qp.m, rp.ctypes.data, ci.ctypes.data, max_border, max_cols, 0) == -1
        assert word in lib.fpsq_band_last_error(None)
        assert lib.fpsq_band_create_coo_arrow(C.byref(h), qp.n, qp.m, 1, rows.ctypes.data, rows.ctypes.data, 0, max_border,
                                              max_cols, 0) == -1
        assert word in lib.fpsq_band_last_error(None)
    assert _analyze(qp, 16, 16)[0] == 0                                   # both maxima, independently
    for max_border, max_cols in ((1, 1), (16, 16)):
        assert _analyze(qp, max_border, max_cols, "cols")[0] == -1 and b"one kind" in lib.fpsq_band_last_error(None)
        assert lib.fpsq_band_create_bordered_cols(C.byref(h), qp.n, qp.m, rp.ctypes.data, ci.ctypes.data, max_border, max_cols,
                                                  0) == -1
        assert b"one kind" in lib.fpsq_band_last_error(None)


def test_with_arrow_is_the_two_generators_composed_and_keeps_xhat_feasible():
    qp0 = problems.pde_control_like(n=4000, m=400, per_row=16, window=512, seed=21)
    for s_rows, s_cols, kind in ((1, 1, "param"), (3, 5, "stride"), (16, 16, "param")):
        qp = problems.with_arrow(qp0, s_rows, s_cols, col_kind=kind, seed=5)
        assert (qp.n, qp.m) == (qp0.n + s_cols, qp0.m + s_rows)
        A = qp.scipy_csr()
        assert np.allclose(A @ qp.xhat, qp.b, rtol=0, atol=1e-12)
        assert (abs(A[:qp0.m, :qp0.n] - qp0.scipy_csr())).nnz == 0        # the base block is untouched
        want = problems.with_long_columns(problems.with_border_rows(qp0, s_rows, kind="mean", seed=5), s_cols, kind=kind,
                                          seed=5)
        again = problems.with_arrow(qp0, s_rows, s_cols, col_kind=kind, seed=5)
        for other in (want, again):
            assert np.array_equal(other.vals, qp.vals) and np.array_equal(other.colind, qp.colind)
            assert np.array_equal(other.rowptr, qp.rowptr) and np.array_equal(other.b, qp.b)
        Ac = A.tocsc()
        for j in range(s_cols):                                           # the columns reach the border rows too: U_s != 0
            touched = np.sort(Ac[:, qp0.n + j].indices)
            assert np.array_equal(touched, np.arange(qp.m) if kind == "param" else np.arange(j % 4, qp.m, 4))
        assert A[qp0.m:, qp0.n:].nnz > 0
    assert problems.with_arrow(qp0, 2, 2, seed=5).vals.tobytes() != problems.with_arrow(qp0, 2, 2, seed=6).vals.tobytes()


def test_python_surface_has_the_new_names_with_the_stated_defaults():
    from fps_amd.device_qp import DeviceArrowBandEqQP, DeviceBandEqQP

    assert issubclass(DeviceArrowBandEqQP, DeviceBandEqQP)
    assert DeviceBandEqQP._create_entry == "fpsq_band_create_bordered_cols"
    assert DeviceArrowBandEqQP._create_entry == "fpsq_band_create_arrow"
    params = inspect.signature(DeviceArrowBandEqQP.__init__).parameters
    assert list(params)[1:4] == ["qp", "border", "cols"] and params["border"].default == 16 and params["cols"].default == 16
    assert qdsolver.qdsolver_correspondence["hip_ldlt_arrow"] is qdsolver.HIPArrowBandedDirectQDSolver
    assert issubclass(qdsolver.HIPArrowBandedDirectQDSolver, qdsolver.HIPBandedDirectQDSolver)
    params = inspect.signature(qdsolver.HIPArrowBandedDirectQDSolver.__init__).parameters
    assert params["border"].default == 16 and params["cols"].default == 16
    params = inspect.signature(qdsolver.band_analysis_arrow).parameters
    assert list(params) == ["nlp", "explicit_linear_constraints", "border", "cols"]
    assert params["border"].default == 16 and params["cols"].default == 16 and params["explicit_linear_constraints"].default is False
    params = inspect.signature(problems.with_arrow).parameters
    assert list(params) == ["qp", "s_rows", "s_cols", "row_kind", "col_kind", "seed"]
    assert (params["row_kind"].default, params["col_kind"].default, params["seed"].default) == ("mean", "param", 0)
    lib = _lib.load()
    for name in ("fpsq_band_create_arrow", "fpsq_band_create_coo_arrow", "fpsq_band_analyze_arrow"):
        assert hasattr(lib, name)
    qp0 = BASES["aug2dc"]()
    model = nlpmodels.EqQPModel(problems.with_arrow(qp0, 2, 3, seed=1))
    base = qdsolver.band_analysis(nlpmodels.EqQPModel(qp0))
    taken = qdsolver.band_analysis_arrow(model)
    assert (taken["border_rows"], taken["border_cols"]) == (2, 3) and taken["bandwidth_blocks"] == base["bandwidth_blocks"]
    assert qdsolver.band_analysis(model, border=16, cols=16) is None      # the older entry: one kind per handle
    assert qdsolver.band_analysis_arrow(model, border=17) is None


def test_the_numpy_restatement_of_the_scheme_meets_the_dense_kkt_solve():
    """pins the algebra before any kernel runs: the nesting M^-1 r = y - Z_c w_c around M_r^-1, and the one-pass form with G,
    against a dense LU of K = [I A'; A -delta I] on the 643-row shape of the device tests (3 mean rows, 5 all-row columns that
    reach them, delta = 0)"""
    qp0 = problems.pde_control_like(n=3000, m=640, per_row=12, window=256, seed=5)
    qp = problems.with_arrow(qp0, 3, 5, seed=9)
    A = qp.scipy_csr()
    Ad = A.toarray()
    lu = sla.lu_factor(np.block([[np.eye(qp.n), Ad.T], [Ad, np.zeros((qp.m, qp.m))]]), check_finite=False)
    model = ArrowModel(A, 0.0, qp0.m + np.arange(3), qp0.n + np.arange(5))
    assert model.pivot_ratio >= 1.0 and np.any(model.U[model.mb:] != 0.0)
    rng = np.random.default_rng(7)
    r1, r2, c = rng.standard_normal(qp.n), rng.standard_normal(qp.n), rng.standard_normal(qp.m)
    rel = lambda a, b: float(np.max(np.abs(a - b)) / np.max(np.abs(b)))  # noqa: E731
    worst = {False: 0.0, True: 0.0}
    for fused in (False, True):
        for mixed, second in ((True, c), (False, r2)):
            got = model.solve(r1, second, mixed, fused=fused)
            s1 = sla.lu_solve(lu, np.concatenate([r1, np.zeros(qp.m)]))
            s2 = sla.lu_solve(lu, np.concatenate([np.zeros(qp.n), second] if mixed else [second, np.zeros(qp.m)]))
            # K [p; q] = [r; 0] gives q = M^-1 A r;  K [p; q] = [0; c] gives q = -M^-1 c, the mixed entry's q2
            want = (s1[:qp.n], s1[qp.n:], s2[:qp.n], s2[qp.n:])
            worst[fused] = max(worst[fused], max(rel(a, b) for a, b in zip(got, want)))
    print(f"\nnumpy model of the arrow scheme against the dense LU: worst relative error nested {worst[False]:.2e}, fused "
          f"{worst[True]:.2e}")
    assert worst[False] < 1e-12 and worst[True] < 1e-12
