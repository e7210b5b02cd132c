"""The symbolic phase of the bordered band (fpsq_band_analyze_bordered: host only, no device) and the generator of long rows.
A few long constraint rows couple with every other row of M = A A' + delta I; the bordered entries store them last and
describe the band of the others (include/fpsq.h "BORDERED BAND")."""
import ctypes as C
import inspect

import numpy as np
import pytest
import scipy.sparse as sp

import fps_amd  # noqa: F401
from fps_amd import _lib, nlpmodels, problems, qdsolver


def _analyze(qp, max_border, bordered=True):
    lib = _lib.load()
    rp = np.ascontiguousarray(qp.rowptr, dtype=np.int32)
    ci = np.ascontiguousarray(qp.colind, dtype=np.int32)
    perm = np.full(qp.m, -1, dtype=np.int32)
    info = _lib.BandInfo()
    if bordered:
        rc = lib.fpsq_band_analyze_bordered(qp.n, qp.m, rp.ctypes.data, ci.ctypes.data, max_border, perm.ctypes.data,
                                            C.byref(info))
    else:
        rc = lib.fpsq_band_analyze(qp.n, qp.m, rp.ctypes.data, ci.ctypes.data, perm.ctypes.data, C.byref(info))
    return rc, perm, info.as_dict()


# The small shapes of the existing tests at which a border can pay at all.  The rule takes a border when the band of the
# other rows is at most a QUARTER as wide in blocks: with the band 1 - 2 blocks wide that needs a matrix of 5 - 9 blocks or
# more (at pde_control_like(m=400) or aug2dc_like(N=30) reverse Cuthill-McKee keeps the band with a long row within 2 - 3
# blocks, and the rule rightly takes nothing).  "pde": one chain, 16 blocks; "aug2dc": two chains, 21 blocks.
BASES = {
    "pde": lambda: problems.pde_control_like(n=20000, m=2000, per_row=40, window=1024, seed=3),
    "aug2dc": lambda: problems.aug2dc_like(N=51),
}


@pytest.mark.parametrize("s", [1, 5, 16])
@pytest.mark.parametrize("base", list(BASES))
def test_long_rows_are_detected_and_the_band_is_the_one_without_them(base, s):
    qp0 = BASES[base]()
    qp = problems.with_border_rows(qp0, s, kind="mean", seed=7)
    rc0, perm0, i0 = _analyze(qp0, 0)
    rc, perm, i = _analyze(qp, 16)
    assert rc0 == 0 and rc == 0
    assert i["border_rows"] == s
    for k in ("bandwidth_blocks", "nblocks", "chains"):
        assert i[k] == i0[k], (k, i, i0)
    assert (i["n"], i["m"], i["nnz"]) == (qp.n, qp.m, qp.nnz)
    assert np.array_equal(np.sort(perm), np.arange(qp.m))                 # a permutation ...
    assert np.array_equal(perm[-s:], qp0.m + np.arange(s))                # ... with the added rows at the end, ascending
    assert np.array_equal(perm[:qp0.m], perm0)                            # ... behind the ordering of the others
    # without a border a row that couples with all others keeps the band at least half the matrix wide, whatever the order
    rc, _, full = _analyze(qp, 0)
    assert rc == 0 and full["border_rows"] == 0
    assert full["bandwidth_blocks"] >= max((full["nblocks"] - 1) // 2, 4 * i["bandwidth_blocks"])


@pytest.mark.parametrize("base", list(BASES))
def test_wrap_around_rows_that_the_ordering_absorbs_are_not_taken(base):
    """"periodic" rows tie the two ends of the band together; reverse Cuthill-McKee orders such a ring into a band at most
    about twice as wide, so a border would gain less than the factor of four the rule asks for: the border stays empty."""
    qp0 = BASES[base]()
    _, _, i0 = _analyze(qp0, 0)
    for s in (1, 5, 16):
        qp = problems.with_border_rows(qp0, s, kind="periodic", seed=7)
        rc, perm, i = _analyze(qp, 16)
        rc_a, perm_a, i_a = _analyze(qp, 0, bordered=False)
        assert rc == 0 and i["border_rows"] == 0 and i == i_a and np.array_equal(perm, perm_a)
        assert i["bandwidth_blocks"] <= 2 * i0["bandwidth_blocks"] + 1


def test_border_rows_anywhere_in_the_callers_order_and_a_shuffled_band():
    qp0 = BASES["pde"]()
    qp = problems.with_border_rows(qp0, 5, seed=2)
    order = np.random.default_rng(3).permutation(qp.m)                    # stored row p of the test's QP = row order[p]
    A = sp.csr_matrix(qp.scipy_csr()[order])
    A.sort_indices()
    import dataclasses

    shuffled = dataclasses.replace(qp, rowptr=A.indptr.astype(np.int32), colind=A.indices.astype(np.int32), vals=A.data,
                                   b=qp.b[order])
    rc, perm, i = _analyze(shuffled, 8)
    assert rc == 0 and i["border_rows"] == 5 and i["reordered"] == 1
    assert np.array_equal(np.sort(perm), np.arange(qp.m))
    where = np.sort(np.nonzero(order >= qp0.m)[0])                        # the long rows in the shuffled numbering
    assert np.array_equal(perm[-5:], where)
    assert i["bandwidth_blocks"] <= 4 and i["nblocks"] == (qp0.m + 127) // 128   # reverse Cuthill-McKee on the band rows


def test_no_border_to_take_is_the_plain_handle():
    qp0 = BASES["pde"]()
    rc_a, perm_a, info_a = _analyze(qp0, 0, bordered=False)
    assert rc_a == 0
    for max_border in (0, 16):                                            # no long rows; nothing asked for
        rc, perm, info = _analyze(qp0, max_border)
        assert rc == 0 and info["border_rows"] == 0
        assert info == info_a and np.array_equal(perm, perm_a)
    long_ = problems.pde_control_like(n=30000, m=7700, per_row=12, window=600, seed=11)   # two chains, reordered
    rc_a, perm_a, info_a = _analyze(long_, 0, bordered=False)
    rc, perm, info = _analyze(long_, 16)
    assert info_a["chains"] == 2 and info == info_a and np.array_equal(perm, perm_a)
    # 17 long rows with max_border = 16: no set of candidates narrows the band, so the border is EMPTY, not partial
    qp17 = problems.with_border_rows(qp0, 17, seed=4)
    rc_a, perm_a, info_a = _analyze(qp17, 0, bordered=False)
    rc, perm, info = _analyze(qp17, 16)
    assert rc == 0 and rc_a == 0 and info["border_rows"] == 0
    assert info == info_a and np.array_equal(perm, perm_a)
    # ... and fewer candidates than long rows likewise
    rc, perm, info = _analyze(problems.with_border_rows(qp0, 5, seed=4), 4)
    assert rc == 0 and info["border_rows"] == 0 and info["bandwidth_blocks"] >= (info["nblocks"] - 1) // 2


def test_max_border_out_of_range_is_an_argument_error():
    qp = BASES["aug2dc"]()
    lib = _lib.load()
    for bad in (-1, 17):
        rc, _, _ = _analyze(qp, bad)
        assert rc == -1
        assert b"max_border" in lib.fpsq_band_last_error(None)
    h = C.c_void_p()
    rp = np.ascontiguousarray(qp.rowptr, dtype=np.int32)
    ci = np.ascontiguousarray(qp.colind, dtype=np.int32)
    for bad in (-1, 17):                                                  # (refused before a device is looked for)
        assert lib.fpsq_band_create_bordered(C.byref(h), qp.n, qp.m, rp.ctypes.data, ci.ctypes.data, bad, 0) == -1
        rows = np.zeros(1, dtype=np.int64)
        assert lib.fpsq_band_create_coo_bordered(C.byref(h), qp.n, qp.m, 1, rows.ctypes.data, rows.ctypes.data, 0, bad, 0) == -1


@pytest.mark.parametrize("kind", ["mean", "periodic"])
def test_with_border_rows_appends_long_rows_and_keeps_xhat_feasible(kind):
    qp0 = problems.pde_control_like(n=4000, m=400, per_row=16, window=512, seed=21)
    for s in (1, 5, 16):
        qp = problems.with_border_rows(qp0, s, kind=kind, seed=5)
        assert (qp.n, qp.m) == (qp0.n, qp0.m + s) and qp.b.shape == (qp.m,) and qp.rowptr.shape == (qp.m + 1,)
        assert qp.rowptr.dtype == np.int32 and qp.colind.dtype == np.int32 and qp.vals.dtype == np.float64
        assert qp.rowptr[0] == 0 and qp.rowptr[-1] == qp.colind.size == qp.vals.size
        assert np.array_equal(qp.rowptr[:qp0.m + 1], qp0.rowptr) and np.array_equal(qp.vals[:qp0.nnz], qp0.vals)
        assert np.array_equal(qp.b[:qp0.m], qp0.b)
        A = qp.scipy_csr()
        assert np.allclose(A @ qp.xhat, qp.b, rtol=0, atol=1e-12)
        for r in range(qp.m):                                             # sorted, distinct columns in range: no duplicates
            c = qp.colind[qp.rowptr[r]:qp.rowptr[r + 1]]
            assert c.size > 0 and c.min() >= 0 and c.max() < qp.n and np.all(np.diff(c) > 0)
        for r in range(qp0.m, qp.m):                                      # the added rows span (nearly) all columns
            c = qp.colind[qp.rowptr[r]:qp.rowptr[r + 1]]
            assert c.max() - c.min() >= qp.n - 8 * s - 16
            if kind == "mean":
                assert np.array_equal(c, np.arange((r - qp0.m) % 16, qp.n, 16))
            else:
                assert c.size == 8
        again = problems.with_border_rows(qp0, s, kind=kind, seed=5)
        assert np.array_equal(again.vals, qp.vals) and np.array_equal(again.colind, qp.colind)
    with pytest.raises(ValueError):
        problems.with_border_rows(qp0, 1, kind="dense")


def test_python_surface_forwards_the_border():
    from fps_amd.device_qp import DeviceBandEqQP, DeviceBorderedBandEqQP

    assert issubclass(DeviceBorderedBandEqQP, DeviceBandEqQP) and DeviceBandEqQP.border == 0
    assert list(inspect.signature(DeviceBorderedBandEqQP.__init__).parameters)[1:3] == ["qp", "border"]
    assert inspect.signature(qdsolver.HIPBandedDirectQDSolver.__init__).parameters["border"].default == 0
    assert inspect.signature(qdsolver.band_analysis).parameters["border"].default == 0
    assert "border_rows" in [f for f, _ in _lib.BandInfo._fields_] and "last_border_ms" in [f for f, _ in _lib.BandInfo._fields_]
    qp0 = BASES["aug2dc"]()
    model = nlpmodels.EqQPModel(problems.with_border_rows(qp0, 3, seed=1))
    plain, taken = qdsolver.band_analysis(model), qdsolver.band_analysis(model, border=16)
    base = qdsolver.band_analysis(nlpmodels.EqQPModel(qp0))
    assert plain["border_rows"] == 0 and plain["bandwidth_blocks"] >= (plain["nblocks"] - 1) // 2
    assert taken["border_rows"] == 3 and taken["bandwidth_blocks"] == base["bandwidth_blocks"]
