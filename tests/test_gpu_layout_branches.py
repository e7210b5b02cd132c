"""Every stored layout of the Jacobian (csrc/fpsq_layout.h), read by the product kernels on the device: the small cases of
tests/host/layout_check.cpp -- same generators, same seeds, so the program's output says which branch each takes -- go
through the C ABI (create, structure, values, fpsq_jac_mul with trans = 0 and 1) and are compared with the float64 CSR
product.

Tolerance (derived, not measured): any summation order of a row of L products obeys |err| <= gamma_L sum_j |a_ij| |x_j|,
gamma_L = L u / (1 - L u), u = 2^-53; the device's order and the reference's each do, hence 2 gamma_L per row.  An empty
row must come out exactly 0.  fpsq_get_info (at_sorted, spmv_a_blocks) says that a case took the branch it was built for."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import fps_amd  # noqa: F401
from fps_amd import _lib

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
M64 = (1 << 64) - 1


def _splitmix(seed):
    state = [seed]

    def rnd():
        state[0] = (state[0] + 0x9e3779b97f4a7c15) & M64
        z = state[0]
        z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
        z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
        return ((z ^ (z >> 31)) >> 16) & 0xffffffff
    return rnd


def _banded_rows(m, n, per, window, seed=1):
    """row i: `per` distinct columns in a window of `window` columns centred at i n / m (clamped)"""
    rnd = _splitmix(seed)
    rows = []
    for i in range(m):
        start = min(max(i * n // m - window // 2, 0), n - window)
        r = set()
        while len(r) < per:
            r.add(start + rnd() % window)
        rows.append(r)
    return rows


def _csr(m, n, rows):
    indptr = np.zeros(m + 1, dtype=np.int32)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    indices = np.array([c for r in rows for c in sorted(r)], dtype=np.int32)
    data = np.random.default_rng(5).standard_normal(indices.size)
    return sp.csr_matrix((data, indices, indptr), shape=(m, n))


def _banded():
    return _csr(512, 4096, _banded_rows(512, 4096, 12, 256))


def _wide_at():
    m, n = 10000, 12000
    return _csr(m, n, [{i, i * 7919 % n, (i * 104729 + 13) % n} for i in range(m)])


def _long_row():
    rnd, r = _splitmix(1), set()
    while len(r) < 3000:
        r.add(rnd() % 4000)
    return _csr(1, 4000, [r])


def _empty_rows_columns():
    rows = _banded_rows(300, 600, 5, 600)
    for i in list(range(0, 300, 7)) + [299]:
        rows[i] = set()
    return _csr(300, 5000, rows)


def _piled():
    rows = _banded_rows(1024, 8192, 12, 256)
    for i in range(0, 1024, 16):
        rows[i].add((i // 16) % 8)
    return _csr(1024, 8192, rows)


# name: (generator, options, environment, at_sorted, spmv_a_blocks).  at_sorted: 2 shared values, 1 column-sorted, 0 neither.
# spmv_a_blocks: the row groups of A (ceil(m / 128) here: no group reaches its nonzero budget) -- or, without them, A's row blocks.
CASES = {
    "banded": (_banded, {}, {}, 2, 4),
    "banded-align-1": (_banded, {}, {"FPSQ_AT_ROW_ALIGN": "1"}, 2, 4),
    "banded-plain-order": (_banded, {}, {"FPSQ_RGCS_PHASE": "0"}, 2, 4),
    "banded-not-shared": (_banded, {}, {"FPSQ_AT_SHARED": "0"}, 1, 4),
    "banded-row-order": (_banded, {}, {"FPSQ_AT_SORTED": "0"}, 0, 4),
    "banded-jac-format-1": (_banded, {"jac_format": 1}, {}, 0, 4),     # CSR stream: 170 rows of 12 fill a block of 2048
    "window-20000": (lambda: _csr(512, 40000, _banded_rows(512, 40000, 12, 20000)), {}, {}, 2, 4),
    "wide-at": (_wide_at, {}, {}, 0, 79),                               # A' blocks wider than 8192: padded, 16-bit columns
    "uniform-200000": (lambda: _csr(512, 200000, _banded_rows(512, 200000, 12, 200000)), {}, {}, 2, 4),
    "one-long-row": (_long_row, {}, {}, 1, 1),                         # compact row group: nothing to share values with
    "empty-rows-columns": (_empty_rows_columns, {}, {}, 2, 3),
    "m-1": (lambda: _csr(1, 3, [{0, 1, 2}]), {}, {}, 2, 1),
    "piled-first-block": (_piled, {}, {}, 2, 8),                       # shared, the first block keeps its own values
    "scattered": (lambda: _csr(8192, 32768, _banded_rows(8192, 32768, 2, 32768)), {}, {}, 1, 64),  # shared given up
    "span-2^21": (lambda: _csr(2, 2200001, [{0, 2200000}, {5}]), {}, {}, 1, 1),                    # no row groups
}


@pytest.mark.parametrize("name", list(CASES))
def test_products_through_every_layout(name, monkeypatch):
    gen, opts, env, at_sorted, a_blocks = CASES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    A = gen()
    m, n = A.shape
    lib = _lib.load()
    o = _lib.Options()
    lib.fpsq_default_options(n, m, C.byref(o))
    for k, v in opts.items():
        setattr(o, k, v)
    h = C.c_void_p()
    assert lib.fpsq_create(C.byref(h), n, m, C.byref(o)) == 0, lib.fpsq_last_error(None)
    try:
        rp, ci = A.indptr.astype(np.int32), A.indices.astype(np.int32)
        assert lib.fpsq_set_jacobian_structure_csr(h, rp.ctypes.data, ci.ctypes.data) == 0, lib.fpsq_last_error(h)
        vals = np.ascontiguousarray(A.data, dtype=np.float64)
        assert lib.fpsq_set_jacobian_values(h, vals.ctypes.data) == 0, lib.fpsq_last_error(h)
        info = _lib.Info()
        assert lib.fpsq_get_info(h, C.byref(info)) == 0
        print(name, "at_sorted", info.at_sorted, "spmv_a_blocks", info.spmv_a_blocks, "spmv_at_blocks", info.spmv_at_blocks)
        assert (info.at_sorted, info.spmv_a_blocks) == (at_sorted, a_blocks)
        rng = np.random.default_rng(11)
        for trans, M in ((0, A), (1, sp.csr_matrix(A.T))):
            x = rng.standard_normal(M.shape[1])
            y = np.full(M.shape[0], np.nan)
            assert lib.fpsq_jac_mul(h, trans, 1.0, x.ctypes.data, 0.0, y.ctypes.data) == 0, lib.fpsq_last_error(h)
            L = np.diff(M.indptr).astype(np.float64)
            bound = 2.0 * (L * U / (1.0 - L * U)) * (abs(M) @ np.abs(x))
            err = np.abs(y - M @ x)
            print(name, "trans", trans, "largest error / bound", np.max(err[bound > 0] / bound[bound > 0], initial=0.0))
            assert np.all(np.isfinite(y)) and np.all(err <= bound), (trans, int(np.argmax(err - bound)))
    finally:
        lib.fpsq_destroy(h)
