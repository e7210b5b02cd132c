"""The dense and the banded direct back-end on ill-conditioned and badly scaled Jacobians (tests/conditioning_cases.py),
against a truth that is better than fp64 (tests/kkt_truth.py), with the bars of tests/conditioning_cases.py:

  scheme-neutral rungs     err <= 8 max(LAPACK max, 1e-13), LAPACK max = the worst of an fp64 LAPACK Cholesky solve of the same
                           M over six elimination orders;
  scheme-sensitive rungs   err <= 8 max(LAPACK max, model), model = tests/direct_scheme_model.py, the inverse-based scheme in
                           numpy: what the ALGORITHM loses.  device / LAPACK max is printed, not asserted.
err = max|got - truth| / max|truth| for each of p1, q1, p2, q2, each held to the bar of ITS OWN LAPACK / model figure.  The
same rule holds the dense factor (max|L L' - M| / max|M|, M in longdouble).  Every test prints one line per rung and entry
(run with -s): cond(M), LAPACK min .. max, model, device, device / LAPACK max -- the multipliers' figures, the larger of q1
and q2; profiles/direct_conditioning.md keeps a run's lines.

The pivot rule of wave_diag16 is checked at the C ABI in its three forms: regularising (tol = reg = sqrt(eps)), dropping
(FPSQ_REG_DROP) and reporting (no regularisation: rc = 1, *info = the first such row)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import fps_amd  # noqa: F401
from fps_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conditioning_cases as cc  # noqa: E402
import direct_scheme_model as dsm  # noqa: E402
import kkt_truth as kt  # noqa: E402

pytestmark = pytest.mark.gpu

REG_DROP = 1e200   # FPSQ_REG_DROP of include/fpsq.h


class _Handle:
    """the dense or the banded handle behind one face: factorize(delta[, A]), solve(entry, r1, r2), info(), close()"""

    def __init__(self, kind, A):
        self.lib = _lib.load()
        self.kind = "dense" if kind == "dense" else "band"
        self.m, self.n = A.shape
        self.h = C.c_void_p()
        if self.kind == "dense":
            assert self.lib.fpsq_dense_create(C.byref(self.h), self.n, self.m, 0) == 0, self.lib.fpsq_dense_last_error(None)
            self.set_values(A)
        else:
            A = sp.csr_matrix(A)
            A.sort_indices()
            self.rp, self.ci = A.indptr.astype(np.int32), A.indices.astype(np.int32)
            rc = self.lib.fpsq_band_create(C.byref(self.h), self.n, self.m, self.rp.ctypes.data, self.ci.ctypes.data, 0)
            assert rc == 0, self.lib.fpsq_band_last_error(None)
            self.set_values(A)

    def err(self):
        return (self.lib.fpsq_dense_last_error if self.kind == "dense" else self.lib.fpsq_band_last_error)(self.h)

    def set_values(self, A):
        """new values on the same shape / pattern (the banded handle takes them at the next factorize)"""
        if self.kind == "dense":
            A = np.ascontiguousarray(A, dtype=np.float64)
            assert self.lib.fpsq_dense_set_jacobian(self.h, A.ctypes.data) == 0
        else:
            A = sp.csr_matrix(A)
            A.sort_indices()
            assert np.array_equal(A.indptr, self.rp) and np.array_equal(A.indices, self.ci)
            self.vals = np.ascontiguousarray(A.data, dtype=np.float64)

    def set_regularization(self, tol, reg):
        fn = self.lib.fpsq_dense_set_regularization if self.kind == "dense" else self.lib.fpsq_band_set_regularization
        assert fn(self.h, tol, reg) == 0

    def factorize(self, delta):
        info = C.c_int32(-1)
        if self.kind == "dense":
            rc = self.lib.fpsq_dense_factorize(self.h, delta, C.byref(info))
        else:
            rc = self.lib.fpsq_band_factorize(self.h, self.vals.ctypes.data, delta, C.byref(info))
        assert rc >= 0, self.err()
        return rc, info.value

    def solve(self, entry, r1, r2):
        fn = getattr(self.lib, f"fpsq_{self.kind}_solve_two_" + ("mixed" if entry == "mixed" else "least_squares"))
        outs = [np.empty(self.n), np.empty(self.m), np.empty(self.n), np.empty(self.m)]
        r1, r2 = np.ascontiguousarray(r1, dtype=np.float64), np.ascontiguousarray(r2, dtype=np.float64)
        assert fn(self.h, r1.ctypes.data, r2.ctypes.data, *[o.ctypes.data for o in outs]) == 0, self.err()
        return outs

    def solve_ls_block(self, R1, R2):
        k = R1.shape[0]
        outs = [np.empty((k, self.n)), np.empty((k, self.m)), np.empty((k, self.n)), np.empty((k, self.m))]
        R1, R2 = np.ascontiguousarray(R1, dtype=np.float64), np.ascontiguousarray(R2, dtype=np.float64)
        rc = self.lib.fpsq_band_solve_two_least_squares_block(self.h, k, R1.ctypes.data, R2.ctypes.data,
                                                              *[o.ctypes.data for o in outs])
        assert rc == 0, self.err()
        return outs

    def factor(self):
        L = np.empty((self.m, self.m))
        assert self.lib.fpsq_dense_get_factor(self.h, L.ctypes.data) == 0
        return L

    def info(self):
        i = _lib.DenseInfo() if self.kind == "dense" else _lib.BandInfo()
        (self.lib.fpsq_dense_get_info if self.kind == "dense" else self.lib.fpsq_band_get_info)(self.h, C.byref(i))
        return i.as_dict()

    def close(self):
        (self.lib.fpsq_dense_destroy if self.kind == "dense" else self.lib.fpsq_band_destroy)(self.h)


def _q(v):
    return float(max(v[1], v[3]))


def _line(tag, ref, entry, err, cond=None):
    lmin, lmax, mod = _q(ref.lapack_min[entry]), _q(ref.lapack_max[entry]), ref.model.get(entry)
    mods = f"{_q(mod):8.1e}" if mod is not None else "       -"
    conds = f"{cond:8.1e}" if cond is not None else "       -"
    print(f"{tag:44s} cond {conds} LAPACK {lmin:8.1e} .. {lmax:8.1e} model {mods} device {_q(err):8.1e} "
          f"device/LAPACK {_q(err) / lmax:6.2f}   per output [{' '.join(f'{x:.1e}' for x in err)}]")


@pytest.mark.parametrize("sweep", ["chain", "step"])
@pytest.mark.parametrize("name", cc.RUNGS)
def test_rung_against_the_truth(name, sweep, monkeypatch):
    """solve_two_mixed and solve_two_least_squares with the chained sweeps (the default) and the step sweeps
    (FPSQ_TRSV_CHAIN=0, read when the handle is created); on the band also the block entry with k = 3 (the matrix-core
    sweep); on the dense handle also the factor."""
    r, ref = cc.rung(name), cc.reference(name)
    monkeypatch.setenv("FPSQ_TRSV_CHAIN", "1" if sweep == "chain" else "0")
    H = _Handle(r.kind, r.A)
    if r.kind != "dense":
        assert H.info()["chains"] == (2 if r.kind == "band2" else 1)
    assert H.factorize(r.delta) == (0, 0)
    print()
    failures = []
    for entry in cc.ENTRIES:
        bar = cc.bar(name, ref, entry)
        kt.check_uncertainty(ref.truth[entry][4], bar, name)
        err = cc.errors(H.solve(entry, *r.rhs(entry)), ref.truth[entry])
        _line(f"{name} {entry} {sweep}", ref, entry, err, ref.cond)
        if not np.all(err <= bar):
            failures.append((entry, sweep, err, bar))
    if r.kind != "dense" and sweep == "chain":
        # columns (g, g2), (g2, g), (g, g2): the truth of the least-squares entry, as it is and with its systems swapped
        t = ref.truth["ls"]
        bar = cc.bar(name, ref, "ls")
        got = H.solve_ls_block(np.stack([r.g, r.g2, r.g]), np.stack([r.g2, r.g, r.g2]))
        for j, (tj, bj) in enumerate(((t, bar), ((t[2], t[3], t[0], t[1]), bar[[2, 3, 0, 1]]), (t, bar))):
            err = cc.errors([o[j] for o in got], tj)
            if j == 0:
                _line(f"{name} ls block(k=3) column 0", ref, "ls", err, ref.cond)
            if not np.all(err <= bj):
                failures.append(("block", j, err, bj))
    if r.kind == "dense" and sweep == "chain":
        M, lmin, lmax, mod = cc.factor_reference(name)
        res = cc.factor_residual(H.factor(), M)
        fbar = 8.0 * max(lmax, mod) if name in cc.SENSITIVE else 8.0 * max(lmax, 1e-13)
        print(f"{name + ' factor |LL^T - M|/|M|':44s} cond {ref.cond:8.1e} LAPACK {lmin:8.1e} .. {lmax:8.1e} model {mod:8.1e} "
              f"device {res:8.1e} device/LAPACK {res / lmax:6.2f}")
        if not res <= fbar:
            failures.append(("factor", res, fbar))
    H.close()
    assert not failures, failures


@pytest.mark.parametrize("name", ["dense-dup-delta-1e-4", "band1-dup-delta-sqrteps", "band2-eps1e-3"])
def test_power_of_two_scaling_changes_nothing_but_exponents(name):
    """A 2^k, delta 4^k, k = +-40, regularisation off:  p1' = p1, q1' = q1 2^-k, p2' = p2 2^-k, q2' = q2 4^-k.  Scaling by a
    power of two commutes with every rounding of the scheme, so the results are expected to be EQUAL (printed); the assertion
    is 8 eps in max norm.  An absolute threshold hidden in a kernel would break this."""
    r = cc.rung(name)
    delta = r.delta if r.delta > 0 else 1e-6    # (the two-chain rung has delta = 0: give the scaling of delta something to do)
    H = _Handle(r.kind, r.A)
    assert H.factorize(delta) == (0, 0)
    base = H.solve("mixed", r.g, r.c)
    print()
    for k in (40, -40):
        s = 2.0 ** k
        H.set_values(r.A * s)
        assert H.factorize(delta * s * s) == (0, 0)
        p1, q1, p2, q2 = H.solve("mixed", r.g, r.c)
        back = (p1, q1 * s, p2 * s, q2 * s * s)
        errs = [kt.relerr(a, b) for a, b in zip(back, base)]
        exact = all(np.array_equal(a, b) for a, b in zip(back, base))
        print(f"{name} k = {k:+d}: exactly equal: {exact}; max-norm differences {errs}")
        assert max(errs) <= 8 * cc.EPS
    H.close()


@pytest.mark.parametrize("name", cc.PIVOT_CASES)
def test_regularised_pivots(name):
    """tol = reg = sqrt(eps), delta = 0, exactly duplicated rows, consistent right-hand sides: the count is the model's and the
    solves are those of (M + reg E) q = r, E selecting the fired rows, within 8 max(LAPACK max on M + reg E,
    64 eps max(M_ii) / reg)."""
    pc, ref = cc.pivot_case(name), cc.pivot_reference(name, False)
    count = dsm.SchemeModel(pc.A, 0.0, cc.stored_order(pc.kind, pc.A), cc.SE, cc.SE, "doubling").count
    assert count == len(pc.fired)
    H = _Handle(pc.kind, pc.A)
    H.set_regularization(cc.SE, cc.SE)
    assert H.factorize(0.0) == (0, 0)
    assert H.info()["regularized_pivots"] == count
    mdiag = float(np.max(np.diag(ref.M64)))
    print()
    for entry in cc.ENTRIES:
        bar = cc.regularised_bar(ref.lapack_max[entry], mdiag)
        kt.check_uncertainty(ref.truth[entry][4], bar, name)
        err = cc.errors(H.solve(entry, *pc.rhs(entry)), ref.truth[entry])
        _line(f"{name} reg {entry}", ref, entry, err)
        assert np.all(err <= bar), (entry, err, bar)
    H.close()


@pytest.mark.parametrize("name", cc.PIVOT_CASES)
def test_dropped_pivots(name):
    """reg = FPSQ_REG_DROP (a pivot of 1e200): the fired rows' multipliers vanish, |q[fired]| <= 1e-50 max|q|, and everything
    else is the solution of the system WITHOUT those rows, at the bar of a scheme-neutral rung (LAPACK on the reduced system)."""
    pc, ref = cc.pivot_case(name), cc.pivot_reference(name, True)
    H = _Handle(pc.kind, pc.A)
    H.set_regularization(cc.SE, REG_DROP)
    assert H.factorize(0.0) == (0, 0)
    assert H.info()["regularized_pivots"] == len(pc.fired)
    print()
    for entry in cc.ENTRIES:
        bar = cc.neutral_bar(ref.lapack_max[entry])
        kt.check_uncertainty(ref.truth[entry][4], bar, name)
        p1, q1, p2, q2 = H.solve(entry, *pc.rhs(entry))
        for q in (q1, q2):
            assert np.max(np.abs(q[pc.fired])) <= 1e-50 * np.max(np.abs(q))
        err = cc.errors((p1, q1[ref.keep], p2, q2[ref.keep]), ref.truth[entry])
        _line(f"{name} drop {entry}", ref, entry, err)
        assert np.all(err <= bar), (entry, err, bar)
    H.close()


def _with_zero_rows(A, rows):
    """same shape and (for a sparse A) same pattern, the rows' values zero"""
    if sp.issparse(A):
        A = sp.csr_matrix(A).copy()
        for r in rows:
            A.data[A.indptr[r]:A.indptr[r + 1]] = 0.0
        return A
    A = A.copy()
    A[list(rows)] = 0.0
    return A


@pytest.mark.parametrize("kind", ["dense", "band1"])
def test_a_zero_row_is_reported_by_its_index(kind):
    """regularisation off, delta = 0: an exactly zero row r gives rc = 1 and *info = r + 1 -- first and last row of a 16-row
    tile, of a 128-row block, the last row before the padding; of two zero rows the lower."""
    base = cc._dense_base() if kind == "dense" else cc.band_near_duplicates(cc.BAND1, 0.0, ())
    m = base.shape[0]
    H = _Handle(kind, base)
    assert H.factorize(0.0) == (0, 0)
    for rows in ((0,), (15,), (16,), (127,), (128,), (m - 1,), (200, 40), (129, 298)):
        H.set_values(_with_zero_rows(base, rows))
        assert H.factorize(0.0) == (1, min(rows) + 1), rows
    H.set_values(base)   # ... and the handle recovers
    assert H.factorize(0.0) == (0, 0)
    H.close()


def test_two_chains_report_the_row_first_in_the_stored_order():
    """one zero row in each elimination chain: *info is the one at the lower STORED position (include/fpsq.h,
    fpsq_band_factorize), whichever chain's kernel runs first -- the same over three factorisations.  Two placements: the
    chains' first blocks (their kernels start side by side: the top chain's row wins), and a top-chain row one block further
    in than the bottom chain's (the bottom chain's row wins)."""
    base = cc.band_near_duplicates(cc.BAND2, 0.0, ())
    m = base.shape[0]
    perm, info = cc.analyze(base)
    assert info["chains"] == 2
    pos = np.empty(m, dtype=np.int64)
    pos[perm] = np.arange(m)
    H = _Handle("band2", base)
    assert H.info()["chains"] == 2
    for top, bottom, winner in ((10, m - 11, 10), (200, m - 6, m - 6)):
        assert pos[top] // 128 % 2 == 0 and pos[bottom] // 128 % 2 == 1 and pos[top] // 128 < 16 and pos[bottom] // 128 < 16
        assert winner == (top if pos[top] < pos[bottom] else bottom)
        H.set_values(_with_zero_rows(base, (top, bottom)))
        got = [H.factorize(0.0) for _ in range(3)]
        assert got == [(1, winner + 1)] * 3, (top, bottom, got)
    H.close()


@pytest.mark.parametrize("name", ["band1-eps1e-2", "band1-wide-eps1e-5"])
def test_band_objgrad_multipliers_on_ill_conditioned_jacobians(name):
    """fpsq_band_qp_objgrad's ys = q1 + sigma q2 and gs = p1 + sigma p2 (include/fpsq.h) on a scheme-neutral rung (cond(M) 4e5)
    and on the scheme-sensitive banded rung (cond 4e11), each under the bar of its class; LAPACK and the model evaluate the
    same formulas from g and c formed in fp64."""
    r, ref = cc.rung(name), cc.objgrad_reference(name)
    lib = _lib.load()
    H = _Handle(r.kind, r.A)
    assert H.factorize(r.delta) == (0, 0)
    qp = C.c_void_p()
    arrs = [np.ascontiguousarray(a) for a in (ref.qdiag, ref.d, ref.b, ref.x)]
    assert lib.fpsq_band_qp_create(H.h, arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data, C.byref(qp)) == 0
    fx, ys, gs = C.c_double(), np.empty(r.m), np.empty(r.n)
    rc = lib.fpsq_band_qp_objgrad(H.h, qp, arrs[3].ctypes.data, cc.SIGMA, 0.0, 0.0, None, C.byref(fx), None, ys.ctypes.data,
                                  gs.ctypes.data)
    assert rc == 0, H.err()
    sensitive = name in cc.SENSITIVE
    bar = cc.sensitive_bar(ref.lapack_max, ref.model) if sensitive else cc.neutral_bar(ref.lapack_max)
    kt.check_uncertainty(ref.unc, np.array([bar[1], bar[0], bar[1], bar[0]]), name)   # (p1, q1, p2, q2) <- (gs, ys, gs, ys)
    err = np.array([kt.relerr(ys, ref.ys), kt.relerr(gs, ref.gs)])
    f = lambda v: "[" + " ".join(f"{x:.2e}" for x in np.asarray(v)) + "]"  # noqa: E731
    print(f"\n{name + ' objgrad (ys, gs)':44s} LAPACK {f(ref.lapack_min)} .. {f(ref.lapack_max)} model {f(ref.model)} "
          f"device {f(err)} device/LAPACK {f(err / ref.lapack_max)}")
    assert np.all(err <= bar), (err, bar)
    lib.fpsq_band_qp_destroy(qp)
    H.close()
