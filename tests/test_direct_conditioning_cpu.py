"""The yardsticks of tests/test_gpu_direct_conditioning.py, checked without a device: the longdouble truth (against mpmath on
one small rung, and its own uncertainty on every rung), the LAPACK reference error over six elimination orders, the numpy
model of the direct back-ends' inverse-based scheme, the classification of every rung, the structure the two-chain rungs rely
on, and the pivots of the regularisation cases.  Every test prints its rung's line (pytest -s):
    rung, cond(M), truth uncertainty, LAPACK min .. max, model (the larger of its two variants), model / LAPACK max."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conditioning_cases as cc  # noqa: E402
import direct_scheme_model as dsm  # noqa: E402
import kkt_truth as kt  # noqa: E402


def test_longdouble_truth_agrees_with_mpmath():
    """40 x 90 with two nearly equal rows, cond(M) ~ 1e9: the refined longdouble solve against 60-digit mpmath.  What a
    caller relies on: the truth is off by less than 1e-3 of what an fp64 LAPACK solve of the same system is off by.  The
    reported uncertainty (the last refinement step) UNDERSTATES the error -- by about ten here: the rounding error of the
    longdouble residual largely repeats from step to step, so the steps stall below it.  This test holds the understatement
    to 1e2 and check_uncertainty asks for an uncertainty of at most 1e-4 of the bar: together, a truth within 1 % of it."""
    rng = np.random.default_rng(12)
    A = rng.uniform(-1, 1, (40, 90)) / np.sqrt(90)
    A[29] = A[7] + 1e-4 * rng.uniform(-1, 1, 90) / np.sqrt(90)
    g, c = rng.standard_normal(90), rng.standard_normal(40)
    t = kt.truth_two_mixed(A, 0.0, g, c)
    exact = kt.mpmath_two_mixed(A, 0.0, g, c)
    err = max(kt.relerr(a, b) for a, b in zip(t[:4], exact))
    lap = cc.errors(cc.lapack_solve(A, cc.gram64(A, 0.0), g, c, True, np.arange(40)), exact + [0.0])
    print(f"\ntruth vs mpmath {err:.2e}, reported uncertainty {t[4]:.2e}, LAPACK vs mpmath {lap.max():.2e}, "
          f"cond {np.linalg.cond(cc.gram64(A, 0.0)):.1e}")
    assert np.linalg.cond(cc.gram64(A, 0.0)) > 1e8
    assert err <= 1e2 * t[4]
    assert err <= 1e-3 * lap.max()
    # the sparse operator is the dense one
    ts = kt.truth_two_least_squares(sp.csr_matrix(A), 1e-6, g, g[::-1].copy())
    td = kt.truth_two_least_squares(A, 1e-6, g, g[::-1].copy())
    assert max(kt.relerr(a, b) for a, b in zip(ts[:4], td[:4])) <= 1e2 * max(ts[4], td[4])


def test_model_factor_is_a_cholesky_factor_on_a_plain_matrix():
    """both variants of the model on a well-conditioned matrix: L L' = M and the solves to rounding, in a permuted stored
    order too -- the model itself has to be right before it explains anything"""
    rng = np.random.default_rng(2)
    A = rng.uniform(-1, 1, (200, 380)) / np.sqrt(380)
    g, c = rng.standard_normal(380), rng.standard_normal(200)
    t = kt.truth_two_mixed(A, 1e-2, g, c)
    for order in (None, rng.permutation(200)):
        for v in dsm.VARIANTS:
            mod = dsm.SchemeModel(A, 1e-2, order, variant=v)
            L = mod.L[:200, :200]
            o = mod.order
            M = cc.gram64(A, 1e-2)[np.ix_(o, o)]
            assert np.max(np.abs(L @ L.T - M)) <= 64 * cc.EPS * np.max(np.abs(M))
            for k in range(mod.nb):
                Lkk = mod.L[128 * k:128 * k + 128, 128 * k:128 * k + 128]
                assert np.max(np.abs(mod.X[k] @ Lkk - np.eye(128))) <= 1e-12
            assert mod.count == 0 and mod.first == 0
            assert cc.errors(mod.solve(g, c, True), t).max() <= 1e-12


@pytest.mark.parametrize("name", cc.RUNGS)
def test_rung_yardsticks_and_classification(name):
    r, ref = cc.rung(name), cc.reference(name)
    lmin, lmax, mod = ref.q_err(ref.lapack_min), ref.q_err(ref.lapack_max), ref.q_err(ref.model)
    print(f"\n{name:24s} cond {ref.cond:8.1e} unc {ref.uncertainty:8.1e} LAPACK {lmin:8.1e} .. {lmax:8.1e} "
          f"model {mod:8.1e} model/LAPACK {mod / lmax:7.1f}  {'neutral' if cc.is_neutral(ref) else 'SENSITIVE'}")
    assert (r.m, r.n) == {"dense": cc.DENSE_SHAPE, "band1": (600, 6000), "band2": (2600, 10400)}[r.kind]
    for e in cc.ENTRIES:
        kt.check_uncertainty(ref.truth[e][4], cc.bar(name, ref, e), name)
        assert np.all(ref.lapack_min[e] <= ref.lapack_max[e]) and np.all(np.isfinite(ref.model[e]))
    # the classification the GPU tests' bars rest on (conditioning_cases.SENSITIVE): a drifting generator is noticed here
    assert cc.is_neutral(ref) == (name in cc.NEUTRAL), (name, mod, lmax)


def test_rung_list_is_what_the_gpu_tests_expect():
    assert len(cc.RUNGS) == 19 and set(cc.SENSITIVE) <= set(cc.RUNGS)
    assert sum(cc.kind_of(r) == "dense" for r in cc.RUNGS) == 9
    assert sum(cc.kind_of(r) == "band1" for r in cc.RUNGS) == 8
    assert any(cc.kind_of(r) != "dense" for r in cc.SENSITIVE)   # the banded handle meets the sensitive bar too
    assert sum(cc.kind_of(r) == "band2" for r in cc.RUNGS) == 2


@pytest.mark.parametrize("name", [r for r in cc.RUNGS if cc.kind_of(r) != "dense"])
def test_band_rungs_have_the_structure_they_are_meant_to_exercise(name):
    r = cc.rung(name)
    perm, info = cc.analyze(r.A)
    pos = np.empty(r.m, dtype=np.int64)
    pos[perm] = np.arange(r.m)
    if r.kind == "band1":
        assert info["chains"] == 1 and info["nblocks"] == 5 and info["bandwidth_blocks"] <= 2
        assert np.array_equal(perm, np.arange(r.m))
        return
    assert info["chains"] == 2 and info["nblocks"] == 21 and info["reordered"] == 1
    blk = pos // 128
    (t0, t1), (b0, b1), (e0, e1), (m0, m1) = cc.BAND2_PAIRS
    assert blk[t0] == blk[t1] == 0                                  # top chain, first block
    assert blk[b0] == blk[b1] and blk[b0] % 2 == 1 and blk[b0] < 16   # bottom chain (odd stored blocks), inside the chain region
    assert blk[e0] == 18 and blk[e1] == 20                          # last top-chain block | the rows left in the middle
    assert blk[m0] == blk[m1] == 20


@pytest.mark.parametrize("name", cc.PIVOT_CASES)
def test_pivot_cases_fire_exactly_where_they_should(name):
    """tol = reg = sqrt(eps), delta = 0: in the model every pivot that should fire is below tol / 100 and every other one
    above 100 tol, so the device's count cannot hinge on rounding; the regularised solve stays within the bar the GPU test
    applies (the bar's second term is checked here against the model, not fitted to a device); FPSQ_REG_DROP's pivot of
    1e200 leaves the fired multipliers below 1e-50 and the rest at the truth of the system without those rows."""
    pc = cc.pivot_case(name)
    order = cc.stored_order(pc.kind, pc.A)
    ref = cc.pivot_reference(name, False)
    dref = cc.pivot_reference(name, True)
    mdiag = float(np.max(np.diag(ref.M64)))
    worst = {}
    for v in dsm.VARIANTS:
        mod = dsm.SchemeModel(pc.A, 0.0, order, cc.SE, cc.SE, v)
        piv = mod.pivots[:pc.m]
        pos = np.empty(pc.m, dtype=np.int64)
        pos[order] = np.arange(pc.m)
        fired_pos = pos[pc.fired]
        others = np.setdiff1d(np.arange(pc.m), fired_pos)
        assert sorted(mod.fired_rows) == pc.fired and mod.count == len(pc.fired)
        assert np.all(piv[fired_pos] < cc.SE / 100) and np.all(piv[others] > 100 * cc.SE)
        drop = dsm.SchemeModel(pc.A, 0.0, order, cc.SE, 1e200, v)
        assert sorted(drop.fired_rows) == pc.fired
        for e in cc.ENTRIES:
            r1, r2 = pc.rhs(e)
            err = cc.errors(mod.solve(r1, r2, e == "mixed"), ref.truth[e])
            bar = cc.regularised_bar(ref.lapack_max[e], mdiag)
            kt.check_uncertainty(ref.truth[e][4], bar, name)
            worst[(v, e)] = float(np.max(err / bar))
            assert np.all(err <= bar), (v, e, err, bar)
            p1, q1, p2, q2 = drop.solve(r1, r2, e == "mixed")
            for q in (q1, q2):
                assert np.max(np.abs(q[pc.fired])) <= 1e-50 * np.max(np.abs(q))
            derr = cc.errors((p1, q1[dref.keep], p2, q2[dref.keep]), dref.truth[e])
            dbar = cc.neutral_bar(dref.lapack_max[e])
            kt.check_uncertainty(dref.truth[e][4], dbar, name)
            assert np.all(derr <= dbar), (v, e, derr, dbar)
    print(f"\n{name:24s} fired {pc.fired} model error / bar at most {max(worst.values()):.2f}")


@pytest.mark.parametrize("kind", ["dense", "band1"])
def test_model_reports_the_first_zero_row(kind):
    """without a regularisation a vanishing pivot is whatever rounding leaves; an exactly ZERO row is reported for certain"""
    pc = cc.pivot_case(f"{kind}-at16")
    base = cc._dense_base() if kind == "dense" else cc.band_near_duplicates(cc.BAND1, 0.0, ())
    order = cc.stored_order(kind, base)
    for rows in ((0,), (15,), (16,), (127,), (128,), (pc.m - 1,), (200, 40)):
        A = sp.lil_matrix(base) if sp.issparse(base) else base.copy()
        for r in rows:
            A[r, :] = 0.0
        assert dsm.SchemeModel(sp.csr_matrix(A) if sp.issparse(A) else A, 0.0, order).first == min(rows) + 1
