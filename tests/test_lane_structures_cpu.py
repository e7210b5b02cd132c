"""What tests/test_gpu_lane_structures.py relies on, pinned with the C restatement alone (no GPU): on the seven Jacobians of
tests/structures.py, cut at k = 1, 2, 3 iterations, the LNLQ lane (ln_method = 1), the LSQR + MINRES lanes of solve_two_extras and
MINRES on K give the same (niter, status, solved) in the restatement's three summation orders, move by less than the caps of the
allowance under re-association, really stop ON the cut (the GPU test is not comparing zeros), and the comparison the GPU test
asserts with rejects a reference that is wrong by one matrix entry or by one iteration."""
import numpy as np
import pytest
import scipy.sparse as sp

import lane_cases as L
from structures import ALL_KINDS

BITE_KINDS = ["dense-row", "dense-column", "empty-columns"]


@pytest.mark.parametrize("kind", ALL_KINDS)
@pytest.mark.parametrize("lane", L.LANES)
def test_the_three_summation_orders_agree_on_the_cuts_and_stay_inside_the_caps(oracle, lane, kind):
    """7 kinds x 3 lanes here, delta in {0, sqrt(eps), 0.25} x k in {1, 2, 3} inside: 189 combinations, none left out."""
    for delta in L.DELTAS:
        for k in L.CUTS:
            want = L.cut_reference(oracle, lane, kind, delta, k)
            for order in (1, 2):
                alt = L.cut_reference(oracle, lane, kind, delta, k, order)
                for cw, ca in zip(want, alt):
                    assert cw[0] == ca[0] and [s[:3] for s in cw[1]] == [s[:3] for s in ca[1]], (delta, k, order)
                assert L.is_finite(alt), (delta, k, order)
            tol = L.allowance(L.spread(oracle, lane, kind, delta, k), k)   # (asserts the caps: 1e-11 at k = 1, 1e-6 at every cut)
            for order in (1, 2):   # the rule the device is held to is one the restatement's own orders satisfy, estimates included
                L.compare(L.cut_reference(oracle, lane, kind, delta, k, order), want, tol, f"order {order} delta={delta:.3g} k={k}")
            if kind == "tiny":   # one row: the recurrences may finish, legitimately, before the cut
                continue
            for rc, stats, vecs in want:
                assert rc == 3
                for i, st in enumerate(stats):
                    lagged = lane == "lnlq" and i == 1   # pass k of lnlq!'s loop is completed, and counted, by iteration k + 1
                    assert st[:3] == (k + 1 if lagged else k, 7, 0), (delta, k, i, st)
                # (MINRES on K at k = 1 is the multiple b'Kb / |Kb|^2 of the right-hand side b: one block of it is zero, and for
                # b = [0; c] at delta = 0 the multiple is -- that system's iterate is exactly zero in both programs)
                if lane == "minres-k" and k == 1:
                    vecs = vecs[:1]
                assert all(np.all(np.isfinite(v)) and np.any(v != 0.0) for v in vecs), (delta, k)


def test_tiny_finishes_before_the_cut_as_measured(oracle):
    """The one-row Jacobian at the largest cut: what the lanes report when they end on their own (delta = 0.25)."""
    got = {lane: [s[:3] for c in L.cut_reference(oracle, lane, "tiny", 0.25, 3) for s in c[1]] for lane in L.LANES}
    assert got["lnlq"] == [(1, 3, 1), (2, 3, 1)]
    assert got["extras"] == [(1, 3, 1), (1, 4, 1)]
    assert got["minres-k"] == [(3, 4, 1), (2, 4, 1), (3, 4, 1), (3, 4, 1)]


def test_lnlq_restatement_survives_the_exact_breakdown_of_a_one_row_jacobian(oracle):
    """On a Jacobian of one row the bidiagonalisation ends after one pass: beta_2 = |B v_1 - alpha_1 u_1| is zero up to rounding,
    and EXACTLY zero when the row is summed right to left (order 2) -- or left to right on the one-row matrix of
    test_fused_qp_entries_on_awkward_structures.  LNLQ's recurrence taken literally then forms tau_2 = -0 tau_1 / 0 and hands
    NaN back for a solved system (the restatement did, until this test; the GPU run of that test with ln_method = 1 showed it:
    device finite, reference NaN).  With the coefficients of the vectors that do not exist set to zero, every order ends at the
    CRAIG point, which here is the exact minimum-norm solution."""
    ex = L.exact(oracle, "lnlq", "tiny", 0.25)
    for delta in L.DELTAS:
        runs = [L.cut_reference(oracle, "lnlq", "tiny", delta, 1, order) for order in (0, 1, 2)]
        assert runs[2][0][1][1][:4] == (2, 3, 1, 0.0) and runs[0][0][1][1][3] > 0.0   # (exact breakdown in order 2 only)
        for run in runs:
            assert L._rel(run[0][2][2], ex[0][2]) < 1e-15 and L._rel(run[0][2][3], ex[0][3]) < 1e-15   # (unregularised for every delta)


def _without_one_entry(A, longest):
    """A with one entry (the middle one) of its longest row / longest column removed from the structure."""
    A = sp.csr_matrix(A)
    if longest == "row":
        i = int(np.argmax(np.diff(A.indptr)))
        e = (A.indptr[i] + A.indptr[i + 1]) // 2
    else:
        j = int(np.argmax(np.bincount(A.indices, minlength=A.shape[1])))
        hits = np.flatnonzero(A.indices == j)
        e = hits[hits.size // 2]
    keep = np.ones(A.nnz, dtype=bool)
    keep[e] = False
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    B = sp.csr_matrix((A.data[keep], (rows[keep], A.indices[keep])), shape=A.shape)
    assert B.nnz == A.nnz - 1
    return B


@pytest.mark.parametrize("kind", BITE_KINDS)
@pytest.mark.parametrize("lane", L.LANES)
def test_the_comparison_rejects_a_reference_wrong_by_one_entry_or_one_iteration(oracle, lane, kind):
    """The comparison of the fixed cuts must bite at k = 1: the restatement run on the same matrix less ONE entry of its longest
    row, or of its longest column, and the result of cut k + 1 offered as that of cut k, are both refused -- on their VECTORS, not
    only on an iteration count -- with the very allowance the GPU test grants."""
    ins = L.inputs(kind)
    for delta in L.DELTAS:
        want = L.cut_reference(oracle, lane, kind, delta, 1)
        tol = L.allowance(L.spread(oracle, lane, kind, delta, 1), 1)
        L.compare(want, want, tol)   # (and accepts what it should)
        for order in (1, 2):
            L.compare(L.cut_reference(oracle, lane, kind, delta, 1, order), want, tol)
        for longest in ("row", "column"):
            wrong = L.restate(oracle, lane, ins, delta, L.cut_options(lane, 1), csr=L.csr_arrays(_without_one_entry(ins["A"], longest)))
            with pytest.raises(AssertionError, match="vector"):
                L.compare(wrong, want, tol, f"{lane} {kind} less one entry of its longest {longest}")
        with pytest.raises(AssertionError, match="vector") as late:
            L.compare(L.cut_reference(oracle, lane, kind, delta, 2), want, tol, f"{lane} {kind} one iteration late")
        assert "niter" in str(late.value)


@pytest.mark.parametrize("kind", ALL_KINDS)
@pytest.mark.parametrize("lane", L.LANES)
def test_the_restatement_run_to_the_end_reaches_the_exact_solve(oracle, lane, kind):
    """Part (b) of the GPU test compares the device, its stopping tests tightened and its conditioning limits off, with exact
    solves; its tolerance is max(1e-9, 10 x what the restatement reaches).  The restatement reaches 1e-7 on all 21 (lane, kind)
    -- 2.0e-12 at worst, profiles/lane_structures.md -- so none is left out there."""
    reached = L.exact_distance(L.tight_reference(oracle, lane, kind, 0.25), L.exact(oracle, lane, kind, 0.25))
    assert reached < 1e-7
    assert all(st[2] == 1 for call in L.tight_reference(oracle, lane, kind, 0.25) for st in call[1])
