"""The LNLQ and MINRES lanes of the device Krylov loop on the awkward Jacobian structures (run with -m gpu on an MI355X).

LSQR and CRAIG are held to the C restatement iteration for iteration on all seven kinds of tests/structures.py
(tests/test_gpu_parity.py: test_recurrences_agree_iteration_for_iteration_before_rounding_grows).  The other recurrences have
update segments, scalar steps, a coefficient block for the A' product (MinresState::ctlT), a merged launch (k_minres_mid) and a
one-iteration reporting lag of their own, all riding inside the product launches and therefore depending on the layouts' block
counts.  Here they get the same treatment, through the C ABI:

  lnlq      fpsq_solve_two_mixed, ln_method = FPSQ_LN_LNLQ (LSQR in lane 0, LNLQ in lane 1)
  extras    fpsq_solve_two_extras (LSQR in lane 0, MINRES on A A' + tau I in lane 1): what hprod! Val(1) calls
  minres-k  fpsq_solve_two_mixed and fpsq_solve_two_least_squares, kkt_method = FPSQ_KKT_MINRES_K

 (a) cut at k = 1, 2, 3 iterations, against the restatement in its default summation order;
 (b) run to the end against exact solves;
 (c) the launch-shape switches FPSQ_RIDE_LEAD and FPSQ_MINRES_MERGE, bitwise, with proof that they engaged.
Inputs, references and the comparison rule are tests/lane_cases.py, pinned on the CPU by tests/test_lane_structures_cpu.py;
measurements are in profiles/lane_structures.md.  Everything is fp64."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import fps_amd  # noqa: F401
from fps_amd import _lib

import lane_cases as L
from abi_handle import _Handle, _rel
from structures import ALL_KINDS

pytestmark = pytest.mark.gpu


def _fuses(lane):
    """fuse_two_rhs picks run_krylov<2> (both lanes in one lock-step loop) or two loops of one lane for lnlq and extras.
    minres_k_device never reads it -- both systems always run in lock-step on interleaved vectors -- so it launches the same
    kernels for 0 and 1 and minres-k keeps the default only."""
    return (1,) if lane == "minres-k" else (0, 1)


def _device(lane, kind, delta, fmt, fuse, opts, check_products=True):
    """The lane's calls on a fresh handle (closed here), in the form of lane_cases.restate()."""
    ins = L.inputs(kind)
    if lane == "minres-k":
        opts = {**opts, "kkt_method": 1}
    H = _Handle(ins["A"], delta=delta, fuse_two_rhs=fuse, jac_format=fmt, **opts)
    try:
        if check_products:   # (a failure of a product is reported as one, not as a failure of a recurrence)
            As = sp.csr_matrix(ins["A"])
            assert _rel(H.jac_mul(0, 1.0, ins["x"], 0.0, np.zeros(ins["m"])), As @ ins["x"]) < 1e-13
            assert _rel(H.jac_mul(1, 1.0, ins["u"], 0.0, np.zeros(ins["n"])), As.T @ ins["u"]) < 1e-13
        if lane == "lnlq":
            entries = [(H.solve_two_mixed, ins["g"], ins["c"])]
        elif lane == "extras":
            entries = [(H.solve_two_extras, ins["r1"], ins["r2"])]
        else:
            entries = [(H.solve_two_mixed, ins["g"], ins["c"]), (H.solve_two_least_squares, ins["g"], ins["r1"])]
        calls = []
        for fn, a, b in entries:
            *vecs, rc = fn(a, b)
            calls.append((rc, [(H.st[i].niter, H.st[i].status, H.st[i].solved, H.st[i].rnorm, H.st[i].arnorm) for i in range(2)], vecs))
        info = _lib.Info()
        assert H.lib.fpsq_get_info(H.h, C.byref(info)) == 0
        return calls, int(info.last_kernel_launches)
    finally:
        H.close()


# ------------------------------------------------------------------------------------------------ (a) fixed cuts

@pytest.mark.parametrize("fmt", [0, 1])  # 0: RGCS / padded / 16-bit-column layouts where representable, 1: plain CSR
@pytest.mark.parametrize("kind", ALL_KINDS)
@pytest.mark.parametrize("lane", L.LANES)
def test_lanes_agree_with_the_restatement_at_fixed_cuts(oracle, lane, kind, fmt):
    """Device and C restatement cut at k = 1, 2, 3 iterations (ls_itmax / ln_itmax / ne_itmax = k), delta in {0, sqrt(eps), 0.25},
    fuse_two_rhs in {0, 1} (see _fuses), a fresh handle per cut: equal return codes, equal (niter, status, solved) per lane -- lane
    0 of the lnlq call is LSQR and is held to the same --, rnorm / arnorm within tol * max(|want|, 1), every output vector within
    tol in relative inf-norm.  tol = max(1e-12, 20 x the restatement's own spread over its three summation orders at the same
    (lane, kind, delta, k)), capped at 1e-11 for k = 1 and 1e-6 for every cut (lane_cases.allowance fails rather than widen;
    measured spreads: profiles/lane_structures.md -- 7.9e-14 at k = 1 and 7.1e-9 at k = 3 at worst, LNLQ on dense-row).  A
    misplaced coefficient, a partial sum over the wrong number of blocks or a lagged step reading the wrong state copy is an
    O(1) difference at k = 1.  Before each cut, A v and A' u of the same handle against scipy to 1e-13.  (On `tiny` the lanes
    finish before the cut and the LNLQ lane ends on a Golub-Kahan beta that is zero up to rounding, or exactly: see
    test_lnlq_restatement_survives_the_exact_breakdown_of_a_one_row_jacobian in tests/test_lane_structures_cpu.py.)"""
    for delta in L.DELTAS:
        for k in L.CUTS:
            want = L.cut_reference(oracle, lane, kind, delta, k)
            spread = L.spread(oracle, lane, kind, delta, k)
            tol = L.allowance(spread, k)
            for fuse in _fuses(lane):
                got, _ = _device(lane, kind, delta, fmt, fuse, L.cut_options(lane, k))
                print(f"cut {lane} {kind} fmt={fmt} delta={delta:.3g} k={k} fuse={fuse}: spread {spread:.1e} tol {tol:.1e} "
                      f"device vectors {L.vector_distance(got, want):.1e} estimates {L.estimate_distance(got, want):.1e} "
                      f"stats {[s[:3] for c in got for s in c[1]]}")
                L.compare(got, want, tol, f"{lane} {kind} fmt={fmt} delta={delta:.3g} k={k} fuse={fuse}")


# ------------------------------------------------------------------------------------------------ (b) to the end

@pytest.mark.parametrize("kind", ALL_KINDS)
@pytest.mark.parametrize("lane", L.LANES)
def test_lanes_run_to_the_exact_solve(oracle, lane, kind):
    """delta = 0.25, the stopping tests tightened (lane_cases.TIGHT: 1e-15 for LSQR and LNLQ, ne_atol = ne_rtol = 1e-14 and
    ne_etol = 1e-16 for MINRES, every conditioning limit off): the device reaches the exact answers -- exact_two_extras; the
    exact KKT solves for MINRES on K; for LNLQ the minimum-norm solution of A x = -c, unregularised whatever delta -- to
    max(1e-9, 10 x what the restatement reaches with the same options), never more than 1e-6.  The restatement reaches 2.0e-12
    at worst (profiles/lane_structures.md), so the bound is 1e-9 on all 21 (lane, kind) and none is left out.  Beyond
    n + m = 7000 the exact solves go through a factorisation of A A' + delta I (lane_cases._kkt_by_elimination)."""
    delta = 0.25
    ex = L.exact(oracle, lane, kind, delta)
    reached = L.exact_distance(L.tight_reference(oracle, lane, kind, delta), ex)
    assert reached < 1e-7   # (else the combination would have to be left out: none is)
    tol = min(max(1e-9, 10 * reached), 1e-6)
    for fuse in _fuses(lane):
        got, _ = _device(lane, kind, delta, 0, fuse, L.tight_options(lane))
        dist = L.exact_distance(got, ex)
        print(f"end {lane} {kind} fuse={fuse}: restatement {reached:.1e} device {dist:.1e} tol {tol:.1e} "
              f"stats {[s[:3] for c in got for s in c[1]]}")
        assert all(c[0] == 0 for c in got)
        assert dist < tol, (fuse, dist, tol)


# ------------------------------------------------------------------------------------------------ (c) the switches

SWITCHES = [("extras", "FPSQ_MINRES_MERGE"), ("extras", "FPSQ_RIDE_LEAD"), ("lnlq", "FPSQ_RIDE_LEAD")]
ENGAGE_KINDS = ["dense-row", "dense-column", "empty-columns"]
_AB = {}


def _switch_ab(monkeypatch, lane, switch, kind):
    """The lane's calls at default tolerances with the switch off and on (set before the handle is created): (calls, launches)
    for either setting.  Kept for the engagement test."""
    key = (lane, switch, kind)
    if key not in _AB:
        runs = []
        for value in ("0", "1"):
            monkeypatch.setenv(switch, value)
            opts = {"ln_method": 1} if lane == "lnlq" else {}
            runs.append(_device(lane, kind, 0.25, 0, 1, opts, check_products=False))
        _AB[key] = runs
    return _AB[key]


@pytest.mark.parametrize("kind", ALL_KINDS)
@pytest.mark.parametrize("lane,switch", SWITCHES)
def test_launch_shape_switches_are_bitwise_neutral_on_the_structures(monkeypatch, lane, switch, kind):
    """FPSQ_RIDE_LEAD = 0 / 1 (the scalar steps in launches of their own, or riding with leader workgroups of the next product)
    for the LNLQ and the extras call, FPSQ_MINRES_MERGE = 0 / 1 (MINRES' stage E1, step A and stage E2 as three launches or as
    k_minres_mid) for the extras call: the same sums in the same order, so every output vector and every statistic is BITWISE
    the same -- what test_minres_stages_in_one_launch_are_bitwise_the_three_launches and
    test_steps_riding_with_leaders_are_bitwise_the_stand_alone_steps assert on PDE-like matrices, here on all seven kinds at
    default tolerances, delta = 0.25."""
    (off, l_off), (on, l_on) = _switch_ab(monkeypatch, lane, switch, kind)
    print(f"switch {lane} {switch} {kind}: launches {l_off} -> {l_on} stats {[s[:3] for c in on for s in c[1]]}")
    for (rc0, st0, v0), (rc1, st1, v1) in zip(off, on):
        assert rc0 == rc1 and st0 == st1
        for a, b in zip(v0, v1):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("lane,switch", SWITCHES)
def test_launch_shape_switches_engage_on_a_hard_structure(monkeypatch, lane, switch):
    """The A/B above must not compare a path with itself: on at least one of dense-row, dense-column, empty-columns the switch
    changes fpsq_info.last_kernel_launches of the call."""
    changed = []
    for kind in ENGAGE_KINDS:
        (_, l_off), (_, l_on) = _switch_ab(monkeypatch, lane, switch, kind)
        if l_off != l_on:
            changed.append(kind)
    print(f"switch {lane} {switch}: launch count changes on {changed}")
    assert changed
