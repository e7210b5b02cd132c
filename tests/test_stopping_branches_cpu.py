"""What tests/test_gpu_stopping_branches.py relies on, pinned with the C restatement alone (no GPU): every case of
tests/stopping_cases.py reaches the exit of the Krylov lanes it is named for, with the same (niter, status, solved, inconsistent)
and return code in the restatement's three summation orders -- the literals of stopping_cases.EXPECT --; a case driven by a limit
does not sit on the edge of that limit; the restatement's own spread stays inside the caps of lane_cases.allowance; and the
comparison the GPU test asserts with refuses the result of another branch, or one nonzero in a vector that must stay zero."""
import numpy as np
import pytest

import lane_cases as L
import stopping_cases as S

COMBOS = S.combos()
IDS = ["-".join(c) for c in COMBOS]


@pytest.mark.parametrize("name,key,lane", COMBOS, ids=IDS)
def test_every_case_gives_its_literals_in_the_three_summation_orders(oracle, name, key, lane):
    for delta in S.CASES[name].deltas:
        want = S.expected(name, key, lane, delta)
        for order in (0, 1, 2):
            calls = S.reference(oracle, name, key, lane, delta, order)
            assert S.literals(calls) == want, (delta, order)
            assert L.is_finite(calls), (delta, order)


def test_the_table_of_literals_is_the_table_of_cases():
    assert sorted(S.EXPECT) == sorted("/".join(c) for c in COMBOS)
    for name, case in S.CASES.items():
        assert case.hits, name
        for lane, call, system, status in case.hits:
            assert lane in case.lanes
            for key in case.matrices:   # the branch the case is named for, at one delta at least and as a literal
                assert any(S.expected(name, key, lane, d)[call][1 + system][1] == status for d in case.deltas), (name, key, lane)
    # every status value of include/fpsq.h is the literal of some case on the tiny matrix or the identity
    seen = {st[1] for k, e in S.EXPECT.items() if "/mid/" not in k for per in e for call in per for st in call[1:]}
    assert seen == set(range(1, 10))


def test_the_ill_conditioned_and_solved_case_really_is_both(oracle):
    """ill-cond-and-solved ends LSQR as SOLVED (3): the status alone does not show that ill_cond fired in the same iteration.
    Without the rtol that solves it the lane ends in that very iteration as ILL_COND."""
    for key in S.CASES["ill-cond-and-solved"].matrices:
        ins = S.case_inputs("ill-cond-and-solved", key)
        opts = {k: v for k, v in S.case_options("ill-cond-and-solved", "mixed").items() if k != "ls_rtol"}
        for delta in S.DELTAS:
            assert S.literals(L.restate(oracle, "mixed", ins, delta, opts, full=True))[0][1] == (1, 6, 0, 1)
            assert S.expected("ill-cond-and-solved", key, "mixed", delta)[0][1:] == ((1, 3, 1, 1), (1, 6, 1, 0))


@pytest.mark.parametrize("name", [n for n, c in S.CASES.items() if c.limits])
def test_limit_driven_cases_do_not_sit_on_the_edge(oracle, name):
    """The driving limit moved by 1 % either way: the same (niter, status, solved, inconsistent) and return code.  A condition on
    the inputs: a case that fails here is replaced, not tolerated."""
    case = S.CASES[name]
    for key in case.matrices:
        for lane in case.lanes:
            for delta in case.deltas:
                want = S.expected(name, key, lane, delta)
                for option in case.limits:
                    for factor in (0.99, 1.01):
                        got = S.literals(S.reference(oracle, name, key, lane, delta, 0, (option, factor)))
                        assert got == want, (key, lane, delta, option, factor)


@pytest.mark.parametrize("name,key,lane", COMBOS, ids=IDS)
def test_the_spread_stays_inside_the_caps_and_the_orders_pass_the_comparison(oracle, name, key, lane):
    for delta in S.CASES[name].literals_only:   # (left out of the comparison for this reason and no other)
        with pytest.raises(AssertionError, match="asks for more than the cap"):
            S.allowance(oracle, name, key, lane, delta)
    for delta in S.held_deltas(name):
        tol = S.allowance(oracle, name, key, lane, delta)   # (asserts the caps of lane_cases.allowance)
        want = S.reference(oracle, name, key, lane, delta)
        for order in (1, 2):
            L.compare(S.reference(oracle, name, key, lane, delta, order), want, tol, f"order {order} delta={delta:.3g}")
        print(f"{name} {key} {lane} delta={delta:.3g}: spread {S.spread(oracle, name, key, lane, delta):.1e} allowance {tol:.1e}")


@pytest.mark.parametrize("name,key,lane", [c for c in COMBOS if c[0] != "baseline" and c[1] != "ident"], ids=lambda v: v)
def test_the_comparison_refuses_the_result_of_the_baseline(oracle, name, key, lane):
    """compare() of a case's reference against the baseline's fails: a device that took the ordinary branch would not pass."""
    for delta in S.CASES[name].literals_only:
        assert S.literals(S.reference(oracle, "baseline", key, lane, delta)) != S.expected(name, key, lane, delta)
    for delta in S.held_deltas(name):
        want = S.reference(oracle, name, key, lane, delta)
        with pytest.raises(AssertionError):
            L.compare(S.reference(oracle, "baseline", key, lane, delta), want, S.allowance(oracle, name, key, lane, delta))


def test_the_comparison_refuses_the_ordinary_result_on_the_identity(oracle):
    """The half-step that is skipped: the same inputs with g moved off the identity block (no beta == 0) give another result."""
    for lane in S.CASES["skip-half-step"].lanes:
        for delta in S.DELTAS:
            want = S.reference(oracle, "skip-half-step", "ident", lane, delta)
            ins = dict(S.case_inputs("skip-half-step", "ident"))
            ins["g"] = ins["g"] + 0.5 * S.inputs("ident")["vec"]["r1"]
            other = L.restate(oracle, lane, ins, delta, S.case_options("skip-half-step", lane), full=True)
            with pytest.raises(AssertionError):
                L.compare(other, want, S.allowance(oracle, "skip-half-step", "ident", lane, delta))


@pytest.mark.parametrize("name", [n for n, c in S.CASES.items() if c.zero])
def test_vectors_of_a_lane_that_never_updates_are_zero_and_one_planted_nonzero_is_refused(oracle, name):
    case = S.CASES[name]
    for key in case.matrices:
        for lane, call, vec in case.zero:
            for delta in case.deltas:
                want = S.reference(oracle, name, key, lane, delta)
                assert not want[call][2][vec].any(), (key, lane, call, vec, delta)
                planted = [(rc, st, [v.copy() for v in vecs]) for rc, st, vecs in want]
                planted[call][2][vec][planted[call][2][vec].size // 2] = 1e-300
                with pytest.raises(AssertionError, match="vector"):
                    L.compare(planted, want, S.allowance(oracle, name, key, lane, delta))
                assert S.exactly_zero_where_the_reference_is(want, want)
                assert not S.exactly_zero_where_the_reference_is(planted, want)
