"""Every stopping branch of the device Krylov lanes (csrc/fpsq_krylov.hip.h) against the C restatement, on inputs built to reach
it (run with -m gpu on an MI355X).  Cases, references, literals and the comparison rule are tests/stopping_cases.py, pinned on the
CPU by tests/test_stopping_branches_cpu.py.

 (a) every case through every entry point that drives its lane, on a fresh handle with default switches: return code and
     (niter, status, solved, inconsistent) per lane EQUAL TO THE LITERALS of stopping_cases.EXPECT, rnorm / arnorm and every vector
     within lane_cases.allowance of the restatement's own spread at that case; outputs preset to NaN come back finite, and exactly
     zero where a lane ended before its first update;
 (b) the forms of the driver (fuse_two_rhs = 0, two launches per iteration, one launch wherever possible, several iterations per
     launch, the two-launch tail of the qp entries) bitwise the default form; CRAIG with x carried through its loop to rounding;
 (c) the history of a handle: the case between ordinary calls, twice in a row, and with the run-ahead count placed before, at and
     behind the true end (fpsq_debug_expect_iterations) -- every call bitwise what a fresh handle gives, statistics included.
A lane that ends at iteration 0 or 1 leaves the host driver (csrc/fpsq_run.hip.h) with its blindly enqueued iterations falling
through, its gated epilogue behind an iteration that never runs, and an expected count of 0 or 1 for the next call.
Everything is fp64; fuse_fallbacks / wait_timeouts / p2p_timeouts stay 0 (tests/conftest.py holds every handle destroyed to it)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import fps_amd  # noqa: F401
from fps_amd import _lib, problems
from fps_amd.device_qp import DeviceEqQP

import lane_cases as L
import stopping_cases as S
from abi_handle import _Handle

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
SIGMA, RHO = 2.0, 1.0
SMALL = [c for c in S.combos(("tiny", "ident"))]
MID = [c for c in S.combos(("mid",))]
ids = "-".join


def _options(name, lane):
    opts = S.case_options(name, lane)
    if lane == "minres-k":
        opts["kkt_method"] = 1
    return opts


def _entries(H, lane, ins):
    mixed, lsq = (H.solve_two_mixed, ins["g"], ins["c"]), (H.solve_two_least_squares, ins["g"], ins["r1"])
    return {"mixed": [mixed], "lnlq": [mixed], "lsq": [lsq], "extras": [(H.solve_two_extras, ins["r1"], ins["r2"])],
            "minres-k": [mixed, lsq]}[lane]


def _calls(H, lane, ins, expect=None):
    """The lane's calls on this handle, in the form of lane_cases.restate(full=True); expect: the run-ahead count of each call."""
    calls = []
    for fn, a, b in _entries(H, lane, ins):
        if expect is not None:
            H.expect(expect)
        *vecs, rc = fn(a, b)
        calls.append((rc, H.stats(), vecs))
    return calls


def _fresh(name, key, lane, delta, ins=None, monkeypatch=None, env=None, repeat=1, **more):
    """The case's calls on a handle of its own (closed here), created under `env`.  repeat: the calls are made that often --
    from the second time on the handle has an expected count, which several iterations per launch need -- and must not change."""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    H = _Handle(S.inputs(key)["A"], delta=delta, **{**_options(name, lane), **more})
    for k in env or {}:
        monkeypatch.delenv(k)
    try:
        calls = _calls(H, lane, ins or S.case_inputs(name, key))
        for again in range(1, repeat):
            _same_bits(_calls(H, lane, ins or S.case_inputs(name, key)), calls, f"repetition {again}")
        info = _lib.Info()
        assert H.lib.fpsq_get_info(H.h, C.byref(info)) == 0
        assert H.counters() == (0, 0, 0)
        return calls, int(info.last_fused_launches), int(info.last_multi_iterations)
    finally:
        H.close()


_DEFAULT = {}


def _default(name, key, lane, delta):
    k = (name, key, lane, float(delta))
    if k not in _DEFAULT:
        _DEFAULT[k] = _fresh(name, key, lane, delta)[0]
    return _DEFAULT[k]


def _same_bits(got, want, what):
    assert len(got) == len(want)
    for ic, ((rc_g, st_g, v_g), (rc_w, st_w, v_w)) in enumerate(zip(got, want)):
        assert rc_g == rc_w and st_g == st_w, (what, ic, rc_g, rc_w, st_g, st_w)
        for i, (a, b) in enumerate(zip(v_g, v_w)):
            assert np.array_equal(a, b), (what, ic, i, float(np.max(np.abs(a - b))))


# ------------------------------------------------------------------------------------------------ (a) the default form

@pytest.mark.parametrize("name,key,lane", SMALL + MID, ids=[ids(c) for c in SMALL + MID])
def test_every_stopping_branch_matches_its_literals_and_the_restatement(oracle, name, key, lane):
    """Fresh handle, default switches, every delta of the case: the literals of stopping_cases.EXPECT exactly (return code, niter,
    status, solved, inconsistent), lane_cases.compare against the restatement with the allowance of its own spread at this case
    (max(1e-12, 20 x spread), capped at 1e-11 where no lane passes iteration 1 and at 1e-6 anywhere), finite outputs that are exactly
    zero where the restatement's are.  (That the literals hold every status 1 .. 9 is asserted by the CPU test of the table; at a
    delta the case lists as literals_only the distance to the restatement is printed, not held.)  For the lanes fpsq_ys_gs serves, the same handle then gives v, w bitwise p2, q2 and gs, ys
    within one rounding of p1 + sigma p2, q1 + sigma q2, with the same return code and statistics."""
    ins = S.case_inputs(name, key)
    for delta in S.CASES[name].deltas:
        want = S.reference(oracle, name, key, lane, delta)
        held = delta not in S.CASES[name].literals_only   # (else the restatement's own orders are too far apart: literals only)
        tol = S.allowance(oracle, name, key, lane, delta) if held else float("nan")
        H = _Handle(S.inputs(key)["A"], delta=delta, **_options(name, lane))
        try:
            got = _calls(H, lane, ins)
            print(f"{name} {key} {lane} delta={delta:.3g}: {S.literals(got)} spread {S.spread(oracle, name, key, lane, delta):.1e} "
                  f"tol {tol:.1e} vectors {L.vector_distance(got, want):.1e} estimates {L.estimate_distance(got, want):.1e}")
            assert S.literals(got) == S.expected(name, key, lane, delta), delta
            if held:
                L.compare(got, want, tol, f"{name} {key} {lane} delta={delta:.3g}")
            assert S.exactly_zero_where_the_reference_is(got, want), delta
            if lane in ("mixed", "lnlq", "minres-k"):
                rc0, st0, (p1, q1, p2, q2) = got[0]
                gs, ys, v, w, rc = H.ys_gs(ins["g"], ins["c"], SIGMA)
                assert rc == rc0 and H.stats() == st0, delta
                assert np.array_equal(v, p2) and np.array_equal(w, q2), delta
                assert np.all(np.abs(gs - (p1 + SIGMA * p2)) <= 4 * EPS * (np.abs(p1) + SIGMA * np.abs(p2))), delta
                assert np.all(np.abs(ys - (q1 + SIGMA * q2)) <= 4 * EPS * (np.abs(q1) + SIGMA * np.abs(q2))), delta
            assert H.counters() == (0, 0, 0)
        finally:
            H.close()
        _DEFAULT[(name, key, lane, float(delta))] = got


# ------------------------------------------------------------------------------------------------ the qp entries

def _qp(name, key):
    """A diagonal QP over the case's matrix whose evaluation at x = 0 hands the case's right-hand sides to the solves exactly:
    g = q .* 0 + d = d, c = A 0 - b = -b."""
    ins = S.case_inputs(name, key)
    A, n, m = ins["A"], ins["n"], ins["m"]
    q = 1.0 + (np.arange(n) % 5) / 4.0
    return problems.EqQP(f"{name}/{key}", n, m, A.indptr.astype(np.int32), A.indices.astype(np.int32), np.ascontiguousarray(A.data),
                         q, ins["g"].copy(), -ins["c"], np.zeros(n), np.zeros(n))


def _stat4(s):
    return (s.niter, s.status, s.solved, s.inconsistent)


def _objgrad(dev, x, expect=None):
    n, m = dev.qp.n, dev.qp.m
    gx, ys, gs = np.full(n, np.nan), np.full(m, np.nan), np.full(n, np.nan)
    if expect is not None:
        assert dev._lib.fpsq_debug_expect_iterations(dev._h, expect) == 0
    fx, rc = dev.objgrad(x, gx=gx, ys=ys, gs=gs)
    return rc, [(s.niter, s.status, s.solved, s.rnorm, s.arnorm, s.inconsistent) for s in dev.stats], [np.array([fx]), gx, ys, gs]


def _hprod(dev, v, approx, expect=None):
    hv = np.full(dev.qp.n, np.nan)
    if expect is not None:
        assert dev._lib.fpsq_debug_expect_iterations(dev._h, expect) == 0
    rc = dev.hprod(v, hv, approx)
    st = [(s.niter, s.status, s.solved, s.rnorm, s.arnorm, s.inconsistent) for s in list(dev.stats4)[: 2 if approx == 2 else 4]]
    return rc, st, [hv]


def _qp_kinds(name):
    """The qp entries a case is driven through: objgrad on its solve_two_mixed lanes, hprod (Val(2) and Val(1)) on its LSQR lanes
    when the branch does not hang on the second right-hand side (hprod's is q .* v)."""
    case = S.CASES[name]
    kinds = [("objgrad", lane) for lane in ("mixed", "lnlq") if lane in case.lanes]
    if "lsq" in case.lanes and "r1" not in case.rhs:
        kinds += [("hprod2", "lsq"), ("hprod1", "lsq")]
    return kinds


def _qp_reference(oracle, kind, qp, delta, opts, order=0):
    o = oracle.default_options(qp.n, qp.m, **opts)
    try:
        oracle.set_sum_order(order)
        if kind == "objgrad":
            r = oracle.qp_objgrad(qp, qp.x, SIGMA, RHO, delta, opts=o)
            return r["rc"], [L._stats(s, True) for s in r["stats"]], [np.array([r["fx"]]), r["gx"], r["ys"], r["gs"]]
        approx = 2 if kind == "hprod2" else 1
        r = oracle.qp_hprod(qp, qp.d, SIGMA, RHO, delta, approx=approx, opts=o)
        return r["rc"], [L._stats(s, True) for s in r["stats"][: 2 if approx == 2 else 4]], [r["Hv"]]
    finally:
        oracle.set_sum_order(0)


def _qp_device(kind, dev, x_or_v=None, expect=None):
    if kind == "objgrad":
        return _objgrad(dev, dev.qp.x if x_or_v is None else x_or_v, expect)
    return _hprod(dev, dev.qp.d if x_or_v is None else x_or_v, 2 if kind == "hprod2" else 1, expect)


QP_SMALL = [(n, k, kind, lane) for n, c in S.CASES.items() for k in c.matrices if k != "mid" for kind, lane in _qp_kinds(n)]
QP_MID = [(n, k, kind, lane) for n, c in S.CASES.items() for k in c.matrices if k == "mid" for kind, lane in _qp_kinds(n)]


@pytest.mark.parametrize("name,key,kind,lane", QP_SMALL, ids=[ids(c) for c in QP_SMALL])
def test_qp_entries_reach_the_same_branches(oracle, monkeypatch, name, key, kind, lane):
    """fpsq_qp_objgrad at x = 0 of a diagonal QP with d = g, b = -c (the solves get the case's right-hand sides exactly), and
    fpsq_qp_hprod with hessian_approx 2 and 1 on v = g, against oracle.qp_objgrad / oracle.qp_hprod with the same options:
    return code and (niter, status, solved, inconsistent) of every recurrence exactly -- those of the case's own lanes equal to
    the literals of stopping_cases.EXPECT --, fx / gx / ys / gs / Hv within lane_cases.allowance of the restatement's spread over its
    three summation orders on this evaluation.  Then FPSQ_FUSE_TAIL=0 (the tail as two launches), bitwise."""
    qp = _qp(name, key)
    opts = S.case_options(name, lane)
    for delta in S.CASES[name].deltas:
        want = _qp_reference(oracle, kind, qp, delta, opts)
        alts = [_qp_reference(oracle, kind, qp, delta, opts, order) for order in (1, 2)]
        for alt in alts:
            assert S.literals([alt]) == S.literals([want])
        spread = max(L.spread_of([want], [[a] for a in alts]), max(L.estimate_distance([a], [want]) for a in alts))
        held = delta not in S.CASES[name].literals_only   # (else: return code and statistics only)
        tol = L.allowance(spread, max(1, max(s[0] for s in want[1]))) if held else float("nan")
        dev = DeviceEqQP(qp, sigma=SIGMA, rho=RHO, delta=delta, **opts)
        got = _qp_device(kind, dev)
        dev.close()
        print(f"{name} {key} {kind} {lane} delta={delta:.3g}: {S.literals([got])} spread {spread:.1e} tol {tol:.1e} "
              f"vectors {L.vector_distance([got], [want]):.1e}")
        lit = S.expected(name, key, lane, delta)[0]
        if kind == "objgrad":
            assert S.literals([got])[0] == lit, delta
        else:   # (the first system is the case's; the second has q .* v for a right-hand side)
            assert S.literals([got])[0][1] == lit[1], delta
            if kind == "hprod1":
                assert got[1][3][:3] == (0, 1, 1)   # MINRES on the zero right-hand side Ssv: ZERO_RHS
        if held:
            L.compare([got], [want], tol, f"{name} {key} {kind} delta={delta:.3g}")
        else:
            assert S.literals([got]) == S.literals([want]), delta
        assert L.is_finite([got])
        monkeypatch.setenv("FPSQ_FUSE_TAIL", "0")
        dev = DeviceEqQP(qp, sigma=SIGMA, rho=RHO, delta=delta, **opts)
        monkeypatch.delenv("FPSQ_FUSE_TAIL")
        two = _qp_device(kind, dev)
        dev.close()
        _same_bits([two], [got], f"FPSQ_FUSE_TAIL=0 delta={delta:.3g}")


def test_qp_entries_refuse_minres_on_k():
    """kkt_method = FPSQ_KKT_MINRES_K serves the three seam entries only (include/fpsq.h): the qp entries return FPSQ_ERR_STATE."""
    qp = _qp("baseline", "tiny")
    dev = DeviceEqQP(qp, sigma=SIGMA, rho=RHO, delta=0.25, kkt_method=1)
    fx, out = C.c_double(), np.full(qp.n, np.nan)
    lib = dev._lib
    assert lib.fpsq_qp_objgrad(dev._h, dev._q, qp.x.ctypes.data, SIGMA, RHO, 0.0, None, C.byref(fx), out.ctypes.data, None, None,
                               dev.stats) == -3
    for approx in (2, 1):
        assert lib.fpsq_qp_hprod(dev._h, dev._q, qp.d.ctypes.data, SIGMA, RHO, 0.0, approx, out.ctypes.data, dev.stats4) == -3
    dev.close()


# ------------------------------------------------------------------------------------------------ (b) the forms of the driver

ALIGNED = {"FPSQ_AT_ROW_ALIGN": "8"}   # (the A' block boundaries of the default handle: the same partial sums)
FORMS = [("fuse_two_rhs=0", {}, dict(fuse_two_rhs=0)),
         ("two launches", {"FPSQ_FUSE_ITER": "0", **ALIGNED}, {}),
         ("one launch wherever possible", {"FPSQ_FUSE_ITER": "2"}, {}),
         ("FPSQ_MULTI_ITER=3", {"FPSQ_MULTI_ITER": "3"}, {}),
         ("one launch, FPSQ_MULTI_ITER=3", {"FPSQ_FUSE_ITER": "2", "FPSQ_MULTI_ITER": "3"}, {})]


@pytest.mark.parametrize("name,key,lane", SMALL, ids=[ids(c) for c in SMALL])
def test_every_form_of_the_driver_is_bitwise_the_default_form(monkeypatch, name, key, lane):
    """fuse_two_rhs = 0 (two loops of one lane), FPSQ_FUSE_ITER=0 (two launches per iteration, on the default handle's A' block
    boundaries), FPSQ_FUSE_ITER=2 (one launch wherever the layouts allow), FPSQ_MULTI_ITER=3 alone and with it: return codes,
    statistics and every vector BITWISE the default form's, for every delta of the case -- a lane that ends at start-up, at
    iteration 1 or with a skipped half-step ends the same way in every form.  Every form makes its calls twice on its handle (a
    first call has no expected count and runs one iteration per launch)."""
    for delta in S.CASES[name].deltas:
        want = _default(name, key, lane, delta)
        for what, env, more in FORMS:
            got, fused, multi = _fresh(name, key, lane, delta, monkeypatch=monkeypatch, env=env, repeat=2, **more)
            print(f"{name} {key} {lane} delta={delta:.3g} {what}: one-launch iterations {fused}, of them sharing a launch {multi}")
            _same_bits(got, want, f"{what} delta={delta:.3g}")
            if (name, lane) == ("baseline", "mixed") and env.get("FPSQ_FUSE_ITER") == "2":   # (not a path against itself)
                assert fused > 0 and (multi > 0) == ("FPSQ_MULTI_ITER" in env)


@pytest.mark.parametrize("name,key,lane", MID, ids=[ids(c) for c in MID])
def test_two_launch_and_one_launch_iterations_agree_on_the_mid_size_matrix(monkeypatch, name, key, lane):
    """The same at the size where the products span several workgroups and the leaders are not alone in the grid: two launches per
    iteration and one launch per iteration, bitwise the default form (which keeps a grid of this size on two launches)."""
    for delta in S.CASES[name].deltas:
        want = _default(name, key, lane, delta)
        two, fused0, _ = _fresh(name, key, lane, delta, monkeypatch=monkeypatch, env={"FPSQ_FUSE_ITER": "0", **ALIGNED})
        one, fused2, _ = _fresh(name, key, lane, delta, monkeypatch=monkeypatch, env={"FPSQ_FUSE_ITER": "2"})
        print(f"{name} {key} {lane} delta={delta:.3g}: one-launch iterations {fused0} / {fused2}")
        _same_bits(two, want, f"two launches delta={delta:.3g}")
        _same_bits(one, want, f"one launch delta={delta:.3g}")
        assert fused0 == 0
        if (name, lane) == ("baseline", "mixed"):   # (the A/B does not compare a path with itself)
            assert fused2 > 0


CRAIG = [c for c in SMALL if c[2] == "mixed"]


@pytest.mark.parametrize("name,key,lane", CRAIG, ids=[ids(c) for c in CRAIG])
def test_craig_with_x_in_its_loop_ends_the_same_way(monkeypatch, name, key, lane):
    """FPSQ_CRAIG_X=1 carries x through the CRAIG loop where the default forms p2 = -A'q2 once behind it: return code, statistics,
    p1, q1, q2 bitwise; p2 to the rounding bound of tests/test_gpu_craig_x_from_y.py, ||dp2|| <= 8 eps (iterations + longest row
    of A') ||p2|| -- and exactly zero where the lane never updates (INCONSISTENT, ZERO_RHS, solved at start-up)."""
    longest = int(np.max(np.diff(sp.csc_matrix(S.inputs(key)["A"]).indptr)))
    for delta in S.CASES[name].deltas:
        (rc0, st0, v0), = _default(name, key, lane, delta)
        ((rc1, st1, v1),), _, _ = _fresh(name, key, lane, delta, monkeypatch=monkeypatch, env={"FPSQ_CRAIG_X": "1"})
        assert rc0 == rc1 and st0 == st1
        for i in (0, 1, 3):
            assert np.array_equal(v0[i], v1[i]), i
        bound = 8 * EPS * (st0[1][0] + longest) * np.linalg.norm(v1[2])
        assert np.all(np.isfinite(v1[2]))
        if delta not in S.CASES[name].literals_only:   # (there the iterates of an inconsistent system grow: x = A'y holds no bound)
            assert np.linalg.norm(v0[2] - v1[2]) <= bound, (delta, bound)


# ------------------------------------------------------------------------------------------------ (c) the history of a handle

def _other_inputs(name, key, lane):
    """Another call for the same handle (same options): the baseline's right-hand sides where the case has its own, else -- the case
    is its options -- right-hand sides that end the lanes at start-up or at iteration 1 (g on the empty columns, c on an empty
    row; LNLQ keeps its c: lnlq! divides by alpha_1, which is zero there); on the identity, g moved off the identity block."""
    vec = S.inputs(key)["vec"]
    ins = dict(S.case_inputs(name, key))
    if key == "ident":
        ins.update(g=vec["g"] + 0.5 * vec["r1"], c=vec["c"] + vec["half_m"], r1=vec["r1"] + vec["g"], r2=vec["r2"] + vec["half_m"])
    elif S.CASES[name].rhs:
        ins.update({k: vec[k] for k in ("g", "c", "r1", "r2")})
    else:
        ins.update(g=vec["gz"], c=vec["c" if lane == "lnlq" else "er"], r1=vec["gz"], r2=vec["er"])
    return ins


@pytest.mark.parametrize("name,key,lane", SMALL + MID, ids=[ids(c) for c in SMALL + MID])
def test_a_case_between_other_calls_is_bitwise_a_fresh_handle(name, key, lane):
    """One handle: another call, the case, the other call, the case twice, the other call.  The run-ahead of every call is the
    iteration count of the one before -- 18 before a lane that ends at 0, 0 before one that runs 18 -- and every call is bitwise
    what a fresh handle gives for the same arguments, statistics included."""
    ins = {"case": S.case_inputs(name, key), "other": _other_inputs(name, key, lane)}
    for delta in S.CASES[name].deltas:
        fresh = {"case": _default(name, key, lane, delta), "other": _fresh(name, key, lane, delta, ins=ins["other"])[0]}
        H = _Handle(S.inputs(key)["A"], delta=delta, **_options(name, lane))
        try:
            for step, which in enumerate(("other", "case", "other", "case", "case", "other")):
                _same_bits(_calls(H, lane, ins[which]), fresh[which], f"delta={delta:.3g} step {step} ({which})")
            assert H.counters() == (0, 0, 0)
        finally:
            H.close()


def _expects(calls):
    """Run-ahead counts before, at and behind the ends of the two lanes of every call: smaller, equal, one more, many more."""
    ends = {s[0] for c in calls for s in c[1]}
    return sorted({e for end in ends for e in (end - 1, end, end + 1, end + 9) if e >= 0} | {0, 1})


@pytest.mark.parametrize("name,key,lane", SMALL, ids=[ids(c) for c in SMALL])
def test_every_placement_of_the_run_ahead_is_bitwise_neutral(name, key, lane):
    """fpsq_debug_expect_iterations before each call: 0 (no speculation), 1, and around the end of either lane -- one less, equal,
    one more, nine more.  Bitwise the fresh handle's result every time."""
    ins = S.case_inputs(name, key)
    for delta in S.CASES[name].deltas:
        want = _default(name, key, lane, delta)
        H = _Handle(S.inputs(key)["A"], delta=delta, **_options(name, lane))
        try:
            for e in _expects(want):
                _same_bits(_calls(H, lane, ins, expect=e), want, f"delta={delta:.3g} expect {e}")
            assert H.counters() == (0, 0, 0)
        finally:
            H.close()


@pytest.mark.parametrize("name,key,kind,lane", QP_SMALL + QP_MID, ids=[ids(c) for c in QP_SMALL + QP_MID])
def test_qp_entries_with_their_speculative_epilogue_do_not_depend_on_the_history(name, key, kind, lane):
    """The qp entries enqueue their epilogue speculatively behind the expected count.  One model: an ordinary evaluation (a random
    point / direction), the case, the ordinary one, the case twice, the ordinary one; then the case with the run-ahead count
    placed around the ends of its lanes.  Every evaluation bitwise the one of a fresh model."""
    qp = _qp(name, key)
    opts = S.case_options(name, lane)
    rng = np.random.default_rng(5)
    arg = {"case": None, "other": rng.standard_normal(qp.n)}
    for delta in S.CASES[name].deltas:
        fresh = {}
        for which in ("case", "other"):
            dev = DeviceEqQP(qp, sigma=SIGMA, rho=RHO, delta=delta, **opts)
            fresh[which] = _qp_device(kind, dev, arg[which])
            dev.close()
        dev = DeviceEqQP(qp, sigma=SIGMA, rho=RHO, delta=delta, **opts)
        for step, which in enumerate(("other", "case", "other", "case", "case", "other")):
            _same_bits([_qp_device(kind, dev, arg[which])], [fresh[which]], f"delta={delta:.3g} step {step} ({which})")
        if key != "mid":
            for e in _expects([fresh["case"]]):
                _same_bits([_qp_device(kind, dev, None, expect=e)], [fresh["case"]], f"delta={delta:.3g} expect {e}")
        dev.close()
