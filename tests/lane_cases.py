"""The LNLQ and MINRES lanes on the Jacobians of tests/structures.py: inputs, the C restatement's results in its three
summation orders, the exact solves and the comparison rule shared by tests/test_lane_structures_cpu.py (which pins all of
it on the CPU) and tests/test_gpu_lane_structures.py (which holds the device to it).  Test infrastructure.

A lane's result is a list of CALLS, one per entry point of the C ABI the lane is driven through; a call is
(rc, [(niter, status, solved, rnorm, arnorm)] * 2, [output vectors])."""
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from abi_handle import _rel
from structures import random_structure

SE = float(np.sqrt(np.finfo(float).eps))
LANES = ["lnlq", "extras", "minres-k"]
DELTAS = [0.0, SE, 0.25]
CUTS = (1, 2, 3)
# the allowance of a fixed cut is max(TOL_FLOOR, SPREAD_FACTOR x the restatement's own spread over its summation orders) -- the
# rule of test_awkward_jacobian_structures_match_the_c_restatement -- and may never exceed these caps: a wider one fails the test
TOL_FLOOR, SPREAD_FACTOR, CAP_FIRST_CUT, CAP_ANY_CUT = 1e-12, 20.0, 1e-11, 1e-6
# stopping tests of the runs to the end: the tight sets of tests/test_gpu_parity.py (TIGHT; test_minres_on_k_method_parity), every
# conditioning limit off
TIGHT = dict(ls_atol=1e-15, ls_rtol=1e-15, ls_axtol=1e-15, ls_btol=1e-15, ls_etol=1e-15, ls_conlim=0.0,
             ln_atol=1e-15, ln_rtol=1e-15, ln_btol=1e-15, ln_conlim=0.0,
             ne_atol=1e-14, ne_rtol=1e-14, ne_etol=1e-16, ne_conlim=0.0)


@functools.lru_cache(maxsize=None)
def inputs(kind):
    """A, its CSR arrays as the restatement takes them, the right-hand sides g, r1 (n) and c, r2 (m), and a pair x (n), u (m)
    for the product checks (a generator of their own: the draws of the right-hand sides do not depend on them)."""
    rng = np.random.default_rng(12)
    A = random_structure(kind, rng)
    m, n = A.shape
    g, c = rng.standard_normal(n), rng.standard_normal(m)
    r1, r2 = rng.standard_normal(n), rng.standard_normal(m)
    rng2 = np.random.default_rng(13)
    x, u = rng2.standard_normal(n), rng2.standard_normal(m)
    return dict(A=A, m=m, n=n, csr=csr_arrays(A), g=g, c=c, r1=r1, r2=r2, x=x, u=u)


def csr_arrays(A):
    return A.indptr.astype(np.int64), A.indices.astype(np.int64), np.ascontiguousarray(A.data)


def cut_options(lane, k):
    """The options of a cut at k iterations, by the names both fpsq_options and the restatement's options use."""
    if lane == "lnlq":
        return dict(ln_method=1, ls_itmax=k, ln_itmax=k)
    if lane == "extras":
        return dict(ls_itmax=k, ne_itmax=k)
    return dict(ne_itmax=k)   # minres-k (the device handle adds kkt_method = 1)


def _stats(st, full=False):
    """full: `inconsistent` appended -- compare() holds whatever follows arnorm to equality (tests/stopping_cases.py)."""
    return (st.niter, st.status, st.solved, st.rnorm, st.arnorm) + ((st.inconsistent,) if full else ())


def restate(oracle, lane, ins, delta, opts, csr=None, full=False):
    """The lane's calls by the C restatement in its current summation order.  opts: cut_options(...) or TIGHT (+ ln_method);
    csr: another matrix of the same shape (the corrupted references of the CPU test).  lane "lnlq" is solve_two_mixed(g, c) with
    whatever least-norm method opts name ("mixed" is its other name), "lsq" is solve_two_least_squares(g, r1) on the LSQR
    lanes; full: the statistics carry `inconsistent` too."""
    m, n = ins["m"], ins["n"]
    rp, ci, va = csr or ins["csr"]
    if lane in ("lnlq", "mixed"):
        o = oracle.solve_two_mixed(m, n, rp, ci, va, delta, ins["g"], ins["c"], opts=oracle.default_options(n, m, **opts))
        return [(o[5], [_stats(s, full) for s in o[4]], list(o[:4]))]
    if lane == "lsq":
        o = oracle.solve_two_least_squares(m, n, rp, ci, va, delta, ins["g"], ins["r1"], opts=oracle.default_options(n, m, **opts))
        return [(o[5], [_stats(s, full) for s in o[4]], list(o[:4]))]
    if lane == "extras":
        o = oracle.solve_two_extras(m, n, rp, ci, va, delta, ins["r1"], ins["r2"], opts=oracle.default_options(n, m, **opts))
        return [(o[3], [_stats(s, full) for s in o[2]], list(o[:2]))]
    kw = dict(itmax=opts.get("ne_itmax", 0))
    for name in ("atol", "rtol", "etol", "conlim"):
        if "ne_" + name in opts:
            kw[name] = opts["ne_" + name]
    w = [oracle.minres_kkt(m, n, rp, ci, va, delta, **rhs, **kw) for rhs in (dict(bp=ins["g"]), dict(bq=ins["c"]), dict(bp=ins["r1"]))]
    calls = []
    for a, b in ((w[0], w[1]), (w[0], w[2])):   # solve_two_mixed(g, c), solve_two_least_squares(g, r1)
        rc = (0 if a[2].solved else 1) | (0 if b[2].solved else 2)   # (the rule of every two-system entry: fps_oracle.c)
        calls.append((rc, [_stats(a[2], full), _stats(b[2], full)], [a[0], a[1], b[0], b[1]]))
    return calls


@functools.lru_cache(maxsize=None)
def _cut_cached(oracle, lane, kind, delta, k, order):
    try:
        oracle.set_sum_order(order)
        return restate(oracle, lane, inputs(kind), delta, cut_options(lane, k))
    finally:
        oracle.set_sum_order(0)


def cut_reference(oracle, lane, kind, delta, k, order=0):
    """The restatement cut at k iterations, summed in `order` (0: left to right, the reference of every comparison)."""
    return _cut_cached(oracle, lane, kind, float(delta), k, order)


def vector_distance(got, want):
    """The largest relative inf-norm distance over the output vectors of all calls."""
    return max(_rel(a, b) for cg, cw in zip(got, want) for a, b in zip(cg[2], cw[2]))


def estimate_distance(got, want):
    """The largest distance of a residual estimate (rnorm, arnorm), relative to max(|want|, 1)."""
    return max(abs(sg[i] - sw[i]) / max(abs(sw[i]), 1.0) for cg, cw in zip(got, want) for sg, sw in zip(cg[1], cw[1]) for i in (3, 4))


def is_finite(calls):
    return all(np.all(np.isfinite(v)) for c in calls for v in c[2])


def spread_of(want, alts):
    """How far re-association alone moves the vectors of a result: the other summation orders against order 0.  (Python's max()
    passes a NaN over, hence the assertion: a run that broke down measures no rounding.)"""
    assert is_finite(want) and all(is_finite(alt) for alt in alts)
    return max(vector_distance(alt, want) for alt in alts)


def spread(oracle, lane, kind, delta, k):
    """spread_of() at this cut: orders 1 and 2 against order 0."""
    return spread_of(cut_reference(oracle, lane, kind, delta, k), [cut_reference(oracle, lane, kind, delta, k, order) for order in (1, 2)])


def allowance(spread_, k):
    tol = max(TOL_FLOOR, SPREAD_FACTOR * spread_)
    assert tol <= (CAP_FIRST_CUT if k == 1 else CAP_ANY_CUT), f"the restatement's own spread {spread_:.1e} at k = {k} asks for more than the cap"
    return tol


def compare(got, want, tol, what=""):
    """The assertion of the fixed cuts: equal return codes, equal (niter, status, solved) per lane -- and equal `inconsistent` where
    the statistics carry it behind arnorm (restate(full=True)) --, the residual estimates within tol * max(|want|, 1), every vector
    within tol in relative inf-norm.  All failures of a comparison are reported together."""
    bad = []
    assert len(got) == len(want)
    for ic, ((rc_g, st_g, v_g), (rc_w, st_w, v_w)) in enumerate(zip(got, want)):
        if rc_g != rc_w:
            bad.append(f"call {ic}: return code {rc_g} != {rc_w}")
        for i, (sg, sw) in enumerate(zip(st_g, st_w)):
            if tuple(sg[:3]) + tuple(sg[5:]) != tuple(sw[:3]) + tuple(sw[5:]):
                bad.append(f"call {ic} lane {i}: (niter, status, solved) {tuple(sg[:3]) + tuple(sg[5:])} != {tuple(sw[:3]) + tuple(sw[5:])}")
            for j, name in ((3, "rnorm"), (4, "arnorm")):
                if not abs(sg[j] - sw[j]) <= tol * max(abs(sw[j]), 1.0):
                    bad.append(f"call {ic} lane {i}: estimate {name} {sg[j]!r} != {sw[j]!r}")
        assert len(v_g) == len(v_w)
        for i, (a, b) in enumerate(zip(v_g, v_w)):
            if not _rel(a, b) < tol:
                bad.append(f"call {ic}: vector {i} differs by {_rel(a, b):.2e}")
    assert not bad, f"{what} (tol {tol:.1e}): " + "; ".join(bad)


# ------------------------------------------------------------------------------------------------ the runs to the end

DENSE_KKT_LIMIT = 7000   # n + m up to which the exact references are oracle.exact_* (the limit of tests/test_gpu_parity.py)


@functools.lru_cache(maxsize=None)
def _normal_solver(kind, shift):
    """b -> (A A' + shift I)^-1 b, factored once per kind: Cholesky of the dense matrix below 4000 rows (a dense column of A
    fills A A' anyway), SuperLU in a symmetric ordering beyond (the 10000-row kind: 1.7 s, against 6 s in the default one)."""
    A = sp.csr_matrix(inputs(kind)["A"])
    m = A.shape[0]
    S = A @ A.T + shift * sp.identity(m)
    if m <= 4000:
        import scipy.linalg as sl

        cf = sl.cho_factor(S.toarray())
        return lambda b: sl.cho_solve(cf, b)
    return spla.splu(sp.csc_matrix(S), permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True)).solve


def _kkt_by_elimination(kind, delta, b1, b2):
    """K [p; q] = [b1; b2], K = [I A'; A -delta I], through its Schur complement: (A A' + delta I) q = A b1 - b2, p = b1 - A' q.
    For the two kinds whose K (12000 and 22000 unknowns, one with a dense column) SuperLU takes minutes to factor."""
    A = sp.csr_matrix(inputs(kind)["A"])
    q = _normal_solver(kind, delta)(A @ b1 - b2)
    return b1 - A.T @ q, q


@functools.lru_cache(maxsize=None)
def _exact_kkt_pair(oracle, kind, delta, which):
    ins = inputs(kind)
    A, m, n = sp.csr_matrix(ins["A"]), ins["m"], ins["n"]
    if n + m <= DENSE_KKT_LIMIT:
        if which == "mixed":
            return list(oracle.exact_two_mixed(A, delta, ins["g"], ins["c"]))
        return list(oracle.exact_two_least_squares(A, delta, ins["g"], ins["r1"]))
    first = _kkt_by_elimination(kind, delta, ins["g"], np.zeros(m))
    second = _kkt_by_elimination(kind, delta, np.zeros(n), ins["c"]) if which == "mixed" else _kkt_by_elimination(kind, delta, ins["r1"], np.zeros(m))
    return [*first, *second]


@functools.lru_cache(maxsize=None)
def exact(oracle, lane, kind, delta):
    """The exact answers of the lane's calls, vectors only, in the order of restate()."""
    ins = inputs(kind)
    A, m, n = sp.csr_matrix(ins["A"]), ins["m"], ins["n"]
    if lane == "lnlq":   # LSQR: the first system of K; LNLQ: the minimum-norm solution of A x = -c, unregularised for every delta
        p1, q1 = _exact_kkt_pair(oracle, kind, delta, "mixed")[:2]
        ye = _normal_solver(kind, 0.0)(-ins["c"])
        return [[p1, q1, -(A.T @ ye), ye]]
    if lane == "extras":
        if n + m <= DENSE_KKT_LIMIT:
            return [list(oracle.exact_two_extras(A, delta, ins["r1"], ins["r2"]))]
        solve = _normal_solver(kind, max(delta, 1e-14))
        return [[solve(A @ ins["r1"]), solve(ins["r2"])]]
    return [_exact_kkt_pair(oracle, kind, delta, "mixed"), _exact_kkt_pair(oracle, kind, delta, "least_squares")]


def tight_options(lane):
    return {**TIGHT, "ln_method": 1} if lane == "lnlq" else dict(TIGHT)


@functools.lru_cache(maxsize=None)
def tight_reference(oracle, lane, kind, delta):
    return restate(oracle, lane, inputs(kind), delta, tight_options(lane))


def exact_distance(calls, ex):
    return max(_rel(a, b) for c, e in zip(calls, ex) for a, b in zip(c[2], e))
