"""Inputs built to reach every exit of the device Krylov lanes (csrc/fpsq_krylov.hip.h), the C restatement's results on them in its
three summation orders, and the literals both are pinned to: shared by tests/test_stopping_branches_cpu.py (no GPU) and
tests/test_gpu_stopping_branches.py.  Test infrastructure, in the manner of tests/lane_cases.py, whose restate(), spread_of(),
allowance() and compare() it uses.

MATRICES
  tiny   43 x 128: sp.random(40, 120, density 0.1, RandomState(1)) + 3 eye, then three EMPTY ROWS (40..42) and eight EMPTY COLUMNS
         (120..127).  A vector supported on the empty columns has A v = 0 exactly, one on the empty rows A'u = 0 exactly.
  ident  16 x 40: 2 [I 0].  With g = e_3 the first LSQR half-step gives beta = 0 exactly.
  mid    605 x 6007: problems.pde_control_like(n=6000, m=600, per_row=20, window=512, seed=17) -- the smallest shape at which the
         one-launch iteration is compared with the two-launch one --, five empty rows and seven empty columns appended: the
         products span several workgroups and the leaders of the one-launch iteration are not alone in the grid.
The right-hand sides are named vectors of inputs(); a case replaces some of g, c (solve_two_mixed), r1 (the second system of
solve_two_least_squares and the first of solve_two_extras), r2 (the second of solve_two_extras).

LANES (the keys of lane_cases.restate): "mixed" LSQR + CRAIG, "lnlq" LSQR + LNLQ (ln_method = 1), "lsq" LSQR + LSQR,
"extras" LSQR + MINRES on A A' + tau I, "minres-k" MINRES on K, both systems of solve_two_mixed and of solve_two_least_squares.

EVERY EXIT OF fpsq_krylov.hip.h, and the case that reaches it (status values: include/fpsq.h)
  lsqr_begin_step    beta1 == 0 -> ZERO_RHS (1), done                       zero-rhs-first, zero-rhs-second (lsq)
  lsqr_begin2_step   alpha == 0 -> ZERO_ATB (2), solved, arnorm 0          zero-atb-first, zero-atb-second
                     solved at iteration 0 by axtol -> ZERO_RESID (4),      startup-limits (the restatement and lsqr! rank
                       inconsistent 0 once 1 <= axtol                        zero_resid over solved here as in the loop)
                     solved_mach at iteration 0                              NOT REACHED: ArNorm / (Anorm rNorm) = 1 identically
                     tired at iteration 0 -> MAXITER                         NOT REACHED: itmax = 0 means "default", itmax < 0 is
                                                                             refused by the options check
  lsqr_sa_step       beta == 0 -> ctl.skip = 1, alpha and v kept             skip-half-step (ident)
  lsqr_sb_step       tired -> MAXITER (7)                                    itmax
                     ill_cond_lim -> ILL_COND (6), BELOW solved              ill-cond (not solved), ill-cond-and-solved (both: 3)
                     solved_lim / solved_opt -> SOLVED (3)                   baseline
                     zero_resid_lim -> ZERO_RESID (4), inconsistent 0        skip-half-step at delta = 0
                     fwd_err -> FWD_ERR (5), it >= 5                         fwd-err
                     ill_cond_mach, solved_mach, zero_resid_mach             NO CASE of their own: with the *_lim partner switched
                                                                             off (a limit of 0) a *_mach test fires alone only on
                                                                             an input whose test quantity lands in (0, eps] -- one
                                                                             converged to, or conditioned at, 1 / eps -- while an
                                                                             exact 0 (the identity) passes the *_lim test with
                                                                             limit 0 as well; the status assignment is the one
                                                                             their *_lim partners reach (here and in MINRES)
  craig_begin_step   beta1 == 0 -> ZERO_RHS                                  zero-rhs-second
                     1 <= btol | beta1 <= eps_c | beta1 <= btol -> SOLVED    startup-limits (btol), craig-startup-rtol (eps_c)
                     tired at iteration 0                                    NOT REACHED (as for LSQR)
  craig_sa_step      alpha == 0 -> INCONSISTENT (8), solved 0, upd_iter -1,  inconsistent (c on an empty row: A'c = 0)
                       x and y untouched
  craig_sb_step      tired -> MAXITER                                        itmax
                     solved -> SOLVED                                        baseline
                     ill_cond -> ILL_COND ABOVE solved                       ill-cond, craig-ill-cond-late (31 iterations at delta
                                                                             = 0, 8 at sqrt(eps); not solved), ill-cond-and-solved
                                                                             (both at iteration 1: status 6 with solved = 1)
  lnlq_begin_step    bNorm == 0 -> ZERO_RHS                                  zero-rhs-second (lnlq)
  lnlq_sa_step       tired -> MAXITER                                        itmax (lnlq)
                     solved_lq -> SOLVED_LQ (9)                              lnlq-lq-point
                     solved_cg -> SOLVED, above solved_lq                    baseline (lnlq), skip-half-step
                     alpha_1 == 0 (c on an empty row)                        NO CASE: lnlq! divides by alpha_1 (tau_1 = beta_1 /
                                                                             alpha_1): restatement and Krylov.jl give NaN
  lnlq_sb_step       no exit
  minres_begin_step  bb == 0 -> ZERO_RHS                                     zero-rhs-second (extras), zero-rhs-* (minres-k)
                     beta1 <= rtol -> solved at iteration 0:
                       ZERO_RESID (4), inconsistent 0 when beta1 <= eps_tol   minres-startup (rtol = 2: eps_tol = atol + 2 beta1)
                       = atol + rtol beta1 too (the restatement and minres!
                       rank zero_resid over solved);
                       SOLVED (3), inconsistent 1 otherwise                   minres-startup-solved (beta1 = 0.5 <= rtol = 0.7,
                                                                             eps_tol = atol + 0.35 < 0.5)
                     tired at iteration 0                                    NOT REACHED (as for LSQR)
  minres_a_step, minres_b_step   no exit
  minres_c_step      it == 1 and beta / beta1 <= 10 eps -> ZERO_ATB (2)      zero-atb-* (minres-k), inconsistent (extras, minres-k)
                     tired -> MAXITER                                        itmax
                     solved_lim / resid_decrease_lim -> SOLVED               baseline, minres-rtol
                     fwd_err -> FWD_ERR                                      minres-fwd-err
                     ill_cond -> ILL_COND                                    minres-ill-cond (gmax / gmin of the rotations stays
                                                                             below 3 on these matrices: ne_conlim = 1.02)
                     zero_resid_lim (test1 <= eps) -> ZERO_RESID             NOT REACHED through the options: needs a residual
                                                                             at machine precision before any other test fires
Every case's (niter, status, solved, inconsistent) per lane and return code are the literals of EXPECT, identical in the three
summation orders; the cases driven by a limit keep them when the limit moves by 1 % either way (Case.limits; a limit equal to the
quantity it is compared with -- axtol = 1 at start-up, rtol = 1 -- sat on the edge and is 2 here).
(craig_sa_step's `upd_iter = -1`: the update kernels of iteration `it` run for a lane that is done only when upd_iter == it, and
upd_iter still is -1 from craig_begin_step, or it - 1 from the iteration before, when alpha == 0 fires: no input tells the
assignment from its absence.  An exact alpha == 0 can be built at iteration 1 only.)"""
import collections
import functools

import numpy as np
import scipy.sparse as sp

import lane_cases as L

SE = L.SE
DELTAS = L.DELTAS
OFF = 0.0   # a tolerance of 0 never fires; a conlim of 0 switches the conditioning limit off


@functools.lru_cache(maxsize=None)
def matrix(key):
    if key == "tiny":
        A = sp.random(40, 120, density=0.1, random_state=np.random.RandomState(1)) + 3 * sp.eye(40, 120)
        return sp.csr_matrix((A.tocoo().data, (A.tocoo().row, A.tocoo().col)), shape=(43, 128))
    if key == "ident":
        return sp.csr_matrix(2.0 * sp.eye(16, 40))
    assert key == "mid"
    from fps_amd import problems

    A = problems.pde_control_like(n=6000, m=600, per_row=20, window=512, seed=17).scipy_csr().tocoo()
    return sp.csr_matrix((A.data, (A.row, A.col)), shape=(605, 6007))


def _unit(k, i, value=1.0):
    e = np.zeros(k)
    e[i] = value
    return e


@functools.lru_cache(maxsize=None)
def inputs(key):
    """The matrix, its CSR arrays as the restatement takes them, and the named right-hand sides."""
    A = matrix(key)
    m, n = A.shape
    v = dict(zero_n=np.zeros(n), zero_m=np.zeros(m), half_n=_unit(n, 0, 0.5), half_m=_unit(m, 0, 0.5))
    if key == "ident":
        v.update(g=_unit(n, 3), c=_unit(m, 5, 4.0), r1=_unit(n, 7), r2=_unit(m, 5, 4.0))
    else:
        rows, cols = A.shape[0] - np.count_nonzero(np.diff(A.indptr) == 0), int(A.indices.max()) + 1   # the non-empty part
        rng = np.random.default_rng(0)
        g, c = rng.standard_normal(n), rng.standard_normal(m)
        c[rows:] = 0.0
        r1, r2 = rng.standard_normal(n), rng.standard_normal(m)
        r2[rows:] = 0.0
        gz = np.zeros(n)
        gz[cols:] = rng.standard_normal(n - cols)      # on the empty columns only: A gz = 0 exactly
        ce = c.copy()
        ce[rows:] = rng.standard_normal(m - rows)      # a component on the empty rows: A x = -ce has no solution
        v.update(g=g, c=c, r1=r1, r2=r2, gz=gz, er=_unit(m, rows + 1), ce=ce)
        assert not (A @ gz).any() and not (A.T @ v["er"]).any()
    return dict(A=A, m=m, n=n, csr=L.csr_arrays(A), vec=v)


# matrices: where the case is run; lanes: the keys of lane_cases.restate it goes through; rhs: which named vector replaces g / c /
# r1 / r2; opts: option overrides; limits: the options that drive the branch (moved by 1 % in the CPU test); hits: (lane, call,
# system, status) the case is built for; zero: (lane, call, vector) that must be exactly zero (an ended lane that never updates);
# literals_only: deltas of the case at which return code and (niter, status, solved, inconsistent) are held, and bitwise equality
# between handles, but no distance to the restatement (its own summation orders are further apart than lane_cases.allowance caps)
Case = collections.namedtuple("Case", "matrices lanes rhs opts limits hits zero deltas literals_only",
                              defaults=({}, {}, (), (), (), tuple(DELTAS), ()))
BOTH = ("tiny", "mid")
ALL_LANES = ("mixed", "lnlq", "lsq", "extras", "minres-k")
LS_ONLY_ETOL = dict(ls_atol=OFF, ls_rtol=OFF, ls_axtol=OFF, ls_btol=OFF, ls_conlim=OFF, ls_etol=0.3)
NE_ONLY_ETOL = dict(ne_atol=OFF, ne_rtol=OFF, ne_conlim=OFF, ne_etol=0.3)

CASES = {
    "baseline": Case(BOTH, ALL_LANES, hits=(("mixed", 0, 0, 3), ("mixed", 0, 1, 3), ("lnlq", 0, 1, 3), ("extras", 0, 1, 3),
                                            ("minres-k", 0, 0, 3))),
    "zero-rhs-first": Case(BOTH, ("mixed", "lsq", "minres-k"), rhs=dict(g="zero_n"),
                           hits=(("mixed", 0, 0, 1), ("minres-k", 0, 0, 1)), zero=(("mixed", 0, 0), ("mixed", 0, 1), ("minres-k", 0, 0))),
    "zero-rhs-second": Case(BOTH, ALL_LANES, rhs=dict(c="zero_m", r1="zero_n", r2="zero_m"),
                            hits=(("mixed", 0, 1, 1), ("lnlq", 0, 1, 1), ("lsq", 0, 1, 1), ("extras", 0, 1, 1), ("minres-k", 0, 1, 1)),
                            zero=(("mixed", 0, 2), ("mixed", 0, 3), ("lnlq", 0, 2), ("lnlq", 0, 3), ("lsq", 0, 2), ("lsq", 0, 3),
                                  ("extras", 0, 1))),
    "zero-atb-first": Case(BOTH, ("mixed", "lsq", "minres-k"), rhs=dict(g="gz"),
                           hits=(("mixed", 0, 0, 2), ("lsq", 0, 0, 2), ("minres-k", 0, 0, 2)), zero=(("mixed", 0, 1), ("lsq", 0, 1))),
    "zero-atb-second": Case(BOTH, ("lsq", "extras", "minres-k"), rhs=dict(r1="gz"),
                            hits=(("lsq", 0, 1, 2), ("extras", 0, 0, 2), ("minres-k", 1, 1, 2)), zero=(("lsq", 0, 3), ("extras", 0, 0))),
    "inconsistent": Case(BOTH, ("mixed", "extras", "minres-k"), rhs=dict(c="er", r2="er"),
                         hits=(("mixed", 0, 1, 8), ("extras", 0, 1, 2), ("minres-k", 0, 1, 2)), zero=(("mixed", 0, 2), ("mixed", 0, 3))),
    # (at delta = 0 the lane ends as ILL_COND after 31 iterations of an inconsistent system whose iterates grow: the restatement's own
    # orders agree on the statistics and differ by 7e-3 in the vectors, beyond the caps of lane_cases.allowance -- literals only)
    "craig-ill-cond-late": Case(("tiny",), ("mixed",), rhs=dict(c="ce"), limits=("ln_conlim",), hits=(("mixed", 0, 1, 6),),
                                literals_only=(0.0,)),
    "fwd-err": Case(BOTH, ("mixed", "lsq"), opts=LS_ONLY_ETOL, limits=("ls_etol",), hits=(("mixed", 0, 0, 5), ("lsq", 0, 1, 5))),
    "ill-cond": Case(BOTH, ("mixed", "lsq"), opts=dict(ls_conlim=3.0, ln_conlim=3.0), limits=("ls_conlim", "ln_conlim"),
                     hits=(("mixed", 0, 0, 6), ("mixed", 0, 1, 6))),
    # (both lanes are solved AND ill-conditioned at iteration 1 -- without the rtol LSQR ends there as ILL_COND, the CPU test checks --:
    # the order of the status assignments decides, SOLVED for LSQR and ILL_COND for CRAIG)
    "ill-cond-and-solved": Case(BOTH, ("mixed", "lsq"), opts=dict(ls_conlim=1.01, ln_conlim=3.0, ls_rtol=0.9, ln_rtol=0.9),
                                limits=("ls_conlim", "ln_conlim", "ls_rtol", "ln_rtol"), hits=(("mixed", 0, 0, 3), ("mixed", 0, 1, 6))),
    "startup-limits": Case(BOTH, ("mixed", "lsq"), opts=dict(ls_axtol=2.0, ln_btol=2.0), limits=("ls_axtol", "ln_btol"),
                           hits=(("mixed", 0, 0, 4), ("mixed", 0, 1, 3)), zero=(("mixed", 0, 1), ("mixed", 0, 2), ("mixed", 0, 3))),
    "craig-startup-rtol": Case(BOTH, ("mixed",), opts=dict(ln_rtol=2.0), limits=("ln_rtol",), hits=(("mixed", 0, 1, 3),),
                               zero=(("mixed", 0, 2), ("mixed", 0, 3))),
    "itmax": Case(BOTH, ALL_LANES, opts=dict(ls_itmax=2, ln_itmax=2, ne_itmax=3),
                  hits=(("mixed", 0, 0, 7), ("mixed", 0, 1, 7), ("lnlq", 0, 1, 7), ("extras", 0, 1, 7), ("minres-k", 0, 0, 7))),
    # (at k = 1 rNorm_lq = |b| <= eps_l while rNorm_cg, measured in the M-norm, is 1 / sqrt(delta) times larger: the LQ point alone)
    "lnlq-lq-point": Case(BOTH, ("lnlq",), opts=dict(ln_rtol=2.0), limits=("ln_rtol",), hits=(("lnlq", 0, 1, 9),), deltas=(SE,)),
    "skip-half-step": Case(("ident",), ("mixed", "lnlq", "lsq"), hits=(("mixed", 0, 0, 4), ("lnlq", 0, 1, 3))),
    "minres-fwd-err": Case(BOTH, ("extras", "minres-k"), opts=NE_ONLY_ETOL, limits=("ne_etol",),
                           hits=(("extras", 0, 1, 5), ("minres-k", 0, 0, 5))),
    "minres-ill-cond": Case(BOTH, ("extras", "minres-k"), opts=dict(ne_conlim=1.02), limits=("ne_conlim",),
                            hits=(("extras", 0, 1, 6), ("minres-k", 0, 0, 6), ("minres-k", 0, 1, 6))),
    "minres-rtol": Case(BOTH, ("extras", "minres-k"), opts=dict(ne_rtol=1.0), limits=("ne_rtol",),
                        hits=(("extras", 0, 1, 3), ("minres-k", 0, 1, 3))),
    "minres-startup": Case(BOTH, ("extras", "minres-k"), rhs=dict(g="half_n", c="half_m", r1="half_n", r2="half_m"),
                           opts=dict(ne_rtol=2.0), limits=("ne_rtol",), hits=(("extras", 0, 1, 4), ("minres-k", 0, 0, 4)),
                           zero=(("extras", 0, 1), ("minres-k", 0, 0), ("minres-k", 0, 1), ("minres-k", 0, 2), ("minres-k", 0, 3))),
    # (solved at start-up WITHOUT zero_resid: beta1 = 0.5 <= rtol, but atol + rtol beta1 = 1.5e-8 + 0.35 < beta1)
    "minres-startup-solved": Case(BOTH, ("extras", "minres-k"), rhs=dict(g="half_n", c="half_m", r1="half_n", r2="half_m"),
                                  opts=dict(ne_rtol=0.7), limits=("ne_rtol",), hits=(("extras", 0, 1, 3), ("minres-k", 0, 0, 3)),
                                  zero=(("extras", 0, 1), ("minres-k", 0, 0), ("minres-k", 0, 1), ("minres-k", 0, 2), ("minres-k", 0, 3))),
}


def held_deltas(name):
    """The deltas of the case at which the device is held to the restatement's vectors and estimates (all but literals_only)."""
    return tuple(d for d in CASES[name].deltas if d not in CASES[name].literals_only)


def case_inputs(name, key):
    """The `ins` of lane_cases.restate for this case on this matrix."""
    ins = inputs(key)
    rhs = {k: ins["vec"][CASES[name].rhs.get(k, k)] for k in ("g", "c", "r1", "r2")}
    return dict(m=ins["m"], n=ins["n"], csr=ins["csr"], A=ins["A"], **rhs)


def case_options(name, lane):
    """The option overrides of the case on this lane, by the names fpsq_options and the restatement share (the device handle
    of "minres-k" adds kkt_method = 1)."""
    opts = dict(CASES[name].opts)
    if lane == "lnlq":
        opts["ln_method"] = 1
    return opts


def reference(oracle, name, key, lane, delta, order=0, scale=None):
    """The case's calls (lane_cases.restate, statistics with `inconsistent`) by the restatement summed in `order`.  scale: (option,
    factor), the limit moved."""
    return _reference(oracle, name, key, lane, float(delta), order, scale)


@functools.lru_cache(maxsize=None)
def _reference(oracle, name, key, lane, delta, order, scale):
    ins = case_inputs(name, key)
    opts = case_options(name, lane)
    if scale is not None:   # (a limit the case leaves at its default is moved from the default)
        opts[scale[0]] = opts.get(scale[0], getattr(oracle.default_options(ins["n"], ins["m"]), scale[0])) * scale[1]
    try:
        oracle.set_sum_order(order)
        return L.restate(oracle, lane, ins, delta, opts, full=True)
    finally:
        oracle.set_sum_order(0)


def literals(calls):
    """[(rc, (niter, status, solved, inconsistent) of system 0, ... of system 1)] per call: the form of EXPECT."""
    return [(c[0], *[(s[0], s[1], s[2], s[5]) for s in c[1]]) for c in calls]


def spread(oracle, name, key, lane, delta):
    """How far re-association alone moves the case's results: the vectors (lane_cases.spread_of) and the residual estimates, which
    compare() holds to the same allowance (CRAIG's rnorm = beta |xi| |c1| moves by more than its vectors at delta = sqrt(eps))."""
    want = reference(oracle, name, key, lane, delta)
    alts = [reference(oracle, name, key, lane, delta, order) for order in (1, 2)]
    return max(L.spread_of(want, alts), max(L.estimate_distance(alt, want) for alt in alts))


def allowance(oracle, name, key, lane, delta):
    """lane_cases.allowance of the restatement's own spread at this case, under its caps: the cap of the first cut where no lane
    of the case goes beyond one iteration, the cap of every cut otherwise."""
    k = max(s[0] for c in reference(oracle, name, key, lane, delta) for s in c[1])
    return L.allowance(spread(oracle, name, key, lane, delta), max(k, 1))


def exactly_zero_where_the_reference_is(got, want):
    """A lane that ended before its first update leaves its vectors at zero: where a vector of the reference is all zero the
    same vector of `got` is, and every vector of `got` is finite (the device's outputs are preset to NaN)."""
    return L.is_finite(got) and all(not a.any() for cg, cw in zip(got, want) for a, b in zip(cg[2], cw[2]) if not b.any())


def combos(keys=None):
    """(case, matrix, lane) of the whole table, or of the given matrices."""
    return [(name, key, lane) for name, case in CASES.items() for key in case.matrices if keys is None or key in keys
            for lane in case.lanes]


def expected(name, key, lane, delta):
    """The literals of this (case, matrix, lane) at delta: one entry for every delta of the case, or one per delta."""
    e = EXPECT[f"{name}/{key}/{lane}"]
    return e[0] if len(e) == 1 else e[CASES[name].deltas.index(delta)]


# (niter, status, solved, inconsistent) per system behind the return code, per call, per delta (one entry: the same for every delta
# of the case); written down from the restatement, held by tests/test_stopping_branches_cpu.py
EXPECT = {
    "baseline/tiny/mixed": [[(0, (18, 3, 1, 1), (18, 3, 1, 0))]],
    "baseline/tiny/lnlq": [[(0, (18, 3, 1, 1), (20, 3, 1, 0))], [(0, (18, 3, 1, 1), (28, 3, 1, 0))], [(0, (18, 3, 1, 1), (21, 3, 1, 0))]],
    "baseline/tiny/lsq": [[(0, (18, 3, 1, 1), (18, 3, 1, 1))]],
    "baseline/tiny/extras": [[(0, (18, 3, 1, 1), (20, 3, 1, 1))], [(0, (18, 3, 1, 1), (20, 3, 1, 1))], [(0, (18, 3, 1, 1), (19, 3, 1, 1))]],
    "baseline/tiny/minres-k": [[(0, (41, 3, 1, 1), (38, 3, 1, 1)), (0, (41, 3, 1, 1), (41, 3, 1, 1))]],
    "baseline/mid/mixed": [[(0, (14, 3, 1, 1), (15, 3, 1, 0))]],
    "baseline/mid/lnlq": [[(0, (14, 3, 1, 1), (18, 3, 1, 0))], [(0, (14, 3, 1, 1), (26, 3, 1, 0))], [(0, (14, 3, 1, 1), (18, 3, 1, 0))]],
    "baseline/mid/lsq": [[(0, (14, 3, 1, 1), (14, 3, 1, 1))]],
    "baseline/mid/extras": [[(0, (14, 3, 1, 1), (17, 3, 1, 1))], [(0, (14, 3, 1, 1), (17, 3, 1, 1))], [(0, (14, 3, 1, 1), (16, 3, 1, 1))]],
    "baseline/mid/minres-k": [[(0, (35, 3, 1, 1), (34, 3, 1, 1)), (0, (35, 3, 1, 1), (35, 3, 1, 1))]],
    "zero-rhs-first/tiny/mixed": [[(0, (0, 1, 1, 0), (18, 3, 1, 0))]],
    "zero-rhs-first/tiny/lsq": [[(0, (0, 1, 1, 0), (18, 3, 1, 1))]],
    "zero-rhs-first/tiny/minres-k": [[(0, (0, 1, 1, 0), (38, 3, 1, 1)), (0, (0, 1, 1, 0), (41, 3, 1, 1))]],
    "zero-rhs-first/mid/mixed": [[(0, (0, 1, 1, 0), (15, 3, 1, 0))]],
    "zero-rhs-first/mid/lsq": [[(0, (0, 1, 1, 0), (14, 3, 1, 1))]],
    "zero-rhs-first/mid/minres-k": [[(0, (0, 1, 1, 0), (34, 3, 1, 1)), (0, (0, 1, 1, 0), (35, 3, 1, 1))]],
    "zero-rhs-second/tiny/mixed": [[(0, (18, 3, 1, 1), (0, 1, 1, 0))]],
    "zero-rhs-second/tiny/lnlq": [[(0, (18, 3, 1, 1), (0, 1, 1, 0))]],
    "zero-rhs-second/tiny/lsq": [[(0, (18, 3, 1, 1), (0, 1, 1, 0))]],
    "zero-rhs-second/tiny/extras": [[(0, (0, 1, 1, 0), (0, 1, 1, 0))]],
    "zero-rhs-second/tiny/minres-k": [[(0, (41, 3, 1, 1), (0, 1, 1, 0)), (0, (41, 3, 1, 1), (0, 1, 1, 0))]],
    "zero-rhs-second/mid/mixed": [[(0, (14, 3, 1, 1), (0, 1, 1, 0))]],
    "zero-rhs-second/mid/lnlq": [[(0, (14, 3, 1, 1), (0, 1, 1, 0))]],
    "zero-rhs-second/mid/lsq": [[(0, (14, 3, 1, 1), (0, 1, 1, 0))]],
    "zero-rhs-second/mid/extras": [[(0, (0, 1, 1, 0), (0, 1, 1, 0))]],
    "zero-rhs-second/mid/minres-k": [[(0, (35, 3, 1, 1), (0, 1, 1, 0)), (0, (35, 3, 1, 1), (0, 1, 1, 0))]],
    "zero-atb-first/tiny/mixed": [[(0, (0, 2, 1, 0), (18, 3, 1, 0))]],
    "zero-atb-first/tiny/lsq": [[(0, (0, 2, 1, 0), (18, 3, 1, 1))]],
    "zero-atb-first/tiny/minres-k": [[(0, (1, 2, 1, 1), (38, 3, 1, 1)), (0, (1, 2, 1, 1), (41, 3, 1, 1))]],
    "zero-atb-first/mid/mixed": [[(0, (0, 2, 1, 0), (15, 3, 1, 0))]],
    "zero-atb-first/mid/lsq": [[(0, (0, 2, 1, 0), (14, 3, 1, 1))]],
    "zero-atb-first/mid/minres-k": [[(0, (1, 2, 1, 1), (34, 3, 1, 1)), (0, (1, 2, 1, 1), (35, 3, 1, 1))]],
    "zero-atb-second/tiny/lsq": [[(0, (18, 3, 1, 1), (0, 2, 1, 0))]],
    "zero-atb-second/tiny/extras": [[(0, (0, 2, 1, 0), (20, 3, 1, 1))], [(0, (0, 2, 1, 0), (20, 3, 1, 1))], [(0, (0, 2, 1, 0), (19, 3, 1, 1))]],
    "zero-atb-second/tiny/minres-k": [[(0, (41, 3, 1, 1), (38, 3, 1, 1)), (0, (41, 3, 1, 1), (1, 2, 1, 1))]],
    "zero-atb-second/mid/lsq": [[(0, (14, 3, 1, 1), (0, 2, 1, 0))]],
    "zero-atb-second/mid/extras": [[(0, (0, 2, 1, 0), (17, 3, 1, 1))], [(0, (0, 2, 1, 0), (17, 3, 1, 1))], [(0, (0, 2, 1, 0), (16, 3, 1, 1))]],
    "zero-atb-second/mid/minres-k": [[(0, (35, 3, 1, 1), (34, 3, 1, 1)), (0, (35, 3, 1, 1), (1, 2, 1, 1))]],
    "inconsistent/tiny/mixed": [[(2, (18, 3, 1, 1), (0, 8, 0, 1))]],
    "inconsistent/tiny/extras": [[(0, (18, 3, 1, 1), (1, 2, 1, 1))]],
    "inconsistent/tiny/minres-k": [[(0, (41, 3, 1, 1), (1, 2, 1, 1)), (0, (41, 3, 1, 1), (41, 3, 1, 1))]],
    "inconsistent/mid/mixed": [[(2, (14, 3, 1, 1), (0, 8, 0, 1))]],
    "inconsistent/mid/extras": [[(0, (14, 3, 1, 1), (1, 2, 1, 1))]],
    "inconsistent/mid/minres-k": [[(0, (35, 3, 1, 1), (1, 2, 1, 1)), (0, (35, 3, 1, 1), (35, 3, 1, 1))]],
    "craig-ill-cond-late/tiny/mixed": [[(2, (18, 3, 1, 1), (31, 6, 0, 0))], [(2, (18, 3, 1, 1), (8, 6, 0, 0))], [(0, (18, 3, 1, 1), (21, 3, 1, 0))]],
    "fwd-err/tiny/mixed": [[(0, (7, 5, 1, 1), (18, 3, 1, 0))]],
    "fwd-err/tiny/lsq": [[(0, (7, 5, 1, 1), (7, 5, 1, 1))]],
    "fwd-err/mid/mixed": [[(0, (6, 5, 1, 1), (15, 3, 1, 0))]],
    "fwd-err/mid/lsq": [[(0, (6, 5, 1, 1), (6, 5, 1, 1))]],
    "ill-cond/tiny/mixed": [[(3, (3, 6, 0, 1), (1, 6, 0, 0))]],
    "ill-cond/tiny/lsq": [[(3, (3, 6, 0, 1), (3, 6, 0, 1))]],
    "ill-cond/mid/mixed": [[(3, (3, 6, 0, 1), (1, 6, 0, 0))]],
    "ill-cond/mid/lsq": [[(3, (3, 6, 0, 1), (3, 6, 0, 1))]],
    "ill-cond-and-solved/tiny/mixed": [[(0, (1, 3, 1, 1), (1, 6, 1, 0))]],
    "ill-cond-and-solved/tiny/lsq": [[(0, (1, 3, 1, 1), (1, 3, 1, 1))]],
    "ill-cond-and-solved/mid/mixed": [[(0, (1, 3, 1, 1), (1, 6, 1, 0))]],
    "ill-cond-and-solved/mid/lsq": [[(0, (1, 3, 1, 1), (1, 3, 1, 1))]],
    "startup-limits/tiny/mixed": [[(0, (0, 4, 1, 0), (0, 3, 1, 0))]],
    "startup-limits/tiny/lsq": [[(0, (0, 4, 1, 0), (0, 4, 1, 0))]],
    "startup-limits/mid/mixed": [[(0, (0, 4, 1, 0), (0, 3, 1, 0))]],
    "startup-limits/mid/lsq": [[(0, (0, 4, 1, 0), (0, 4, 1, 0))]],
    "craig-startup-rtol/tiny/mixed": [[(0, (18, 3, 1, 1), (0, 3, 1, 0))]],
    "craig-startup-rtol/mid/mixed": [[(0, (14, 3, 1, 1), (0, 3, 1, 0))]],
    "itmax/tiny/mixed": [[(3, (2, 7, 0, 1), (2, 7, 0, 0))]],
    "itmax/tiny/lnlq": [[(3, (2, 7, 0, 1), (3, 7, 0, 0))]],
    "itmax/tiny/lsq": [[(3, (2, 7, 0, 1), (2, 7, 0, 1))]],
    "itmax/tiny/extras": [[(3, (2, 7, 0, 1), (3, 7, 0, 1))]],
    "itmax/tiny/minres-k": [[(3, (3, 7, 0, 1), (3, 7, 0, 1)), (3, (3, 7, 0, 1), (3, 7, 0, 1))]],
    "itmax/mid/mixed": [[(3, (2, 7, 0, 1), (2, 7, 0, 0))]],
    "itmax/mid/lnlq": [[(3, (2, 7, 0, 1), (3, 7, 0, 0))]],
    "itmax/mid/lsq": [[(3, (2, 7, 0, 1), (2, 7, 0, 1))]],
    "itmax/mid/extras": [[(3, (2, 7, 0, 1), (3, 7, 0, 1))]],
    "itmax/mid/minres-k": [[(3, (3, 7, 0, 1), (3, 7, 0, 1)), (3, (3, 7, 0, 1), (3, 7, 0, 1))]],
    "lnlq-lq-point/tiny/lnlq": [[(0, (18, 3, 1, 1), (2, 9, 1, 0))]],
    "lnlq-lq-point/mid/lnlq": [[(0, (14, 3, 1, 1), (2, 9, 1, 0))]],
    "skip-half-step/ident/mixed": [[(0, (1, 4, 1, 0), (1, 3, 1, 0))], [(0, (1, 3, 1, 1), (1, 3, 1, 0))], [(0, (1, 3, 1, 1), (1, 3, 1, 0))]],
    "skip-half-step/ident/lnlq": [[(0, (1, 4, 1, 0), (2, 3, 1, 0))], [(0, (1, 3, 1, 1), (2, 3, 1, 0))], [(0, (1, 3, 1, 1), (2, 3, 1, 0))]],
    "skip-half-step/ident/lsq": [[(0, (1, 4, 1, 0), (1, 4, 1, 0))], [(0, (1, 3, 1, 1), (1, 3, 1, 1))], [(0, (1, 3, 1, 1), (1, 3, 1, 1))]],
    "minres-fwd-err/tiny/extras": [[(0, (18, 3, 1, 1), (7, 5, 1, 1))]],
    "minres-fwd-err/tiny/minres-k": [[(0, (12, 5, 1, 1), (9, 5, 1, 1)), (0, (12, 5, 1, 1), (12, 5, 1, 1))]],
    "minres-fwd-err/mid/extras": [[(0, (14, 3, 1, 1), (6, 5, 1, 1))]],
    "minres-fwd-err/mid/minres-k": [[(0, (10, 5, 1, 1), (7, 5, 1, 1)), (0, (10, 5, 1, 1), (10, 5, 1, 1))]],
    "minres-ill-cond/tiny/extras": [[(2, (18, 3, 1, 1), (2, 6, 0, 1))]],
    "minres-ill-cond/tiny/minres-k": [[(3, (2, 6, 0, 1), (2, 6, 0, 1)), (3, (2, 6, 0, 1), (2, 6, 0, 1))]],
    "minres-ill-cond/mid/extras": [[(2, (14, 3, 1, 1), (2, 6, 0, 1))]],
    "minres-ill-cond/mid/minres-k": [[(3, (2, 6, 0, 1), (2, 6, 0, 1)), (3, (2, 6, 0, 1), (2, 6, 0, 1))]],
    "minres-rtol/tiny/extras": [[(0, (18, 3, 1, 1), (1, 3, 1, 1))]],
    "minres-rtol/tiny/minres-k": [[(0, (1, 3, 1, 1), (1, 3, 1, 1)), (0, (1, 3, 1, 1), (1, 3, 1, 1))]],
    "minres-rtol/mid/extras": [[(0, (14, 3, 1, 1), (1, 3, 1, 1))]],
    "minres-rtol/mid/minres-k": [[(0, (1, 3, 1, 1), (1, 3, 1, 1)), (0, (1, 3, 1, 1), (1, 3, 1, 1))]],
    "minres-startup/tiny/extras": [[(0, (19, 3, 1, 1), (0, 4, 1, 0))], [(0, (19, 3, 1, 1), (0, 4, 1, 0))], [(0, (18, 3, 1, 1), (0, 4, 1, 0))]],
    "minres-startup/tiny/minres-k": [[(0, (0, 4, 1, 0), (0, 4, 1, 0)), (0, (0, 4, 1, 0), (0, 4, 1, 0))]],
    "minres-startup/mid/extras": [[(0, (14, 3, 1, 1), (0, 4, 1, 0))]],
    "minres-startup/mid/minres-k": [[(0, (0, 4, 1, 0), (0, 4, 1, 0)), (0, (0, 4, 1, 0), (0, 4, 1, 0))]],
    "minres-startup-solved/tiny/extras": [[(0, (19, 3, 1, 1), (0, 3, 1, 1))], [(0, (19, 3, 1, 1), (0, 3, 1, 1))], [(0, (18, 3, 1, 1), (0, 3, 1, 1))]],
    "minres-startup-solved/tiny/minres-k": [[(0, (0, 3, 1, 1), (0, 3, 1, 1)), (0, (0, 3, 1, 1), (0, 3, 1, 1))]],
    "minres-startup-solved/mid/extras": [[(0, (14, 3, 1, 1), (0, 3, 1, 1))]],
    "minres-startup-solved/mid/minres-k": [[(0, (0, 3, 1, 1), (0, 3, 1, 1)), (0, (0, 3, 1, 1), (0, 3, 1, 1))]],
}
