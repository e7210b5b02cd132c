"""Shapes built to run the CSR row-product kernels of the banded direct back-end (k_bq_*, k_bqb_*, k_bn_* in
csrc/fpsq_band.hip.h and csrc/fpsq_band_nlp.hip.h) at every lane-group width and through the second trip of their grid-stride
loops, the yardsticks they are held to, and the literals both are pinned to: shared by tests/test_lane_groups_cpu.py (no GPU)
and tests/test_gpu_lane_groups.py.  Test infrastructure, in the manner of tests/stopping_cases.py.

LANES.  A kernel gives LG lanes to a row; lane_group(nnz, rows) (csrc/fpsq_lanegroup.h, restated below) picks LG = the largest
power of two <= nnz // rows, and WITH_LANE_GROUP instantiates 1, 2, 4, 8, 16, 32, 64.  A model evaluates it three times:
lgA = lane_group(nnz, m) for the rows of A, lgT = lane_group(nnz, n) for the rows of A', lgR = lane_group(nnz(R), n) for the
off-diagonal part R of a sparse objective Hessian.  A tile is 256 // LG rows; a grid is capped at 2048 workgroups (4096 for
k_bn_vals and k_gather_d, 256 entries each), above which a workgroup walks a second tile.

CASES (ragged_band: pde_control_like's rule with a row length per row)
  case        n     m     rows of A                     window  nnz      lgA lgT  cond(A)  there for
  wide-rows   1536  96    160                           512     15360    64  8    1.7      rows of 2.5 LG at LG = 64; m < 128; columns of 1 entry
  m-near-n    1100  1000  40                            128     40000    32  32   22       A' at 32; the base of the lgR cases
  both-64     600   500   80                            160     40000    64  64   18       A' at 64; n, mpad multiples of the tile, m < mpad
  lgT-16      1000  500   40                            160     20000    32  16   4.7      A' at 16
  lgT-8       1400  330   30, 41, 52                    192     13530    32  8    2.7      A' at 8; no row a multiple of LG
  thin        900   700   1, 1, 2, 1, 1, 3, 1           64      1000     1   1    2.0      one lane on both sides; 146 empty columns
  lg2         900   300   2, 3, 2, 1, 5, 2              64      750      2   1    1.9      A at 2, a row shorter than LG; 361 empty columns
  ragged      1300  1000  1, 97, 33, 200, 7, 64, 65, 13 256     60000    32  32   13       rows of 1 .. 6 LG + 8 entries under one LG
  stride      9000  8300  128                           256     1062400  64  64   --       2250 / 2080 tiles against 2048; nnz > 4096 x 256;
                                                                                           two elimination chains (rperm is live)
  lg4-2       1200  600   4, 5, 6, 3                    64      2700     4   2    2.5      the widths 4 / 2, a row shorter than LG
  lg8-4       3600  1500  12                            256     18000    8   4    3.0      the widths 8 / 4
  lg16-2      2000  250   17, 23                        128     5000     16  2    2.2      the width 16 on the A side
  both-64-shuffled, ragged-shuffled: the rows of both-64 / ragged in a random order; the symbolic phase reorders them
  (reordered == 1), so rperm / vperm / t_perm are live at 64 / 64 and 32 / 32 lanes.
(both-64 has window 160, not 200: with 200 the reverse Cuthill-McKee pass cannot bring the shuffled rows under three blocks of
bandwidth and the handle keeps the caller's order.  cond(A) by dense SVD; the nonlinear model's sigma_min(J(x)) is printed by
tests/test_lane_groups_cpu.py.)
SPARSE HESSIANS (problems.with_sparse_hessian): on m-near-n the half-widths 1, 2, 3, 6, 12, 23, 45 -- the smallest that reach
lgR = 1, 2, 4, 8, 16, 32, 64 (64 is reached at n = 1100) --, and half-width 2 on thin, lg2, lg4-2, lg8-4, lg16-2, lgT-8, lgT-16,
both-64, so that the kernels that take the Hessian as a template flag run at every width of lgA and lgT too.

EVERY WITH_LANE_GROUP SITE OF THE BAND UNIT, the lanes it dispatches on, and the case that reaches each width.
By width -- lgA: 1 thin, 2 lg2, 4 lg4-2, 8 lg8-4, 16 lg16-2, 32 m-near-n / lgT-16 / lgT-8 / ragged(-shuffled), 64 wide-rows /
both-64(-shuffled) / stride;  lgT: 1 thin / lg2, 2 lg4-2 / lg16-2, 4 lg8-4, 8 wide-rows / lgT-8, 16 lgT-16, 32 m-near-n /
ragged(-shuffled), 64 both-64(-shuffled) / stride;  lgR: m-near-n with the half-width of that width.  "all" = each of these;
"hess" = the cases of HESS_CASES, which cover every width of that side; second trip of the grid-stride loop: stride.
  fpsq_band.hip, single-vector entries (bq_launches, fpsq_band_jac_mul)
    k_bq_pack_sq          lgR  objgrad, hprod with a sparse Hessian                 all (m-near-n)
    k_bq_prologue         lgA  objgrad, hprod; nlp hprod Val(2), Val(1)             all; stride (partials of a capped grid)
                               (its FPSQ_BAND_QP_G form is a developer switch and is not run)
    k_bq_epilogue         lgT  objgrad, hprod; nlp hprod Val(2)                     all; stride
    k_bq_epilogue_sq      lgT  objgrad, hprod with a sparse Hessian                 hess
    k_bq_jacmul           lgR  out -= R tv behind k_bq_epilogue_sq                  all (m-near-n)
                          lgA  jac_mul, trans = 0 (rows = m, not mpad)              all; stride
                          lgT  jac_mul, trans = 1                                   all; stride
                          lg   jac_mul, trans = 1 on a handle with long columns     out of scope (test_gpu_band_long_columns.py)
  fpsq_band.hip, block entries
    k_bqb_prologue        lgA  hprod_block, solve_two_least_squares_block           all; stride
                          lgA  border_factor, bordered handles only                 out of scope (tests/test_gpu_band_border.py)
    k_bqb_epilogue        lgT  hprod_block (MODE 0; 1 with a sparse Hessian: hess); all; stride
                               solve_two_least_squares_block (MODE 2)
    k_bqb_pack_sq         lgR  hprod_block with a sparse Hessian                    all (m-near-n)
    k_bqb_rsub            lgR  hprod_block, objgrad_block with a sparse Hessian     all (m-near-n)
    k_bqb_og_pack_sq      lgR  objgrad_block with a sparse Hessian                  all (m-near-n)
    k_bqb_og_prologue     lgA  objgrad_block (FD; without FD: hess)                 all; stride
    k_bqb_og_epilogue     lgT  objgrad_block (with SQ: hess)                        all; stride
  fpsq_band_nlp.hip.h
    k_bn_cons             lgA  cons (rows = m)                                      all; stride
    k_bn_tvals            lgT  objgrad: J(x)' into the transposed values            all; stride
    k_bn_prologue         lgA  objgrad                                              all; stride
    k_bn_epilogue         lgT  objgrad                                              all; stride
    k_bn_epilogue_h1      lgT  hprod Val(1)                                         all; stride
    k_bn_hgv              lgA  hprod Val(1)                                         all; stride
    k_bn_jtz              lgT  hprod Val(1)                                         all; stride
  fpsq_band_nlp.hip.h, the model with function terms: three of the dispatches above launch a function form from their `else`
  branch; the other sites are shared as they are.  "fn" = part 1 of tests/test_gpu_band_fn_nlp.py, which runs every case of
  this table (all seven widths on each side) and stride (the second trip).
    k_bn_cons_fn                    lgA  cons (rows = m)                            fn: all; stride
    k_bn_tvals_fn                   lgT  objgrad: J(x)' and G(x)' per row           fn: all; stride
    k_bn_prologue<LG, false, true>  lgA  objgrad (the FN form)                      fn: all; stride
  fpsq_band_nlp.hip.h, the model with coupling terms.  The five kernels with the flag CP are the rows above instantiated as
  k_bn_*<LG, true> (the rows above are <LG, false>); k_bn_jtz and the Val(1) k_bq_prologue site are shared as they are; k_bn_tvals
  is not run (k_bcn_vals, per entry, twice).  "coupled" = the cases of tests/coupled_cases.py, which reach
  lgA 2, 4, 16, 32; lgT 1, 2, 32; lgR 1, 8 and no other width (tests/test_lane_groups_cpu.py recomputes the three sets); second
  trip of the grid-stride loop: coupled_cases.py STRIDE at 2 / 1 / 1.  "lanes" = the cases of tests/coupled_lane_cases.py (a
  denser term rule on the shapes of this table), which reach every width of lgA, of lgT and of lgR
  (tests/test_coupled_lane_groups_cpu.py recomputes the three sets; tests/test_gpu_coupled_lane_groups.py runs them).
    k_bn_cons<LG, true>         lgA  cons (rows = m)                                coupled; STRIDE; lanes: all
    k_bn_prologue<LG, true>     lgA  objgrad                                        coupled; STRIDE; lanes: all
    k_bn_epilogue<LG, true>     lgT  objgrad                                        coupled; STRIDE; lanes: all
    k_bcn_finish                lgR  objgrad with gx: the rows of S                 coupled; STRIDE; lanes: all
    k_bcn_hcv                   lgR  hprod Val(2), rho > 0                          coupled; STRIDE; lanes: all
    k_bq_pack_sq                lgR  hprod Val(1) (<LG, true>; Val(2): bq_launches) coupled; STRIDE; lanes: all
    k_bn_epilogue_h1<LG, true>  lgT  hprod Val(1)                                   coupled; STRIDE; lanes: all
    k_bcn_finish_h1             lgR  hprod Val(1): the rows of S                    coupled; STRIDE; lanes: all
    k_bn_hgv<LG, true>          lgA  hprod Val(1)                                   coupled; STRIDE; lanes: all
  not under WITH_LANE_GROUP but capped (one helper, flat_grid): k_bn_vals (objgrad) and the k_gather_d launches of
  fpsq_band_nlp_create (the handle of stride is reordered into two chains, so both gathers run): 4150 blocks of entries against
  4096 on stride; with coupling terms k_bcn_vals (4219 blocks on STRIDE) and k_bcn_assemble (2813 on STRIDE; 6501 on the case
  assemble-stride of tests/coupled_lane_cases.py, which takes it through its second trip).

YARDSTICKS.  exact_linear: tests/sparse_hessian_ref.py (one LU of K = [I A'; A -delta I], kept), which on a diagonal Hessian
evaluates the formulae of oracle.exact_qp_objgrad / exact_qp_hprod.  exact_nonlinear: tests/sepquad_ref.py with its three
solves on kept factors (_KeptFactorOracle): SepQuadRef factorises K again for every call, three seconds each on stride."""
import copy
import dataclasses
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from fps_amd import problems
from oracle_qdsolver import OracleQDSolver
from sepquad_ref import SepQuadRef
from sparse_hessian_ref import SparseHessianRef

SE = float(np.sqrt(np.finfo(float).eps))
SIGMA, CURV = 1e3, 0.3
WIDTHS = (1, 2, 4, 8, 16, 32, 64)
MAX_GRID = 2048        # kBqMaxGrid of csrc/fpsq_band.hip: workgroups of a product kernel
MAX_GRID_FLAT = 4096   # flat_grid of csrc/fpsq_band_nlp.hip.h: the per-entry launches of the nonlinear model (256 entries a workgroup)


def lane_group(nnz, rows):
    """csrc/fpsq_lanegroup.h lane_group: the largest power of two <= the mean row length nnz // rows, 1 .. 64"""
    mean = int(nnz) // int(rows) if rows > 0 else 1
    lg = 1
    while lg < 64 and 2 * lg <= mean:
        lg *= 2
    return lg


def hessian_lanes(qp):
    """lgR = lane_group(nnz(R), n), R = Q - diag(Q) (the `_lanes` of tests/test_gpu_band_qp_sparse_hessian.py)"""
    return lane_group(int(qp.hess_vals.size) - int(np.count_nonzero(qp.hess_csr().diagonal())), qp.n)


def tiles(rows, lg):
    """row tiles a product kernel with `lg` lanes per row walks, 256 // lg rows each; more than MAX_GRID: a second trip"""
    rpb = 256 // lg
    return (rows + rpb - 1) // rpb


def ragged_band(n, m, lens, window, seed):
    """problems.pde_control_like's rule with a row length of its own per row: row i has lens[i] distinct sorted columns, one per
    equal stratum [k window // lens[i], (k + 1) window // lens[i]) of a column window of width `window` centred at
    floor(i n / m) (clamped), at offset lo + floor(u(seed, entry, 11) (hi - lo)), entry = the entry's CSR position; values
    2 u(seed, entry, 12) - 1; the stratum that holds the centre column is placed on it and gets +4.  `lens` is repeated to m
    entries.  x, xhat, qdiag, d, b come from problems._finish.  With one length for every row it IS pde_control_like."""
    window = min(int(window), n)
    lens = np.resize(np.asarray(lens, dtype=np.int64), m)
    assert lens.min() >= 1 and lens.max() <= window
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(rowptr[-1])
    rows = np.repeat(np.arange(m, dtype=np.int64), lens)
    eid = np.arange(nnz, dtype=np.int64)
    ks = eid - rowptr[rows]
    per = lens[rows]
    centre = (np.arange(m, dtype=np.int64) * n) // m
    start = np.clip(centre - window // 2, 0, n - window)
    lo, hi = (ks * window) // per, ((ks + 1) * window) // per
    off = lo + np.floor(problems.uniform01(seed, eid, 11) * (hi - lo)).astype(np.int64)
    vals = 2.0 * problems.uniform01(seed, eid, 12) - 1.0
    rel = (centre - start)[rows]
    hit = (rel >= lo) & (rel < hi)
    cols = start[rows] + np.where(hit, rel, off)
    vals = np.where(hit, vals + 4.0, vals)
    assert cols.min() >= 0 and cols.max() < n and np.all((np.diff(cols) > 0) | (np.diff(rows) > 0))
    return problems._finish(f"ragged-band-n{n}-m{m}", n, m, rowptr, cols, vals, seed)


@dataclasses.dataclass(frozen=True)
class Case:
    """A shape and the literals tests/test_lane_groups_cpu.py pins on it."""
    n: int
    m: int
    lens: tuple           # row lengths, repeated to m rows
    window: int
    seed: int
    nnz: int
    lgA: int
    lgT: int
    rows: tuple           # (shortest, longest) row of A
    cols: tuple           # (empty columns, shortest non-empty column, longest column)
    band: dict            # what qdsolver.band_analysis reports: chains, nblocks, bandwidth_blocks, reordered
    shuffle: int = None   # seed of the row shuffle (`_shuffled` of tests/test_gpu_band_nlp.py) of `base`; None: natural order
    base: str = None

    @property
    def mpad(self):
        return 128 * ((self.m + 127) // 128)


def _band(chains, nblocks, bandwidth_blocks, reordered=0):
    return dict(chains=chains, nblocks=nblocks, bandwidth_blocks=bandwidth_blocks, reordered=reordered)


CASES = {
    "wide-rows": Case(1536, 96, (160,), 512, 31, 15360, 64, 8, (160, 160), (0, 1, 23), _band(1, 1, 0)),
    "m-near-n": Case(1100, 1000, (40,), 128, 32, 40000, 32, 32, (40, 40), (0, 12, 70), _band(1, 8, 1)),
    "both-64": Case(600, 500, (80,), 160, 33, 40000, 64, 64, (80, 80), (0, 28, 111), _band(1, 4, 2)),
    "lgT-16": Case(1000, 500, (40,), 160, 34, 20000, 32, 16, (40, 40), (0, 4, 39), _band(1, 4, 1)),
    "lgT-8": Case(1400, 330, (30, 41, 52), 192, 35, 13530, 32, 8, (30, 52), (0, 2, 19), _band(1, 3, 1)),
    "thin": Case(900, 700, (1, 1, 2, 1, 1, 3, 1), 64, 36, 1000, 1, 1, (1, 3), (146, 1, 5), _band(1, 6, 1)),
    "lg2": Case(900, 300, (2, 3, 2, 1, 5, 2), 64, 37, 750, 2, 1, (1, 5), (361, 1, 4), _band(1, 3, 1)),
    "ragged": Case(1300, 1000, (1, 97, 33, 200, 7, 64, 65, 13), 256, 38, 60000, 32, 32, (1, 200), (0, 14, 83), _band(1, 8, 2)),
    "stride": Case(9000, 8300, (128,), 256, 39, 1062400, 64, 64, (128, 128), (0, 54, 191), _band(2, 65, 4, 1)),
    # the widths the table of the issue leaves to the older suites, so that this table alone covers every width on each side
    "lg4-2": Case(1200, 600, (4, 5, 6, 3), 64, 40, 2700, 4, 2, (3, 6), (99, 1, 8), _band(1, 5, 1)),
    "lg8-4": Case(3600, 1500, (12,), 256, 41, 18000, 8, 4, (12, 12), (20, 1, 16), _band(1, 12, 1)),
    "lg16-2": Case(2000, 250, (17, 23), 128, 42, 5000, 16, 2, (17, 23), (157, 1, 8), _band(1, 2, 1)),
}
for _base, _seed, _bw in (("both-64", 5, 2), ("ragged", 5, 3)):   # (what the reverse Cuthill-McKee pass makes of the shuffle)
    CASES[_base + "-shuffled"] = dataclasses.replace(CASES[_base], shuffle=_seed, base=_base,
                                                     band=_band(1, CASES[_base].band["nblocks"], _bw, 1))
NAMES = list(CASES)

# half-widths of problems.with_sparse_hessian(qp("m-near-n"), hw, HESS_SEED): lgR -> the SMALLEST half-width that reaches it
HESS_BASE, HESS_SEED = "m-near-n", 11
HESS_HALF_WIDTHS = {1: 1, 2: 2, 4: 3, 8: 6, 16: 12, 32: 23, 64: 45}
# (case, half-width): lgR.  Every lgR on HESS_BASE (32 lanes on both sides of A), and half-width 2 on one case per width of lgA
# and of lgT: the kernels that take the Hessian as a template flag (k_bq_epilogue_sq and the block forms) at the other widths
HESS_CASES = {(HESS_BASE, hw): lgr for lgr, hw in HESS_HALF_WIDTHS.items()}
HESS_CASES.update({(name, 2): 2 for name in ("thin", "lg2", "lg4-2", "lg8-4", "lg16-2", "lgT-8", "lgT-16", "both-64")})


@functools.lru_cache(maxsize=None)
def qp(name):
    """the EqQP of a case (shared, read-only)"""
    c = CASES[name]
    if c.base is not None:
        from test_gpu_band_nlp import _shuffled

        out = _shuffled(qp(c.base), c.shuffle)
    else:
        out = ragged_band(c.n, c.m, c.lens, c.window, c.seed)
    for a in (out.rowptr, out.colind, out.vals, out.qdiag, out.d, out.b, out.x, out.xhat):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def hess_qp(name, hw):
    """the case with a sparse objective Hessian of half-width `hw` (a key of HESS_CASES)"""
    return problems.with_sparse_hessian(qp(name), hw, HESS_SEED)


@functools.lru_cache(maxsize=None)
def nlp_data(name):
    """the separable-quadratic model of a case: curvature CURV on the case's pattern"""
    return problems.with_quadratic_constraints(qp(name), curv=CURV, seed=7)


# ---- the yardsticks, each with ONE sparse LU per (model, delta) behind it

@functools.lru_cache(maxsize=None)
def exact_linear(name, delta, hw=None):
    """tests/sparse_hessian_ref.py on the case (hw: on hess_qp(name, hw)); with Q = diag(qdiag) it evaluates the formulae of
    oracle.exact_qp_objgrad / exact_qp_hprod on the same K = [I A'; A -delta I] (tests/test_lane_groups_cpu.py holds the two
    together), and keeps the factor."""
    return SparseHessianRef(qp(name) if hw is None else hess_qp(name, hw), delta)


def exact_linear_with(ref, d, b):
    """the same factor on the model with its linear term and right-hand side replaced (K depends on neither)"""
    out = copy.copy(ref)
    out.qp = dataclasses.replace(ref.qp, d=d, b=b)
    return out


class _KeptFactorOracle(OracleQDSolver):
    """OracleQDSolver's three solves by their definitions (oracle.exact_two_mixed / exact_two_least_squares / exact_two_extras),
    through sparse LUs that are kept while J and delta stay: SepQuadRef refactorises K for every call, which the 8300-row
    case cannot afford.  K = [I J'; J -delta I]; the extras factor J J' + max(delta, 1e-14) I as tests/sepquad_ref.py does."""

    def __init__(self, nlp):
        super().__init__(nlp)
        self._key = self._lu = self._lu_m = None

    def _factor(self, nlp, x):
        J = self._jac(nlp, x)
        key = (hash(J.data.tobytes()), float(nlp.delta))
        if key != self._key:
            n, m = self.nvar, self.ncon
            self._lu = spla.splu(sp.bmat([[sp.identity(n), J.T], [J, -float(nlp.delta) * sp.identity(m)]], format="csc"))
            self._key, self._lu_m = key, None
        return J

    def _kkt(self, top, bottom):
        sol = self._lu.solve(np.concatenate([top, bottom]))
        return sol[:self.nvar], sol[self.nvar:]

    def solve_two_mixed(self, nlp, x, rhs1, rhs2):
        self._factor(nlp, x)
        p1, q1 = self._kkt(np.asarray(rhs1, float), np.zeros(self.ncon))
        p2, q2 = self._kkt(np.zeros(self.nvar), np.asarray(rhs2, float))
        return p1, q1, p2, q2

    def solve_two_least_squares(self, nlp, x, rhs1, rhs2):
        self._factor(nlp, x)
        p1, q1 = self._kkt(np.asarray(rhs1, float), np.zeros(self.ncon))
        p2, q2 = self._kkt(np.asarray(rhs2, float), np.zeros(self.ncon))
        return p1, q1, p2, q2

    def solve_two_extras(self, nlp, x, rhs1, rhs2):
        J = self._factor(nlp, x)
        if self._lu_m is None:
            self._lu_m = spla.splu(sp.csc_matrix(J @ J.T + max(float(nlp.delta), 1e-14) * sp.identity(self.ncon)))
        return self._lu_m.solve(J @ np.asarray(rhs1, float)), self._lu_m.solve(np.asarray(rhs2, float))


@functools.lru_cache(maxsize=None)
def exact_nonlinear(name, delta):
    """tests/sepquad_ref.py on the case at xk = xhat, rho = eta = 0 (set ref.pen.rho / ref.pen.eta), its solves kept"""
    ref = SepQuadRef(nlp_data(name), SIGMA, 0.0, delta, 0.0, qp(name).xhat)
    ref.pen.qdsolver = _KeptFactorOracle(ref.model)
    return ref
