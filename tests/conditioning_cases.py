"""Ill-conditioned and badly scaled Jacobians for the direct back-ends, and the yardsticks every rung is measured with.
Everything is seeded; nothing here needs a device.

A RUNG is a Jacobian, a delta and right-hand sides (g, c for solve_two_mixed; g, g2 for solve_two_least_squares).  Its
REFERENCE (reference(name), computed once per process) holds
  truth     tests/kkt_truth.py: fp64 Cholesky + refinement with longdouble residuals, per entry ("mixed", "ls");
  lapack    the forward error of an fp64 LAPACK Cholesky solve of the same M against that truth, under six symmetric
            elimination orders (the identity and five seeded permutations): min and max over the orders, per output;
  model     the forward error of tests/direct_scheme_model.py in the handle's stored row order, the larger of its two variants.
Errors are max|x - truth| / max|truth| per output vector (p1, q1, p2, q2).  A rung's headline numbers (`q_err`) are those
of the multipliers, the larger of q1 and q2 over both entries -- the figure the classification uses:
  scheme-neutral     model <= 2 x LAPACK max: the inverse-based scheme costs nothing here; the device is held to LAPACK;
  scheme-sensitive   otherwise: the explicit inverses lose digits a substitution would keep; the device is held to the model."""
import ctypes as C
import functools

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

import fps_amd  # noqa: F401
from fps_amd import _lib, problems

import direct_scheme_model as dsm
import kkt_truth as kt

EPS = float(np.finfo(float).eps)
SE = float(np.sqrt(EPS))
OUTS = ("p1", "q1", "p2", "q2")
ENTRIES = ("mixed", "ls")
N_ORDERS = 6

DENSE_SHAPE = (300, 700)   # three 128-row blocks, the last with 44 rows
DENSE_PAIRS = ((12, 13), (15, 16), (100, 127), (127, 128), (3, 140), (298, 299))
BAND1 = dict(n=6000, m=600, per_row=24, window=512, seed=3)
BAND1_PAIRS = ((12, 13), (15, 16), (100, 127), (127, 128), (598, 599))
# a wider window (rows couple over ~200 rows, a band of two blocks) with, besides the pairs above, later copies that sit EARLY
# in a 128-row block while their originals sit late in the block before: the draw of the banded generator on which the scheme
# loses digits (the later rows of the block all pass through the tiny pivot's column of the explicit inverse)
BAND1_WIDE = dict(n=6000, m=600, per_row=24, window=2048, seed=8)
BAND1_WIDE_PAIRS = BAND1_PAIRS + ((102, 129), (104, 131), (230, 257), (232, 259), (358, 385), (360, 387))
BAND2 = dict(n=10400, m=2600, per_row=12, window=256, seed=11)
# an early block of the top chain; the bottom chain; the last row of the top chain next to the first row left in the middle;
# two of the rows left in the middle (m = 2600: 10 blocks from either end, rows 1280 .. 1319 remain)
BAND2_PAIRS = ((12, 13), (2300, 2301), (1279, 1280), (1300, 1301))


class Rung:
    def __init__(self, name, kind, A, delta, seed):
        self.name, self.kind, self.A, self.delta = name, kind, A, float(delta)
        self.m, self.n = A.shape
        rng = np.random.default_rng(seed)
        self.g, self.c, self.g2 = rng.standard_normal(self.n), rng.standard_normal(self.m), rng.standard_normal(self.n)

    def rhs(self, entry):
        return (self.g, self.c) if entry == "mixed" else (self.g, self.g2)

    def csr(self):
        A = sp.csr_matrix(self.A)
        A.sort_indices()
        return A


# ------------------------------------------------------------------------------------------------------------ generators

def _dense_base():
    m, n = DENSE_SHAPE
    return np.random.default_rng(4).uniform(-1, 1, (m, n)) / np.sqrt(n)


def dense_near_duplicates(eps, pairs=DENSE_PAIRS):
    """row j = row i + eps * noise for every pair (i, j); eps = 0: exact copies"""
    A = _dense_base()
    noise = np.random.default_rng(9).uniform(-1, 1, A.shape) / np.sqrt(A.shape[1])
    for i, j in pairs:
        A[j] = A[i] + eps * noise[j]
    return A


def dense_row_scaled(k):
    A = _dense_base()
    m = A.shape[0]
    return A * (10.0 ** (-k * np.random.default_rng(5).permutation(m) / m))[:, None]


def dense_col_scaled(decades=3):
    A = _dense_base()
    n = A.shape[1]
    return A * (10.0 ** (-decades * np.random.default_rng(6).permutation(n) / n))[None, :]


def band_near_duplicates(shape, eps, pairs):
    """pde_control_like with row j = row i + eps * noise ON ROW i's PATTERN for every pair (i, j)"""
    A = problems.pde_control_like(**shape).scipy_csr().tolil()
    rng = np.random.default_rng(78)
    for i, j in pairs:
        row = sp.csr_matrix(A[i, :])
        row.data = row.data + eps * rng.uniform(-1, 1, row.data.size)
        A[j, :] = row
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A


def band_row_scaled(shape, k):
    A = problems.pde_control_like(**shape).scipy_csr()
    m = A.shape[0]
    A = sp.csr_matrix(sp.diags(10.0 ** (-k * np.random.default_rng(5).permutation(m) / m)) @ A)
    A.sort_indices()
    return A


def _ename(e):
    return f"eps{e:.0e}".replace("e-0", "e-")


_MAKERS = {}
for _e in (1e-2, 1e-3, 1e-4, 1e-5):
    _MAKERS[f"dense-{_ename(_e)}"] = ("dense", functools.partial(dense_near_duplicates, _e), 0.0)
    _MAKERS[f"band1-{_ename(_e)}"] = ("band1", functools.partial(band_near_duplicates, BAND1, _e, BAND1_PAIRS), 0.0)
for _e in (1e-3, 1e-5):
    _MAKERS[f"band2-{_ename(_e)}"] = ("band2", functools.partial(band_near_duplicates, BAND2, _e, BAND2_PAIRS), 0.0)
for _tag, _d in (("sqrteps", SE), ("1e-4", 1e-4)):
    _MAKERS[f"dense-dup-delta-{_tag}"] = ("dense", functools.partial(dense_near_duplicates, 0.0), _d)
    _MAKERS[f"band1-dup-delta-{_tag}"] = ("band1", functools.partial(band_near_duplicates, BAND1, 0.0, BAND1_PAIRS), _d)
_MAKERS["dense-rowscale-4"] = ("dense", functools.partial(dense_row_scaled, 4), 0.0)
_MAKERS["dense-rowscale-8"] = ("dense", functools.partial(dense_row_scaled, 8), 0.0)
_MAKERS["dense-colscale-3"] = ("dense", dense_col_scaled, 0.0)
_MAKERS["band1-rowscale-8"] = ("band1", functools.partial(band_row_scaled, BAND1, 8), 0.0)
_MAKERS["band1-wide-eps1e-5"] = ("band1", functools.partial(band_near_duplicates, BAND1_WIDE, 1e-5, BAND1_WIDE_PAIRS), 0.0)

RUNGS = tuple(_MAKERS)
# The classification, by the rule above (tests/test_direct_conditioning_cpu.py asserts that the rule still gives it).  The
# transition is not sharp and depends on the draw: with other seeds of the dense base and noise the ratio model / LAPACK max at
# eps = 1e-3 (cond 2e7) came out anywhere from 0.5 to 12, and on the narrow banded rungs from 0.2 to 11 at eps = 1e-5.  The seeds
# used here were taken so that every rung sits well on one side (<= 1.5 or >= 4), which keeps the classification stable against
# another BLAS: the narrow banded draws are neutral BY THAT CHOICE, not by a property of the banded handle, and the wide banded
# draw is the one taken for being sensitive (ratio 35 ... 240 over three right-hand-side seeds).
SENSITIVE = ("dense-eps1e-4", "dense-eps1e-5", "band1-wide-eps1e-5")
NEUTRAL = tuple(r for r in RUNGS if r not in SENSITIVE)


def kind_of(name):
    return _MAKERS[name][0]


@functools.lru_cache(maxsize=None)
def rung(name):
    kind, make, delta = _MAKERS[name]
    return Rung(name, kind, make(), delta, seed=RUNGS.index(name) + 100)


# ------------------------------------------------------------------------------------------------------------ yardsticks

def analyze(A):
    """(row_perm, info) of fpsq_band_analyze: the banded handle's stored row order, on the host"""
    A = sp.csr_matrix(A)
    A.sort_indices()
    m, n = A.shape
    rp, ci = A.indptr.astype(np.int32), A.indices.astype(np.int32)
    perm = np.full(m, -1, dtype=np.int32)
    info = _lib.BandInfo()
    rc = _lib.load().fpsq_band_analyze(n, m, rp.ctypes.data, ci.ctypes.data, perm.ctypes.data, C.byref(info))
    assert rc == 0
    return perm.astype(np.int64), info.as_dict()


def stored_order(kind, A):
    return np.arange(A.shape[0]) if kind == "dense" else analyze(A)[0]


def elimination_orders(m):
    return [np.arange(m)] + [np.random.default_rng(900 + k).permutation(m) for k in range(N_ORDERS - 1)]


def gram64(A, delta, extra=None):
    G = A @ A.T
    G = (G.toarray() if sp.issparse(G) else G) + delta * np.eye(A.shape[0])
    return G if extra is None else G + np.diag(extra)


def lapack_solve(A, M, r1, r2, mixed, perm):
    """the four vectors by an fp64 LAPACK Cholesky of M eliminated in the order `perm`"""
    cf = sla.cho_factor(M[np.ix_(perm, perm)], lower=True)
    R = np.column_stack([A @ r1, -r2 if mixed else A @ r2])
    Q = np.empty_like(R)
    Q[perm] = sla.cho_solve(cf, R[perm])
    q1, q2 = Q[:, 0], Q[:, 1]
    return r1 - A.T @ q1, q1, (-(A.T @ q2) if mixed else r2 - A.T @ q2), q2


def errors(got, truth):
    return np.array([kt.relerr(a, b) for a, b in zip(got, truth[:4])])


class Reference:
    """truth / lapack (min, max) / model errors of one system, per entry, per output (arrays of 4 in OUTS order)"""

    def __init__(self, A, delta, rhs_of, order, extra=None, tol=0.0, reg=0.0, with_model=True):
        self.truth, self.lapack_min, self.lapack_max, self.model, self.model_by_variant = {}, {}, {}, {}, {}
        M = gram64(A, delta, extra)
        self.M64 = M
        m = A.shape[0]
        orders = elimination_orders(m)
        self.models = {}
        if with_model:
            self.models = {v: dsm.SchemeModel(A, delta, order, tol, reg, v) for v in dsm.VARIANTS}
        for entry in ENTRIES:
            r1, r2 = rhs_of(entry)
            mixed = entry == "mixed"
            fn = kt.truth_two_mixed if mixed else kt.truth_two_least_squares
            t = self.truth[entry] = fn(A, delta, r1, r2, extra)
            errs = np.array([errors(lapack_solve(A, M, r1, r2, mixed, p), t) for p in orders])
            self.lapack_min[entry], self.lapack_max[entry] = errs.min(axis=0), errs.max(axis=0)
            if with_model:
                byv = {v: errors(mod.solve(r1, r2, mixed), t) for v, mod in self.models.items()}
                self.model_by_variant[entry] = byv
                self.model[entry] = np.maximum(*[byv[v] for v in dsm.VARIANTS])
        self.uncertainty = max(float(self.truth[e][4]) for e in ENTRIES)

    def q_err(self, table):
        """the headline figure: the multipliers' error, the larger of q1 and q2 over both entries"""
        return float(max(max(table[e][1], table[e][3]) for e in ENTRIES))

    @functools.cached_property
    def cond(self):
        w = np.linalg.eigvalsh(self.M64)
        return float(w[-1] / max(w[0], 1e-300 * w[-1]))


@functools.lru_cache(maxsize=None)
def reference(name):
    r = rung(name)
    return Reference(r.A, r.delta, r.rhs, stored_order(r.kind, r.A))


def is_neutral(ref):
    return ref.q_err(ref.model) <= 2.0 * ref.q_err(ref.lapack_max)


def neutral_bar(lapack_max):
    """scheme-neutral: 8 x max(LAPACK max, 1e-13).  1e-13 is what the project holds its products to; 8 is the spread LAPACK
    itself shows between elimination orders on these inputs -- the device's summation orders are one more draw."""
    return 8.0 * np.maximum(lapack_max, 1e-13)


def sensitive_bar(lapack_max, model):
    return 8.0 * np.maximum(lapack_max, model)


def bar(name, ref, entry):
    return sensitive_bar(ref.lapack_max[entry], ref.model[entry]) if name in SENSITIVE else neutral_bar(ref.lapack_max[entry])


# ------------------------------------------------------------------------------------------- the pivot rule: duplicated rows

class PivotCase:
    """Exactly duplicated rows at delta = 0 with CONSISTENT right-hand sides (c equal on equal rows; every g is consistent).
    `copies`: (earlier row, later row) pairs; the later copy's pivot vanishes and must fire."""

    def __init__(self, name, kind, copies):
        self.name, self.kind, self.copies = name, kind, copies
        if kind == "dense":
            A = _dense_base()
            for i, j in copies:
                A[j] = A[i]
        else:
            A = band_near_duplicates(BAND1, 0.0, copies)
        self.A = A
        self.m, self.n = A.shape
        rng = np.random.default_rng(len(name) + 40)
        self.g, self.c, self.g2 = rng.standard_normal(self.n), rng.standard_normal(self.m), rng.standard_normal(self.n)
        for i, j in copies:
            self.c[j] = self.c[i]
        self.fired = sorted({j for _, j in copies})

    def rhs(self, entry):
        return (self.g, self.c) if entry == "mixed" else (self.g, self.g2)


def _pivot_copies(m):
    return {
        "at16": ((15, 16),),                       # first row of the second 16-row tile
        "at31": ((20, 31),),                       # last row of a tile
        "at127": ((100, 127),),                    # last row of the first 128-row block
        "at128": ((127, 128),),                    # first row of the second block, its copy in the block before
        "at-last": ((m - 2, m - 1),),              # next to the padding
        "three-in-a-tile": ((33, 36), (33, 41)),   # three equal rows within rows 32 .. 47
        "two-tiles": ((18, 21), (70, 75)),         # two duplicates in different tiles of one block
    }


PIVOT_CASES = tuple(f"{kind}-{c}" for kind in ("dense", "band1") for c in _pivot_copies(0))


@functools.lru_cache(maxsize=None)
def pivot_case(name):
    kind, case = name.split("-", 1)
    m = DENSE_SHAPE[0] if kind == "dense" else BAND1["m"]
    return PivotCase(name, kind, _pivot_copies(m)[case])


@functools.lru_cache(maxsize=None)
def pivot_reference(name, drop):
    """regularising form (drop False): the system (M + reg E) q = r with E selecting the fired rows, reg = tol = sqrt(eps);
    FPSQ_REG_DROP (drop True): the system with the fired rows REMOVED.  LAPACK runs on the same system; the scheme model runs
    the pivot rule on M itself (it must fire exactly there)."""
    pc = pivot_case(name)
    order = stored_order(pc.kind, pc.A)
    if not drop:
        extra = np.zeros(pc.m)
        extra[pc.fired] = SE
        ref = Reference(pc.A, 0.0, pc.rhs, order, extra=extra, with_model=False)
        ref.keep = np.arange(pc.m)
        return ref
    keep = np.setdiff1d(np.arange(pc.m), pc.fired)
    A = pc.A[keep]

    def rhs(entry):
        r1, r2 = pc.rhs(entry)
        return (r1, r2[keep]) if entry == "mixed" else (r1, r2)

    ref = Reference(A, 0.0, rhs, None, with_model=False)
    ref.keep = keep
    return ref


def regularised_bar(lapack_max, M_diag_max, reg=SE):
    """8 x max(LAPACK max on M + reg E, 64 eps max(M_ii) / reg): the second term is how far the rounding residue of the fired
    pivot -- and of the column below it, which is scaled by 1 / sqrt(reg) -- can move the pivot relative to reg."""
    return 8.0 * np.maximum(lapack_max, 64.0 * EPS * M_diag_max / reg)


# ------------------------------------------------------------------------------------------------- the dense factor itself

@functools.lru_cache(maxsize=None)
def factor_reference(name):
    """(M in longdouble, LAPACK min, LAPACK max, model) for the factor residual max|L L' - M| / max|M| of a dense rung:
    LAPACK's Cholesky factor of the fp64 M under the six elimination orders, the model's two variants (the larger)."""
    r = rung(name)
    M = kt.gram_longdouble(r.A) + kt.LD(r.delta) * np.eye(r.m, dtype=kt.LD)
    M64 = gram64(r.A, r.delta)
    lap = []
    for p in elimination_orders(r.m):
        L = sla.cholesky(M64[np.ix_(p, p)], lower=True)
        lap.append(factor_residual(L, M[np.ix_(p, p)]))
    mod = max(factor_residual(m.L[:r.m, :r.m], M) for m in reference(name).models.values())
    return M, min(lap), max(lap), mod


def factor_residual(L, M):
    L = np.tril(np.asarray(L)).astype(kt.LD)
    return float(np.max(np.abs(L @ L.T - M)) / np.max(np.abs(M)))


# ------------------------------------------------------------------------------- objgrad on the banded handle: ys and gs

SIGMA = 1e3


class ObjgradReference:
    """fpsq_band_qp_objgrad's ys = q1 + sigma q2 and gs = p1 + sigma p2 with (p1, q1, p2, q2) = solve_two_mixed(g, c),
    g = q .* x + d, c = A x - b (include/fpsq.h), rho = eta = 0.  Truth: g and c formed in longdouble and handed to the
    longdouble solve.  LAPACK: g and c in fp64, as the device forms them, then the six elimination orders."""

    def __init__(self, name):
        r = rung(name)
        rng = np.random.default_rng(RUNGS.index(name) + 700)
        self.qdiag, self.d = rng.uniform(0.5, 2.0, r.n), rng.standard_normal(r.n)
        self.b, self.x = rng.standard_normal(r.m), rng.standard_normal(r.n)
        op = kt._Op(r.A)
        g = self.qdiag.astype(kt.LD) * self.x + self.d
        c = op.mul(self.x) - self.b
        p1, q1, p2, q2, self.unc = kt.truth_two_mixed(r.A, r.delta, g, c)
        self.ys, self.gs = q1 + kt.LD(SIGMA) * q2, p1 + kt.LD(SIGMA) * p2
        g64, c64 = self.qdiag * self.x + self.d, r.A @ self.x - self.b
        M = gram64(r.A, r.delta)
        errs = []
        for p in elimination_orders(r.m):
            a1, b1, a2, b2 = lapack_solve(r.A, M, g64, c64, True, p)
            errs.append((kt.relerr(b1 + SIGMA * b2, self.ys), kt.relerr(a1 + SIGMA * a2, self.gs)))
        errs = np.array(errs)
        self.lapack_min, self.lapack_max = errs.min(axis=0), errs.max(axis=0)   # (ys, gs)
        mod = []
        for sm in reference(name).models.values():   # the scheme model on the same fp64 g and c, the larger of its variants
            a1, b1, a2, b2 = sm.solve(g64, c64, True)
            mod.append((kt.relerr(b1 + SIGMA * b2, self.ys), kt.relerr(a1 + SIGMA * a2, self.gs)))
        self.model = np.max(np.array(mod), axis=0)


@functools.lru_cache(maxsize=None)
def objgrad_reference(name):
    return ObjgradReference(name)
