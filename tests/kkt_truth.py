"""A truth for the two saddle-point solves that is better than fp64: the normal equations  M q = r,  M = A A' + delta I
(+ diag(extra)), solved by an fp64 Cholesky factorisation plus iterative refinement whose residuals are formed in
numpy.longdouble (64-bit mantissa on x86-64) WITHOUT forming M -- r - (A (A'q) + delta q + extra .* q) -- and whose iterate is
kept in longdouble; p follows from q in longdouble.  As long as cond(M) eps_fp64 < 1 the refinement contracts and the answer
is right to about cond(M) eps_longdouble: 1e-13 or better at cond 2e11, where an fp64 factorisation alone keeps five digits.

`uncertainty` = the size of the LAST refinement step relative to the solution (max over the two systems, max norm): what
the iteration still moves by.  It understates the error somewhat (the residual's own rounding error repeats from step to
step; against mpmath it is a factor of ten, and tests/test_direct_conditioning_cpu.py holds it below a hundred), which is why
a caller that is about to apply a bar FAILS (check_uncertainty) as soon as the uncertainty exceeds 1e-4 of that bar: the
truth is then within 1 % of the bar.

A is a dense array or a scipy.sparse matrix; sparse products are hand-written CSR sums on longdouble arrays (scipy.sparse
has no longdouble)."""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

LD = np.longdouble
MAX_STEPS = 40


class _Op:
    """A x and A'y in longdouble"""

    def __init__(self, A):
        self.sparse = sp.issparse(A)
        if self.sparse:
            A = sp.csr_matrix(A)
            A.sort_indices()
            self.m, self.n = A.shape
            self.rowptr = A.indptr.astype(np.int64)
            self.cols = A.indices.astype(np.int64)
            self.vals = A.data.astype(LD)
            self.rows = np.repeat(np.arange(self.m, dtype=np.int64), np.diff(self.rowptr))
            self.nonempty = np.flatnonzero(np.diff(self.rowptr) > 0)
            self.A64 = A
        else:
            self.A64 = np.asarray(A, dtype=np.float64)
            self.m, self.n = self.A64.shape
            self.Ald = self.A64.astype(LD)

    def mul(self, x):
        x = np.asarray(x, dtype=LD)
        if not self.sparse:
            return self.Ald @ x
        out = np.zeros(self.m, dtype=LD)
        if self.vals.size:
            out[self.nonempty] = np.add.reduceat(self.vals * x[self.cols], self.rowptr[self.nonempty])
        return out

    def tmul(self, y):
        y = np.asarray(y, dtype=LD)
        if not self.sparse:
            return self.Ald.T @ y
        out = np.zeros(self.n, dtype=LD)
        np.add.at(out, self.cols, self.vals * y[self.rows])
        return out

    def gram64(self):
        G = self.A64 @ self.A64.T
        return G.toarray() if self.sparse else G


def gram_longdouble(A):
    """A A' in longdouble, dense (for the residual of a factor; small m only)"""
    A = A.toarray() if sp.issparse(A) else np.asarray(A)
    A = A.astype(LD)
    return A @ A.T


class NormalEquations:
    """M = A A' + delta I + diag(extra): fp64 factor for the corrections, longdouble operator for the residuals"""

    def __init__(self, A, delta, extra=None):
        self.op = _Op(A)
        self.delta = LD(delta)
        self.extra = None if extra is None else np.asarray(extra, dtype=LD)
        M = self.op.gram64() + float(delta) * np.eye(self.op.m)
        if extra is not None:
            M = M + np.diag(np.asarray(extra, dtype=np.float64))
        self.M64 = M
        self.cf = sla.cho_factor(M, lower=True)

    def apply(self, q):
        out = self.op.mul(self.op.tmul(q)) + self.delta * q
        return out if self.extra is None else out + self.extra * q

    def solve(self, r):
        """(q in longdouble, size of the last refinement step relative to q, that step)"""
        r = np.asarray(r, dtype=LD)
        q = np.zeros(self.op.m, dtype=LD)
        if not np.any(r):
            return q, 0.0, q
        last = np.inf
        for _ in range(MAX_STEPS):
            res = r - self.apply(q)
            dq = sla.cho_solve(self.cf, res.astype(np.float64)).astype(LD)
            q = q + dq
            step = float(np.max(np.abs(dq)) / np.max(np.abs(q)))
            stalled = step >= 0.5 * last   # the steps have stopped shrinking: the longdouble residual's own rounding level
            last = step
            if step == 0.0 or stalled:
                break
        return q, last, dq


class Uncertainty(float):
    """the last refinement step relative to the solution: the larger of the two multiplier vectors' as the number itself,
    and per output in `per_output` (p1, q1, p2, q2; for p the image A'dq of the step relative to p -- the near-null
    directions of A' that dominate a step of q hardly move p, so p is known much better than q)"""
    per_output = None


def _two(ne, rq1, rq2, r1, r2, mixed):
    q1, u1, d1 = ne.solve(rq1)
    q2, u2, d2 = ne.solve(rq2)
    p1 = np.asarray(r1, dtype=LD) - ne.op.tmul(q1)
    p2 = -ne.op.tmul(q2) if mixed else np.asarray(r2, dtype=LD) - ne.op.tmul(q2)
    unc = Uncertainty(max(u1, u2))
    unc.per_output = np.array([relerr(p1 + ne.op.tmul(d1), p1), u1, relerr(p2 + ne.op.tmul(d2), p2), u2])
    return p1, q1, p2, q2, unc


def truth_two_mixed(A, delta, r1, r2, extra=None):
    """K [p1; q1] = [r1; 0], K [p2; q2] = [0; r2] with K = [I A'; A -(delta I + diag(extra))]:
    q1 = M^-1 A r1, p1 = r1 - A'q1, q2 = -M^-1 r2, p2 = -A'q2.  Returns (p1, q1, p2, q2, uncertainty), longdouble arrays.
    r1, r2 may be longdouble themselves."""
    ne = NormalEquations(A, delta, extra)
    return _two(ne, ne.op.mul(r1), -np.asarray(r2, dtype=LD), r1, r2, True)


def truth_two_least_squares(A, delta, r1, r2, extra=None):
    """K [p1; q1] = [r1; 0], K [p2; q2] = [r2; 0]:  q_i = M^-1 A r_i, p_i = r_i - A'q_i."""
    ne = NormalEquations(A, delta, extra)
    return _two(ne, ne.op.mul(r1), ne.op.mul(r2), r1, r2, False)


def check_uncertainty(uncertainty, bar, what=""):
    """The reported uncertainty must be at most 1e-4 of the bar it serves -- with the understatement of up to 1e2 that the
    mpmath cross-check allows, a truth within 1 % of the bar --; otherwise the test FAILS (it does not skip).
    `bar`: one number (held against the multipliers' uncertainty) or one per output (p1, q1, p2, q2)."""
    bar = np.asarray(bar, dtype=np.float64)
    unc = uncertainty.per_output if bar.shape == (4,) else float(uncertainty)
    assert np.all(unc <= 1e-4 * bar), f"{what}: truth uncertain to {unc}, bar {bar}"


def relerr(got, want):
    """max|got - want| / max|want|, the difference formed in longdouble"""
    want = np.asarray(want, dtype=LD)
    return float(np.max(np.abs(np.asarray(got, dtype=LD) - want)) / max(np.max(np.abs(want)), LD(1e-300)))


def mpmath_two_mixed(A, delta, r1, r2, dps=60):
    """the same four vectors by mpmath at `dps` digits (dense, tiny shapes only): the cross-check of the longdouble truth"""
    import mpmath as mp

    A = np.asarray(A, dtype=np.float64)
    m, n = A.shape
    with mp.workdps(dps):
        Am = mp.matrix(A.tolist())
        M = Am * Am.T + mp.mpf(float(delta)) * mp.eye(m)
        g, c = mp.matrix([float(v) for v in r1]), mp.matrix([float(v) for v in r2])
        q1 = mp.lu_solve(M, Am * g)
        q2 = -mp.lu_solve(M, c)
        p1 = g - Am.T * q1
        p2 = -(Am.T * q2)
        return [np.array([LD(mp.nstr(v, 25)) for v in vec], dtype=LD) for vec in (p1, q1, p2, q2)]
