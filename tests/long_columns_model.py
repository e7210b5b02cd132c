"""The long-column scheme of the banded back-end in numpy, fp64 -- what include/fpsq.h "LONG COLUMNS" and the kernel comments
of csrc/fpsq_band.hip.h describe, with LAPACK's dense Cholesky in the place of the block-banded one and numpy's summation
orders instead of the device's:

    A = [A_b | U]  (U: the long columns),   B = A_b A_b' + delta I,   Z = B^-1 U,   S = I + U'Z = L_s L_s',
    M^-1 r = y - Z w,   y = B^-1 r,   w = S^-1 (U'y).

The rows of A'q that belong to long columns are taken as w (U'(y - Z w) = w), as the device takes them.  The model says what
the SCHEME loses on an input -- roughly cond(B) cond(S) where the long columns dominate; what a kernel loses beyond that is a
defect.  It carries no fitted constant."""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp


class LongColumnsModel:
    def __init__(self, A, delta, cols):
        self.A = sp.csr_matrix(A)
        self.m, self.n = self.A.shape
        self.cols = np.asarray(cols, dtype=np.int64)
        rest = np.setdiff1d(np.arange(self.n), self.cols)
        self.U = self.A[:, self.cols].toarray()
        Ab = self.A[:, rest]
        self.B = (Ab @ Ab.T).toarray() + float(delta) * np.eye(self.m)
        self.cf = sla.cho_factor(self.B, lower=True)
        self.Z = sla.cho_solve(self.cf, self.U)
        self.S = np.eye(self.cols.size) + self.U.T @ self.Z
        self.Ls = np.linalg.cholesky(np.tril(self.S) + np.tril(self.S, -1).T)   # (the lower triangle, as the kernel reads it)
        d = np.diag(self.Ls)
        self.pivot_ratio = float((d.max() / d.min()) ** 2)

    def msolve(self, R):
        """(M^-1 R, w) for R: (m, k)"""
        y = sla.cho_solve(self.cf, R)
        g = self.U.T @ y
        w = sla.solve_triangular(self.Ls.T, sla.solve_triangular(self.Ls, g, lower=True), lower=False)
        return y - self.Z @ w, w

    def at_mul(self, q, w):
        """A'q with the rows of the long columns replaced by w"""
        out = self.A.T @ q
        out[self.cols] = w
        return out

    def solve(self, r1, r2, mixed):
        """(p1, q1, p2, q2) of solve_two_mixed (mixed) or solve_two_least_squares, as the entries form them"""
        A = self.A
        r1, r2 = np.asarray(r1, dtype=np.float64), np.asarray(r2, dtype=np.float64)
        Q, W = self.msolve(np.column_stack([A @ r1, -r2 if mixed else A @ r2]))
        q1, q2 = Q[:, 0].copy(), Q[:, 1].copy()
        p1 = r1 - self.at_mul(q1, W[:, 0])
        p2 = -self.at_mul(q2, W[:, 1]) if mixed else r2 - self.at_mul(q2, W[:, 1])
        return p1, q1, p2, q2
