"""The arrow scheme of the banded back-end in numpy, fp64 -- what include/fpsq.h "ARROW BAND" and the kernel comments of
csrc/fpsq_band.hip.h describe, with LAPACK's dense Cholesky in the place of the block-banded one and numpy's summation orders
instead of the device's.  Stored row order: the band rows, then the border rows; L = the long columns, "o" = the others:

    A = [A_b,o U_b; A_s,o U_s],   M = A A' + delta I = M_r + U U',   U = [U_b; U_s] (all rows),
    M_r = [B C; C' D],   B = A_b,o A_b,o' + delta I,   C = A_b,o A_s,o',   D = A_s,o A_s,o' + delta I,
    M_r^-1 [r; t]:  y = B^-1 r,  w_r = S_r^-1 (t - C'y),  u = y - Z_r w_r,   Z_r = B^-1 C,   S_r = D - C'Z_r,
    M^-1 r = y - Z_c w_c,   y = M_r^-1 r,   Z_c = M_r^-1 U,   S_c = I + U'Z_c,   w_c = S_c^-1 U'y.

`msolve` is that nesting as written; `msolve_fused` is the one-pass algebra of the fused kernels, with G = U_s' - U_b'Z_r:
    w_r = S_r^-1 (t - C'y),   w_c = S_c^-1 (U_b'y + G w_r),   band rows y - Z_r w_r - Z_c,b w_c,   border rows w_r - Z_c,s w_c.
The rows of A'q that belong to long columns are taken as w_c, as the device takes them.  The model says what the SCHEME loses
on an input; what a kernel loses beyond that is a defect.  It carries no fitted constant."""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp


def _chol_solve(L, g):
    return sla.solve_triangular(L.T, sla.solve_triangular(L, g, lower=True), lower=False)


class ArrowModel:
    def __init__(self, A, delta, rows, cols):
        """rows: the border rows, cols: the long columns (the caller's indices)"""
        self.A = sp.csr_matrix(A)
        self.m, self.n = self.A.shape
        self.rows = np.asarray(rows, dtype=np.int64)
        self.cols = np.asarray(cols, dtype=np.int64)
        self.band = np.setdiff1d(np.arange(self.m), self.rows)
        self.order = np.concatenate([self.band, self.rows])          # stored row -> the caller's
        self.mb, delta = self.band.size, float(delta)
        rest = np.setdiff1d(np.arange(self.n), self.cols)
        Ao = self.A[self.order][:, rest]
        Ab, As = Ao[:self.mb], Ao[self.mb:]
        self.U = self.A[self.order][:, self.cols].toarray()
        self.B = (Ab @ Ab.T).toarray() + delta * np.eye(self.mb)
        self.C = (Ab @ As.T).toarray()
        self.D = (As @ As.T).toarray() + delta * np.eye(self.rows.size)
        self.cf = sla.cho_factor(self.B, lower=True)
        self.Zr = sla.cho_solve(self.cf, self.C)
        Sr = self.D - self.C.T @ self.Zr
        self.Lr = np.linalg.cholesky(np.tril(Sr) + np.tril(Sr, -1).T)
        self.Zc = self._mr_solve(self.U)
        Sc = np.eye(self.cols.size) + self.U.T @ self.Zc
        self.Lc = np.linalg.cholesky(np.tril(Sc) + np.tril(Sc, -1).T)   # (the lower triangle, as the kernel reads it)
        d = np.diag(self.Lc)
        self.pivot_ratio = float((d.max() / d.min()) ** 2)
        self.G = self.U[self.mb:].T - self.U[:self.mb].T @ self.Zr

    def _mr_solve(self, R):
        """M_r^-1 R for R: (m, k) in the stored order"""
        y = sla.cho_solve(self.cf, R[:self.mb])
        wr = _chol_solve(self.Lr, R[self.mb:] - self.C.T @ y)
        return np.vstack([y - self.Zr @ wr, wr])

    def msolve(self, R):
        """(M^-1 R, w_c), nested; R: (m, k) in the CALLER's row order, and so is the result"""
        y = self._mr_solve(R[self.order])
        wc = _chol_solve(self.Lc, self.U.T @ y)
        out = np.empty_like(y)
        out[self.order] = y - self.Zc @ wc
        return out, wc

    def msolve_fused(self, R):
        """the same by the one-pass algebra of k_arrow_reduce / k_arrow_update"""
        Rs = R[self.order]
        y = sla.cho_solve(self.cf, Rs[:self.mb])
        wr = _chol_solve(self.Lr, Rs[self.mb:] - self.C.T @ y)
        wc = _chol_solve(self.Lc, self.U[:self.mb].T @ y + self.G @ wr)
        u = np.vstack([y - self.Zr @ wr - self.Zc[:self.mb] @ wc, wr - self.Zc[self.mb:] @ wc])
        out = np.empty_like(u)
        out[self.order] = u
        return out, wc

    def at_mul(self, q, w):
        """A'q with the rows of the long columns replaced by w"""
        out = self.A.T @ q
        out[self.cols] = w
        return out

    def solve(self, r1, r2, mixed, fused=False):
        """(p1, q1, p2, q2) of solve_two_mixed (mixed) or solve_two_least_squares, as the entries form them"""
        A = self.A
        r1, r2 = np.asarray(r1, dtype=np.float64), np.asarray(r2, dtype=np.float64)
        Q, W = (self.msolve_fused if fused else self.msolve)(np.column_stack([A @ r1, -r2 if mixed else A @ r2]))
        q1, q2 = Q[:, 0].copy(), Q[:, 1].copy()
        p1 = r1 - self.at_mul(q1, W[:, 0])
        p2 = -self.at_mul(q2, W[:, 1]) if mixed else r2 - self.at_mul(q2, W[:, 1])
        return p1, q1, p2, q2
