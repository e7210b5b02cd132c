"""The direct back-ends' elimination scheme in numpy, fp64 -- what DESIGN.md section 7 and the kernel comments of
csrc/fpsq_direct.hip.h describe, with numpy's summation orders instead of the device's:

  * M = A A' + delta I in a given STORED row order, padded to a multiple of 128 rows; pad rows are decoupled (unit diagonal);
  * right-looking blocked Cholesky with 128-row blocks: the diagonal block is factored and the EXPLICIT inverse X_k = L_kk^-1
    formed (k_potrf_inv128m); panels are products L_ik = M_ik X_k'; the trailing matrix takes M_ij -= L_ik L_jk';
  * both sweeps multiply by X_k / X_k' and never substitute (k_trsv_step3, k_trsv_chain, k_trsm_chain16):
        forward   y_k = X_k r_k,   r_i -= L_ik y_k (i > k);      backward   q_k = X_k' y_k,   y_i -= L_ki' q_k (i < k);
  * the pivot rule of wave_diag16:  `if not (d > tol): d = reg; count += 1`  with a regularisation set (only the diagonal
    entry is replaced: the rest of the column keeps what rounding left and is scaled by 1 / sqrt(reg)), and without one
    `if not (d > 0): d = 1` with the first such row recorded.

Two variants of the diagonal block, because "the explicit inverse" can be had in two ways:
  "trsolve"   unblocked Cholesky of the 128 x 128 block, X_k from a triangular solve of the identity;
  "doubling"  what the kernel does: eight 16-column panels, left-looking; each 16 x 16 diagonal tile factored with its own
              inverse X16, the tiles below it multiplied by X16'; then X_k by doubling, X21 = -X22 (L21 X11), from the 16 x 16
              inverses up to 128.
A rung's model error is the larger of the two.  The model says what the ALGORITHM loses on an input; what a kernel loses
beyond that is a defect.  It carries no fitted constant."""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

DB = 128
TILE = 16
VARIANTS = ("trsolve", "doubling")


class _Pivots:
    def __init__(self, tol, reg, size):
        self.dyn = reg > 0.0
        self.thr = tol if self.dyn else 0.0
        self.sub = reg if self.dyn else 1.0
        self.seen = np.full(size, np.nan)   # every pivot as the test saw it (before any replacement), by stored position
        self.fired = []                     # stored positions whose pivot was replaced


def _chol_unblocked(a, off, pv):
    """in-place right-looking Cholesky of the lower triangle of `a` with the pivot rule; `off`: stored position of row 0"""
    n = a.shape[0]
    for j in range(n):
        d = a[j, j]
        pv.seen[off + j] = d
        if not (d > pv.thr):
            pv.fired.append(off + j)
            d = pv.sub
        rp = 1.0 / np.sqrt(d)
        col = a[j + 1:, j] * rp
        a[j, j] = d * rp
        a[j + 1:, j] = col
        a[j + 1:, j + 1:] -= np.outer(col, col)
    return np.tril(a)


def _diag_block(Mkk, off, pv, variant):
    """(L_kk, X_k = L_kk^-1) of one 128 x 128 diagonal block"""
    if variant == "trsolve":
        L = _chol_unblocked(Mkk.copy(), off, pv)
        return L, sla.solve_triangular(L, np.eye(DB), lower=True)
    W = Mkk.copy()
    X = np.zeros((DB, DB))
    for o in range(0, DB, TILE):
        e = o + TILE
        W[o:, o:e] -= W[o:, :o] @ W[o:e, :o].T                     # (a) left-looking update of the panel
        L16 = _chol_unblocked(W[o:e, o:e].copy(), off + o, pv)      # (b) the 16 x 16 factor and its inverse
        X16 = sla.solve_triangular(L16, np.eye(TILE), lower=True)
        W[o:e, o:e] = L16
        W[e:, o:e] = W[e:, o:e] @ X16.T                             # (c) the tiles below
        X[o:e, o:e] = X16
    L = np.tril(W)
    h = TILE
    while h < DB:                                                   # (d) X by doubling
        for b0 in range(0, DB, 2 * h):
            a, b, c = b0, b0 + h, b0 + 2 * h
            X[b:c, a:b] = -(X[b:c, b:c] @ (L[b:c, a:b] @ X[a:b, a:b]))
        h *= 2
    return L, X


class SchemeModel:
    """Factorisation of M = A A' + delta I (+ diag(extra)) in the stored order `order` (order[p] = the caller's row at stored
    position p; None = identity) by the scheme above.
      L            mpad x mpad lower factor, stored order
      pivots       the pivots the rule tested, stored order (first m entries: the real rows)
      fired_rows   caller's rows whose pivot was replaced, in elimination order
      count        how many (fpsq_*_info.regularized_pivots when a regularisation is set)
      first        1-based caller's row of the first one in stored order, 0 if none (*info without a regularisation)"""

    def __init__(self, A, delta, order=None, tol=0.0, reg=0.0, variant="doubling"):
        assert variant in VARIANTS
        self.sparse = sp.issparse(A)
        self.A = sp.csr_matrix(A) if self.sparse else np.asarray(A, dtype=np.float64)
        self.m, self.n = self.A.shape
        m = self.m
        self.order = np.arange(m) if order is None else np.asarray(order, dtype=np.int64)
        assert np.array_equal(np.sort(self.order), np.arange(m))
        G = self.A @ self.A.T
        G = G.toarray() if self.sparse else G
        G = G + delta * np.eye(m)
        self.nb = (m + DB - 1) // DB
        mpad = self.mpad = self.nb * DB
        W = np.eye(mpad)
        W[:m, :m] = G[np.ix_(self.order, self.order)]
        pv = _Pivots(tol, reg, mpad)
        self.X = []
        for k in range(self.nb):
            a, b = k * DB, (k + 1) * DB
            Lkk, Xk = _diag_block(W[a:b, a:b], a, pv, variant)
            W[a:b, a:b] = Lkk
            self.X.append(Xk)
            if b < mpad:
                W[b:, a:b] = W[b:, a:b] @ Xk.T
                W[b:, b:] -= W[b:, a:b] @ W[b:, a:b].T
        self.L = np.tril(W)
        self.pivots = pv.seen
        fired = [p for p in pv.fired if p < m]
        self.fired_rows = [int(self.order[p]) for p in fired]
        self.count = len(fired)
        self.first = int(self.order[min(fired)]) + 1 if fired else 0

    def factor_in_callers_order(self):
        """L with rows and columns put back in the caller's order (lower triangular only for the identity order)"""
        m = self.m
        out = np.zeros((m, m))
        out[np.ix_(self.order, self.order)] = self.L[:m, :m]
        return out

    def msolve(self, R):
        """M^-1 R for R: (m, k) in the caller's order, by the two sweeps"""
        m, nb = self.m, self.nb
        r = np.zeros((self.mpad, R.shape[1]))
        r[:m] = R[self.order]
        L, X = self.L, self.X
        y = np.zeros_like(r)
        for k in range(nb):
            a, b = k * DB, (k + 1) * DB
            y[a:b] = X[k] @ r[a:b]
            if b < self.mpad:
                r[b:] -= L[b:, a:b] @ y[a:b]
        q = np.zeros_like(r)
        for k in range(nb - 1, -1, -1):
            a, b = k * DB, (k + 1) * DB
            q[a:b] = X[k].T @ y[a:b]
            if a > 0:
                y[:a] -= L[a:b, :a].T @ q[a:b]
        out = np.empty((m, R.shape[1]))
        out[self.order] = q[:m]
        return out

    def solve(self, r1, r2, mixed):
        """(p1, q1, p2, q2) of solve_two_mixed (mixed) or solve_two_least_squares, as the entries form them"""
        A = self.A
        r1, r2 = np.asarray(r1, dtype=np.float64), np.asarray(r2, dtype=np.float64)
        R = np.column_stack([A @ r1, -r2 if mixed else A @ r2])
        Q = self.msolve(R)
        q1, q2 = Q[:, 0].copy(), Q[:, 1].copy()
        p1 = r1 - A.T @ q1
        p2 = -(A.T @ q2) if mixed else r2 - A.T @ q2
        return p1, q1, p2, q2
