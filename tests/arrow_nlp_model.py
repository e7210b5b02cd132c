"""The nonlinear model on an arrow band in numpy, fp64: what fpsq_band_nlp_objgrad / _hprod compute on a handle with border
rows and long columns (csrc/fpsq_band_nlp.hip.h), assembled the way the device assembles it, on the arrow scheme of
tests/arrow_model.py at J(x):

  * every M-solve is ArrowModel.msolve (or msolve_fused) on J(x) J(x)' + delta I;
  * J'q takes the rows of the LONG COLUMNS from w_c, the correction's own by-product (the virtual rows of the transposed
    structure), and J'c from U'c;
  * H'q is formed over the other columns, and AT THE LONG COLUMNS separately, from h over each column's own entries in index
    order (k_bn_lc_epilogue, k_bn_lc_epilogue_h1) -- `curvature_at_long_columns=False` leaves those sums out, which is what the
    transposed structure alone would give (th = 0 at the virtual entries).

Formulas: include/fpsq.h fpsq_band_nlp_objgrad / _hprod.  Never used by the product; it carries no fitted constant."""
import numpy as np
import scipy.sparse as sp

from arrow_model import ArrowModel
from fps_amd import nlpmodels


class ArrowNLPModel:
    def __init__(self, data, x, delta, rows, cols, fused=False, curvature_at_long_columns=True):
        self.nlp = nlpmodels.SepQuadConModel(data)
        self.qp, self.x = data.qp, np.asarray(x, float)
        self.J = self.nlp._J(self.x)
        self.arrow = ArrowModel(self.J, delta, rows, cols)
        self.fused, self.at_long = fused, curvature_at_long_columns
        self.cols = np.asarray(cols, dtype=np.int64)
        H = sp.csc_matrix(self.nlp._H)
        H.sort_indices()
        self.Hc = H
        rest = np.ones(self.qp.n, dtype=bool)
        rest[self.cols] = False
        self.Ht_rest = sp.csr_matrix(sp.diags(rest.astype(float)) @ self.nlp._H.T)   # H' with the long columns' rows empty

    def _msolve(self, R):
        return (self.arrow.msolve_fused if self.fused else self.arrow.msolve)(R)

    def jt(self, q, w):
        """J'q, the long columns' rows replaced by w"""
        return self.arrow.at_mul(q, w)

    def jt_keep(self, c):
        """J'c for an operand that is not a solution: the long columns' rows are U'c"""
        return self.jt(c, self.arrow.U.T @ c[self.arrow.order])

    def ht(self, q):
        """H'q; at the long columns summed separately over the column's entries, in index order"""
        out = self.Ht_rest @ q
        if self.at_long:
            for j in self.cols:
                lo, hi = self.Hc.indptr[j], self.Hc.indptr[j + 1]
                s = 0.0
                for t in range(lo, hi):
                    s += self.Hc.data[t] * q[self.Hc.indices[t]]
                out[j] = s
        return out

    def objgrad(self, sigma, rho, eta=0.0, xk=None):
        """dict(fx, gx, ys, gs, c) and the three vectors an hprod runs on (qe, hc, gs)"""
        qp, x = self.qp, self.x
        g = qp.qdiag * x + qp.d
        c = self.nlp.cons(x)
        Q, W = self._msolve(np.column_stack([self.J @ g, -c]))
        q1, q2 = Q[:, 0], Q[:, 1]
        s1, s2, s3 = self.jt(q1, W[:, 0]), self.jt(q2, W[:, 1]), self.jt_keep(c)
        h1, h2, h3 = self.ht(q1), self.ht(q2), self.ht(c)
        gs, p2 = g - s1 - sigma * s2, -s2
        qe = qp.qdiag - (h1 + sigma * h2)
        dx = x - (np.zeros(qp.n) if xk is None else xk) if eta > 0.0 else np.zeros(qp.n)
        ys = q1 + sigma * q2
        gx = gs + (sigma - qe) * p2 + h2 * gs + rho * s3 + eta * dx
        fx = x @ (0.5 * qp.qdiag * x + qp.d) - c @ ys + 0.5 * rho * (c @ c) + 0.5 * eta * (dx @ dx)
        self.qe, self.hc, self.gs = qe, h3, gs
        return {"fx": fx, "gx": gx, "ys": ys, "gs": gs, "c": c}

    def hprod(self, v, sigma, rho, eta, hessian_approx):
        """at the point of the last objgrad"""
        qe, hc, gs = self.qe, self.hc, self.gs
        Jv = self.J @ v
        Q, W = self._msolve(np.column_stack([Jv, self.J @ (qe * v)]))
        s1, s2 = self.jt(Q[:, 0], W[:, 0]), self.jt(Q[:, 1], W[:, 1])
        Hv = (qe * v - s2) - qe * s1 + 2.0 * sigma * s1 + eta * v
        if hessian_approx == 2:
            return Hv + (hc * v + rho * self.jt_keep(Jv) if rho > 0.0 else 0.0)
        Z, Wz = self._msolve(np.column_stack([self.nlp._H @ (gs * v), np.zeros(self.qp.m)]))
        return Hv + rho * (self.jt_keep(Jv) + hc * v) - self.ht(Q[:, 0]) * gs - self.jt(Z[:, 0], Wz[:, 0])
