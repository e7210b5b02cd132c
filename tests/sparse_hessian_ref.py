"""Test infrastructure: the exact penalty evaluations on an eq-QP with a sparse symmetric objective Hessian, in scipy alone --
independent of the library and of oracle/ (whose exact_qp_* helpers know diag(q) only).

K = [I A'; A -delta I] is factorised once per (qp, delta) with SuperLU; with Q = qp.hess_csr()
  objgrad (model-Fletcherpenaltynlp.jl:403-437):  g = Q x + d, c = A x - b, K [p1; q1] = [g; 0], K [p2; q2] = [0; c],
      ys = q1 + sigma q2, gs = p1 + sigma p2, gx = gs - Q p2 + sigma p2 + rho A'c + eta (x - xk),
      fx = f - c'ys + rho/2 c'c + eta/2 |x - xk|^2;
  hprod Val(2) (:521-570):  K [p1; .] = [v; 0], K [p2; .] = [Q v; 0], Ptv = v - p1,
      Hv = p2 - Q Ptv + 2 sigma Ptv + rho A'(A v) + eta v."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


class SparseHessianRef:
    def __init__(self, qp, delta):
        self.qp, self.n, self.m = qp, qp.n, qp.m
        self.A = qp.scipy_csr()
        self.Q = qp.hess_csr()
        K = sp.bmat([[sp.identity(qp.n), self.A.T], [self.A, -float(delta) * sp.identity(qp.m)]], format="csc")
        self._lu = spla.splu(K)

    def _solve(self, top, bottom):
        sol = self._lu.solve(np.concatenate([top, bottom]))
        return sol[:self.n], sol[self.n:]

    def objgrad(self, x, sigma, rho, eta=0.0, xk=None):
        qp, A, Q = self.qp, self.A, self.Q
        g = Q @ x + qp.d
        f = float(x @ (0.5 * (Q @ x) + qp.d))
        c = A @ x - qp.b
        p1, q1 = self._solve(g, np.zeros(self.m))
        p2, q2 = self._solve(np.zeros(self.n), c)
        ys, gs = q1 + sigma * q2, p1 + sigma * p2
        gx = gs - Q @ p2 + sigma * p2
        fx = f - c @ ys
        if rho > 0:
            gx = gx + rho * (A.T @ c)
            fx += rho / 2 * (c @ c)
        if eta > 0:
            dx = x - (np.zeros_like(x) if xk is None else xk)
            gx = gx + eta * dx
            fx += eta / 2 * (dx @ dx)
        return dict(fx=fx, gx=gx, ys=ys, gs=gs)

    def hprod(self, v, sigma, rho, eta=0.0):
        A, Q = self.A, self.Q
        p1, _ = self._solve(v, np.zeros(self.m))
        p2, _ = self._solve(Q @ v, np.zeros(self.m))
        ptv = v - p1
        Hv = p2 - Q @ ptv + 2.0 * sigma * ptv
        if rho > 0:
            Hv = Hv + rho * (A.T @ (A @ v))
        if eta > 0:
            Hv = Hv + eta * v
        return Hv

    def kkt_point(self):
        """(x*, lambda*) of the QP itself: [Q A'; A 0] [x; lambda] = [-d; b]"""
        K = sp.bmat([[self.Q, self.A.T], [self.A, None]], format="csc")
        sol = spla.splu(K).solve(np.concatenate([-self.qp.d, self.qp.b]))
        return sol[:self.n], sol[self.n:]
