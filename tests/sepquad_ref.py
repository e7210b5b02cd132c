"""Test infrastructure: the CPU restatement of the penalty function on the separable-quadratic model
(nlpmodels.SepQuadConModel, the model behind fpsq_band_nlp_* / DeviceBandSepQuadNLP), built from the host mirror
FletcherPenaltyNLP with the EXACT oracle as its back-end:
  * `_compute_ys_gs` of the mirror (exact KKT solve at J(x));
  * the gradient in the -ys form -- Hsv = hprod(x, -ys, v), as `hprod!` / `hess_coord!` and the paper's H_sigma have it
    (model-Fletcherpenaltynlp.jl:477, :538, :590) -- which is the gradient of `obj`; `FletcherPenaltyNLP.grad` keeps the
    literal +ys of `grad!` (:382, :415) and is NOT (tests/test_band_nlp_cpu.py measures both);
  * `hprod_` of the mirror as it is, Val(2) and Val(1).
Never used by the product."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from fps_amd import nlpmodels
from fps_amd.penalty_nlp import FletcherPenaltyNLP
from oracle_qdsolver import OracleQDSolver


class _SparseExtrasOracle(OracleQDSolver):
    """OracleQDSolver whose solve_two_extras factorises J J' + tau I as a SPARSE matrix (the oracle's own forms it densely,
    which a 10^4-row grid does not allow); the definition is the same: tau = max(delta, 1e-14),
    (M^-1 J rhs1, M^-1 rhs2) (solve_linear_system.jl:51-72)."""

    def solve_two_extras(self, nlp, x, rhs1, rhs2):
        J = self._jac(nlp, x)
        tau = max(float(nlp.delta), 1e-14)
        lu = spla.splu(sp.csc_matrix(J @ J.T + tau * sp.identity(J.shape[0])))
        return lu.solve(J @ np.asarray(rhs1, float)), lu.solve(np.asarray(rhs2, float))


class SepQuadRef:
    def __init__(self, data, sigma, rho, delta, eta=0.0, xk=None):
        self.model = nlpmodels.SepQuadConModel(data)
        self.pen = FletcherPenaltyNLP(self.model, sigma=sigma, rho=rho, delta=delta, qds=_SparseExtrasOracle(self.model))
        self.pen.eta = eta
        if xk is not None:
            self.pen.xk = np.asarray(xk, float)

    def obj(self, x):
        return self.pen.obj(x)

    def objgrad(self, x):
        """dict(fx, gx, ys, gs, c): gx in the -ys form"""
        pen, nlp = self.pen, self.model
        x = np.asarray(x, float)
        fx = pen.obj(x)
        gs, ys, v, w = (a.copy() for a in pen._compute_ys_gs(x))
        gx = gs - nlp.hprod(x, -ys, v) + pen.sigma * v + nlp.hprod(x, w, gs, obj_weight=0.0)
        if pen.rho > 0.0:
            gx = gx + pen.rho * nlp.jtprod(x, pen.cx)
        if pen.eta > 0.0:
            gx = gx + pen.eta * (x - pen.xk)
        return {"fx": fx, "gx": gx, "ys": ys, "gs": gs, "c": pen.cx.copy()}

    def grad_literal(self, x):
        """FletcherPenaltyNLP.grad: Hsv with +ys, as `grad!` writes it"""
        return self.pen.grad(np.asarray(x, float))

    def hprod(self, x, v, hessian_approx):
        self.pen.hessian_approx = hessian_approx
        return self.pen.hprod(np.asarray(x, float), np.asarray(v, float))
