"""Test infrastructure: the CPU restatement of the penalty function on the COUPLED quadratic model
(nlpmodels.CoupledQuadConModel, the model behind fpsq_band_nlp_create_coupled / DeviceBandCoupledQuadNLP).  It is
tests/sepquad_ref.py on that model and nothing else: the host mirror FletcherPenaltyNLP with the EXACT oracle as its back-end,
  * `_compute_ys_gs` of the mirror (exact KKT solve at J(x));
  * the gradient in the -ys form, Hsv = hprod(x, -ys, v) -- the gradient of `obj` (tests/test_band_coupled_nlp_cpu.py measures
    it and the literal +ys form of `grad!`);
  * `hprod_` of the mirror as it is, Val(2) and Val(1).
`keep_factors=True` runs the three solves on LUs that are kept while J and delta stay (lane_group_cases._KeptFactorOracle: the
same definitions), which the larger GPU cases need.  Never used by the product."""
import numpy as np

from fps_amd import nlpmodels
from fps_amd.penalty_nlp import FletcherPenaltyNLP
from sepquad_ref import SepQuadRef, _SparseExtrasOracle


class CoupledQuadRef(SepQuadRef):
    def __init__(self, data, sigma, rho, delta, eta=0.0, xk=None, keep_factors=False):
        self.model = nlpmodels.CoupledQuadConModel(data)
        if keep_factors:
            from lane_group_cases import _KeptFactorOracle

            qds = _KeptFactorOracle(self.model)
        else:
            qds = _SparseExtrasOracle(self.model)
        self.pen = FletcherPenaltyNLP(self.model, sigma=sigma, rho=rho, delta=delta, qds=qds)
        self.pen.eta = eta
        if xk is not None:
            self.pen.xk = np.asarray(xk, float)
