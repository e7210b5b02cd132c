"""Test infrastructure: tests/sepquad_ref.py's CPU restatement of the penalty function with the model swapped for
nlpmodels.SepFuncConModel (elementwise function terms, the model behind fpsq_band_nlp_create_fn / DeviceBandSepFuncNLP): the
mirror's exact KKT solve at J(x), the gradient in the -ys form, the mirror's hprod_ as it is.  `kept=True` runs the three solves
on factors that are kept while J and delta stay (lane_group_cases._KeptFactorOracle), which the 8300-row case needs.
Never used by the product."""
import functools

import numpy as np

from fps_amd import nlpmodels, problems
from fps_amd.penalty_nlp import FletcherPenaltyNLP
from lane_group_cases import SIGMA, _KeptFactorOracle, qp
from sepquad_ref import SepQuadRef, _SparseExtrasOracle

CURV = 0.1   # (at 0.3 the case `thin` drops to sigma_min(J) = 0.069: tests/test_band_fn_nlp_cpu.py holds the condition)


class SepFuncRef(SepQuadRef):
    def __init__(self, data, sigma, rho, delta, eta=0.0, xk=None, kept=False):
        self.model = nlpmodels.SepFuncConModel(data)
        qds = (_KeptFactorOracle if kept else _SparseExtrasOracle)(self.model)
        self.pen = FletcherPenaltyNLP(self.model, sigma=sigma, rho=rho, delta=delta, qds=qds)
        self.pen.eta = eta
        if xk is not None:
            self.pen.xk = np.asarray(xk, float)


def fn_codes(nnz, seed=11):
    """the code draw of the lane-group and arrow tests: uniform over the table, a generator of its own"""
    return np.random.default_rng(seed).integers(0, len(problems.FN_TABLE), nnz).astype(np.uint8)


def fn_data_of(eqqp, codes=None):
    """the function model on an EqQP: with_quadratic_constraints(curv = 0.1, seed = 7) values, codes from fn_codes"""
    return problems.with_function_constraints(eqqp, curv=CURV, seed=7,
                                              codes=fn_codes(eqqp.vals.size) if codes is None else codes)


@functools.lru_cache(maxsize=None)
def fn_data(name):
    """the function model of a case of tests/lane_group_cases.py (shared, read-only)"""
    return fn_data_of(qp(name))


@functools.lru_cache(maxsize=None)
def exact_fn(name, delta):
    """SepFuncRef on the case at xk = xhat, rho = eta = 0 (set ref.pen.rho / ref.pen.eta), its solves kept"""
    return SepFuncRef(fn_data(name), SIGMA, 0.0, delta, 0.0, qp(name).xhat, kept=True)
