"""Test infrastructure: the inputs of the tests of elementwise function terms in the OBJECTIVE of the banded nonlinear model
(fpsq_band_nlp_set_objective_terms, problems.with_objective_terms): one draw of weights and code bytes per variable, the
function model of tests/sepfunc_ref.py with those terms on the cases of tests/lane_group_cases.py, and its restatement.  The
restatements (SepQuadRef, SepFuncRef, CoupledRef, ...) build nlpmodels' host classes from the data they are given, and those
classes honour the terms: the yardstick of a model with terms is its EXISTING restatement on data that carries them.
Never used by the product."""
import functools

import numpy as np

from fps_amd import problems
from fps_amd import nlpmodels
from fps_amd.penalty_nlp import FletcherPenaltyNLP
from lane_group_cases import SIGMA, _KeptFactorOracle, qp
from sepfunc_ref import SepFuncRef, fn_data
from sepquad_ref import SepQuadRef

SEED = 13


def terms(n, seed=SEED):
    """(w, codes): codes uniform over the table, |w| in [0.5, 1.5) with a random sign, a quarter of the weights set to 0"""
    r = np.random.default_rng(seed)
    codes = r.integers(0, 6, n).astype(np.uint8)
    w = r.uniform(.5, 1.5, n) * r.choice([-1, 1], n)
    w[r.random(n) < .25] = 0
    return w, codes


def with_terms(data, seed=SEED, always=()):
    """`data` with the draw in its objective; the variables `always` carry a weight whatever the draw says (1.25 where it drew 0)"""
    w, codes = terms(data.qp.n, seed)
    always = np.asarray(always, dtype=np.int64)
    w[always] = np.where(w[always] == 0.0, 1.25, w[always])
    return problems.with_objective_terms(data, w, codes)


class SepQuadKeptRef(SepQuadRef):
    """SepQuadRef with its three solves on LUs that are kept while J and delta stay (lane_group_cases._KeptFactorOracle: the
    same definitions), as SepFuncRef(kept=True) and CoupledQuadRef(keep_factors=True) have them"""

    def __init__(self, data, sigma, rho, delta, eta=0.0, xk=None):
        self.model = nlpmodels.SepQuadConModel(data)
        self.pen = FletcherPenaltyNLP(self.model, sigma=sigma, rho=rho, delta=delta, qds=_KeptFactorOracle(self.model))
        self.pen.eta = eta
        if xk is not None:
            self.pen.xk = np.asarray(xk, float)


@functools.lru_cache(maxsize=None)
def objfn_data(name):
    """the function model of a lane-group case with the draw above in its objective (shared, read-only)"""
    return with_terms(fn_data(name))


@functools.lru_cache(maxsize=None)
def exact_objfn(name, delta):
    """SepFuncRef on it at xk = xhat, rho = eta = 0 (set ref.pen.rho / ref.pen.eta), its solves kept"""
    return SepFuncRef(objfn_data(name), SIGMA, 0.0, delta, 0.0, qp(name).xhat, kept=True)
