"""The shapes the coupled quadratic model on bordered and arrow band handles (fpsq_band_nlp_create_coupled_arrow,
DeviceArrowBandCoupledQuadNLP) is tested on, shared by tests/test_band_coupled_arrow_nlp_cpu.py (no GPU) and
tests/test_gpu_band_coupled_arrow_nlp.py.  Test infrastructure, in the manner of tests/coupled_cases.py.

The six shapes of tests/test_gpu_band_arrow_nlp.py under problems.with_coupled_constraints(qp, curv=0.3, pairs=2, seed=7) -- on
an arrow pattern that rule couples the first entry of every row with its last, which is a long column -- and the real model
problems.free_final_time_like(2000).  `counts` below: (terms, terms on a long column, terms between two long columns, terms in
border rows), then the longest row of S; they are asserted by the CPU test.

  case                        counts                    longest   there for
  m640-r3-c5-param            1286 /  643 /    0 /  6       574   three trips of 256; four long columns with empty rows of S
  m640-r16-c16-stride-first   1312 / 1312 /  656 / 32       160   a short long row; a term between two long columns in every row;
                                                                  the long columns at index 0 .. 15
  m1500-r1-c1-shuffled        3002 / 1501 /    0 /  2      1183   the four-entries-per-trip loop, once; a reordered handle
  aug2dc-N51-r2-c16-param     5206 / 2603 /    0 /  4      2601   two chains
  rows-only                   1284 /    0 /    0 /  4         8   terms in border rows alone, no long row
  cols-only                   1280 /  640 /    0 /  0       573   no border
  free-final-time             4000 / 4000 /    0 /  0      4000   the real model: every term on the long column theta, explicit
                                                                  zeros under the terms, separable curvature in the border row
Each case runs at the delta the arrow test gives its shape (free-final-time: sqrt(eps)), (rho, eta) in {(0, 0), (1, 0.5)},
x = qp.x, xk = qp.xhat."""
import functools

import numpy as np

from fps_amd import problems
from test_gpu_band_arrow_nlp import CASES as ARROW_CASES

SE = float(np.sqrt(np.finfo(float).eps))
SIGMA, CURV, PAIRS = 1e3, 0.3, 2
RHO_ETA = ((0.0, 0.0), (1.0, 0.5))
FFT_N = 2000
FFT = "free-final-time"

# name -> (terms, on a long column, both long, in border rows, the longest row of S)
COUNTS = {
    "m640-r3-c5-param": (1286, 643, 0, 6, 574),
    "m640-r16-c16-stride-first": (1312, 1312, 656, 32, 160),
    "m1500-r1-c1-shuffled": (3002, 1501, 0, 2, 1183),
    "aug2dc-N51-r2-c16-param": (5206, 2603, 0, 4, 2601),
    "rows-only": (1284, 0, 0, 4, 8),
    "cols-only": (1280, 640, 0, 0, 573),
    FFT: (2 * FFT_N, 2 * FFT_N, 0, 0, 2 * FFT_N),
}
NAMES = list(COUNTS)


def delta(name):
    return SE if name == FFT else ARROW_CASES[name][1]


def limits(name):
    """(border, cols) the handle is created with"""
    return (16, 16) if name == FFT else ARROW_CASES[name][2]


def want_info(name):
    return {"border_rows": 1, "border_cols": 1, "nblocks": 16} if name == FFT else ARROW_CASES[name][3]


@functools.lru_cache(maxsize=None)
def problem(name):
    """(the CoupledQuadNLP, border rows, long columns) of a case (shared, read-only)"""
    if name == FFT:
        data = problems.free_final_time_like(FFT_N)
        rows, cols = np.array([FFT_N]), np.array([data.qp.n - 1])
    else:
        qp, rows, cols = ARROW_CASES[name][0]()
        data = problems.with_coupled_constraints(qp, curv=CURV, pairs=PAIRS, seed=7)
    for a in (data.hvals, data.b, data.t_row, data.t_j, data.t_k, data.t_w, data.qp.vals, data.qp.x, data.qp.xhat):
        a.setflags(write=False)
    return data, np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)


def v_of(qp):
    return np.random.default_rng(0).standard_normal(qp.n)


def counts(name):
    """COUNTS recomputed from the terms"""
    import scipy.sparse as sp

    d, rows, cols = problem(name)
    lj, lk = np.isin(d.t_j, cols), np.isin(d.t_k, cols)
    one = np.ones(2 * d.nterms)
    S = sp.coo_matrix((one, (np.concatenate([d.t_j, d.t_k]), np.concatenate([d.t_k, d.t_j]))), shape=(d.qp.n, d.qp.n)).tocsr()
    return (d.nterms, int(np.count_nonzero(lj | lk)), int(np.count_nonzero(lj & lk)), int(np.count_nonzero(np.isin(d.t_row, rows))),
            int(np.diff(S.indptr).max()))


def without_special_terms(name):
    """the model without the terms that touch a long column or lie in a border row: what the plain coupled entry could state"""
    d, rows, cols = problem(name)
    keep = ~(np.isin(d.t_j, cols) | np.isin(d.t_k, cols) | np.isin(d.t_row, rows))
    return problems.CoupledQuadNLP(d.qp, d.hvals, d.b, d.t_row[keep], d.t_j[keep], d.t_k[keep], d.t_w[keep])


@functools.lru_cache(maxsize=None)
def expected(name):
    """what the yardstick (tests/coupled_quad_ref.py) says at x = qp.x, xk = qp.xhat: one dict per (rho, eta), computed once and
    left unchanged"""
    from coupled_quad_ref import CoupledQuadRef

    d, _, _ = problem(name)
    qp = d.qp
    ref = CoupledQuadRef(d, SIGMA, 0.0, delta(name), 0.0, qp.xhat, keep_factors=True)
    out = {}
    for rho, eta in RHO_ETA:
        ref.pen.rho, ref.pen.eta = rho, eta
        e = ref.objgrad(qp.x)
        e["Hv2"], e["Hv1"] = ref.hprod(qp.x, v_of(qp), 2), ref.hprod(qp.x, v_of(qp), 1)
        for a in e.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        out[(rho, eta)] = e
    return out
