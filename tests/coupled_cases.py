"""The shapes the coupled quadratic model (fpsq_band_nlp_create_coupled, DeviceBandCoupledQuadNLP) is tested on, shared by
tests/test_band_coupled_nlp_cpu.py (no GPU: the couplings must matter on each of them) and tests/test_gpu_band_coupled_nlp.py.
Test infrastructure, in the manner of tests/lane_group_cases.py.

  case               shape                                                     there for
  small              pde_control_like(n=4000, m=400, per_row=16, window=512)   m is not a multiple of 128
  row-shuffled       the rows of small in a random order                       the reordered handle: the terms' rows go through
                                                                               the permutation
  aug2dc             aug2dc_like(N=100)                                        two chains; two or three entries per row; rows with
                                                                               one term (the four corner rows have two entries)
  m-multiple-of-128  pde_control_like(n=6000, m=640, per_row=24, window=512)   m a multiple of 128
  bilinear           bilinear_control_like(N=2000)                             the real model: h = 0, an explicit zero of A under
                                                                               every term, one term per row
  sparse-terms       small, terms on every third row only                      rows and entries with empty lists; variables with
                                                                               an empty row of S
  hub                pde_control_like(n=600, m=500, per_row=40, window=160),   one long row of S (the hub's: the 284 columns its
                     8 terms per row, and the column with the most rows        rows touch) among rows of 8 on average: lgR = 8
                     coupled to every other entry of each of its rows          lanes per row of S, 36 trips of the group on the
                                                                               hub's row; entries of S with several contributors
                                                                               (6635 terms on 4956 entries); lgA = lgT = 32
  stride             bilinear_control_like(N=360000)                           the second trip of every grid-stride loop of the new
                                                                               kernels (see STRIDE below)

PAIRS = 2 terms per row and CURV = 0.3 (tests/test_gpu_band_nlp.py's curvature) unless the case says otherwise.

STRIDE.  n = 720001, m = 360000, nnz = 1080000, lgA = 2, lgT = 1, lgR = 1: the row kernels walk 2813 (rows of A, 128 a tile) and
2813 (rows of A' and of S, 256 a tile) tiles against kBqMaxGrid = 2048, and the per-entry kernels 4219 (k_bcn_vals, 256 entries a
workgroup) against 4096; k_bcn_assemble's 2813 workgroups stay under 4096: its second trip takes nnz(S) > 1048576, which with
one term per row would be N > 524288, and which a dense term rule reaches at n = 2048 -- the case assemble-stride of
tests/coupled_lane_cases.py (tests/test_gpu_coupled_lane_groups.py)."""
import dataclasses
import functools

import numpy as np

from fps_amd import problems

SE = float(np.sqrt(np.finfo(float).eps))
SIGMA, CURV, PAIRS = 1e3, 0.3, 2


def shuffled(qp, seed):
    """`_shuffled` of tests/test_gpu_band_nlp.py: the same QP with its constraint rows in a random order"""
    import scipy.sparse as sp

    perm = np.random.default_rng(seed).permutation(qp.m)
    A = sp.csr_matrix(qp.scipy_csr()[perm])
    A.sort_indices()
    return dataclasses.replace(qp, rowptr=A.indptr.astype(np.int32), colind=A.indices.astype(np.int32), vals=A.data.copy(),
                               b=qp.b[perm])


def small_qp():
    return problems.pde_control_like(n=4000, m=400, per_row=16, window=512, seed=21)


def with_hub(qp, curv, pairs, seed):
    """with_coupled_constraints(qp, curv, pairs, seed) plus: the column that lies in the most rows (the first such) is coupled,
    in each of those rows, to every other entry of the row it is not coupled to yet; weights by the same rule from
    default_rng(seed + 1)"""
    base = problems.with_coupled_constraints(qp, curv, pairs, seed)
    hub = int(np.argmax(np.bincount(qp.colind, minlength=qp.n)))
    rng = np.random.default_rng(seed + 1)
    have = {(int(r), min(int(j), int(k)), max(int(j), int(k))) for r, j, k in zip(base.t_row, base.t_j, base.t_k)}
    t_row, t_k, t_w = [], [], []
    for i in range(qp.m):
        lo, hi = qp.rowptr[i], qp.rowptr[i + 1]
        cols = qp.colind[lo:hi]
        if hub not in cols:
            continue
        ah = qp.vals[lo + int(np.flatnonzero(cols == hub)[0])]
        for e in range(lo, hi):
            c = int(qp.colind[e])
            if c != hub and (i, min(c, hub), max(c, hub)) not in have:
                t_row.append(i), t_k.append(c)
                t_w.append(curv * np.sqrt(abs(ah * qp.vals[e])) * rng.uniform(0.5, 1.5) * rng.choice([-1.0, 1.0]))
    cat = lambda a, b: np.concatenate([a, np.asarray(b, dtype=a.dtype)])  # noqa: E731
    return hub, problems._coupled(qp, base.hvals, cat(base.t_row, t_row), cat(base.t_j, np.full(len(t_row), hub)),
                                  cat(base.t_k, t_k), cat(base.t_w, t_w))


def _coupled(qp, **kw):
    return problems.with_coupled_constraints(qp, curv=CURV, pairs=PAIRS, seed=7, **kw)


# name -> (the model, what DeviceBandCoupledQuadNLP.info() must say about the handle)
CASES = {
    "small": (lambda: _coupled(small_qp()), {}),
    "row-shuffled": (lambda: _coupled(shuffled(small_qp(), 5)), {"reordered": 1}),
    "aug2dc": (lambda: _coupled(problems.aug2dc_like(N=100)), {"chains": 2}),
    "m-multiple-of-128": (lambda: _coupled(problems.pde_control_like(n=6000, m=640, per_row=24, window=512, seed=5)), {}),
    "bilinear": (lambda: problems.bilinear_control_like(N=2000), {}),
    "sparse-terms": (lambda: _coupled(small_qp(), rows=np.arange(0, 400, 3)), {}),
    "hub": (lambda: with_hub(problems.pde_control_like(n=600, m=500, per_row=40, window=160, seed=33), CURV, 8, 7)[1], {}),
}
STRIDE_N = 360000


@functools.lru_cache(maxsize=None)
def data(name):
    """the CoupledQuadNLP of a case (shared, read-only)"""
    out = problems.bilinear_control_like(N=STRIDE_N) if name == "stride" else CASES[name][0]()
    for a in (out.hvals, out.b, out.t_row, out.t_j, out.t_k, out.t_w, out.qp.vals, out.qp.x, out.qp.xhat):
        a.setflags(write=False)
    return out


def without_terms(d):
    """the separable model on the same data: what dropping the terms leaves"""
    return problems.SepQuadNLP(d.qp, d.hvals, d.b)


def s_pattern(d):
    """(rows of S with an entry, nnz(S), the longest row of S) from the terms alone"""
    import scipy.sparse as sp

    one = np.ones(2 * d.nterms)
    S = sp.coo_matrix((one, (np.concatenate([d.t_j, d.t_k]), np.concatenate([d.t_k, d.t_j]))), shape=(d.qp.n, d.qp.n)).tocsr()
    lens = np.diff(S.indptr)
    return int(np.count_nonzero(lens)), int(S.nnz), int(lens.max())
