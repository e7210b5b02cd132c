"""Synthetic equality-constrained QP workloads (BASELINE.json `configs`).

The reference publishes no data for its hot path, only sizes; these generators are this build's
specification of them.  Every random number comes from a counter-based generator
``u(seed, i, k) = splitmix64(seed ^ i*GOLDEN ^ k*C2) / 2**64`` so any language can reproduce the same bits.

User model (what FletcherPenaltyNLP wraps, model-Fletcherpenaltynlp.jl:105-188):
    f(x) = 1/2 x' Q x + d' x,     c(x) = A x - b = 0,     Q = diag(q) unless the QP carries a sparse symmetric Hessian
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass
from typing import Optional

import numpy as np

_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_C2 = np.uint64(0xD1B54A32D192ED03)


def splitmix64(z: np.ndarray) -> np.ndarray:
    z = z.astype(np.uint64, copy=True)
    with np.errstate(over="ignore"):
        z += _GOLDEN
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def uniform01(seed: int, i, k) -> np.ndarray:
    """u(seed, i, k) in [0, 1); i and k broadcast."""
    i = np.asarray(i, dtype=np.uint64)
    k = np.asarray(k, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed) ^ (i * _GOLDEN) ^ (k * _C2)
    return (splitmix64(z) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


@dataclass
class EqQP:
    """Equality-constrained QP with a CSR Jacobian (0-based int32 indices, fp64 values)."""

    name: str
    n: int
    m: int
    rowptr: np.ndarray
    colind: np.ndarray
    vals: np.ndarray
    qdiag: np.ndarray
    d: np.ndarray
    b: np.ndarray
    x: np.ndarray  # evaluation point (infeasible)
    xhat: np.ndarray  # a feasible point, b = A xhat
    # the objective Hessian Q when it is not diagonal: n x n CSR, 0-based int32, FULL symmetric storage (both triangles);
    # None = diag(qdiag).  With a sparse Q, qdiag holds its diagonal.
    hess_rowptr: Optional[np.ndarray] = None
    hess_colind: Optional[np.ndarray] = None
    hess_vals: Optional[np.ndarray] = None

    @property
    def nnz(self) -> int:
        return int(self.vals.size)

    @property
    def has_sparse_hessian(self) -> bool:
        return self.hess_vals is not None

    def hess_csr(self):
        """Q as a scipy CSR matrix, whichever way the QP stores it."""
        import scipy.sparse as sp

        if self.hess_vals is None:
            return sp.diags(self.qdiag, format="csr")
        return sp.csr_matrix((self.hess_vals, self.hess_colind, self.hess_rowptr), shape=(self.n, self.n))

    def scipy_csr(self):
        import scipy.sparse as sp

        return sp.csr_matrix((self.vals, self.colind, self.rowptr), shape=(self.m, self.n))

    def point(self, t: int) -> np.ndarray:
        """t-th distinct evaluation point (a line-search never evaluates the same x twice,
        which is what defeats the hash(x) memo of model-Fletcherpenaltynlp.jl:235-237)."""
        idx = np.arange(self.n)
        return self.xhat + 0.1 * (2.0 * uniform01(977 + t, idx, 5) - 1.0)


def _finish(name, n, m, rowptr, colind, vals, seed) -> EqQP:
    import scipy.sparse as sp

    idx = np.arange(n)
    qdiag = 1.0 + 9.0 * uniform01(seed, idx, 1)
    d = 2.0 * uniform01(seed, idx, 2) - 1.0
    xhat = 2.0 * uniform01(seed, idx, 3) - 1.0
    A = sp.csr_matrix((vals, colind, rowptr), shape=(m, n))
    b = A @ xhat
    x = xhat + 0.1 * (2.0 * uniform01(seed, idx, 4) - 1.0)
    return EqQP(name, n, m, rowptr.astype(np.int32), colind.astype(np.int32), vals, qdiag, d, b, x, xhat)


def with_sparse_hessian(qp: EqQP, half_width: int = 2, seed: int = 4321) -> EqQP:
    """A copy of `qp` whose objective Hessian is sparse, symmetric and banded -- the shape of a mass or stiffness matrix:
    Q[i, j] = Q[j, i] = 2 u(seed, i * half_width + (j - i - 1), 21) - 1 for 0 < j - i <= half_width, except that every row
    i with i % 7 == 3 has NO off-diagonal entry (its column neither), and Q[i, i] = 1 + 9 u(seed, i, 22) + sum_j |Q[i, j]|:
    strictly diagonally dominant with a positive diagonal, hence positive definite.  `qdiag` holds the diagonal of Q."""
    import scipy.sparse as sp

    n, hw = qp.n, int(half_width)
    assert hw >= 1
    i = np.repeat(np.arange(n, dtype=np.int64), hw)
    k = np.tile(np.arange(hw, dtype=np.int64), n)
    j = i + k + 1
    keep = (j < n) & (i % 7 != 3) & (j % 7 != 3)
    i, j, k = i[keep], j[keep], k[keep]
    v = 2.0 * uniform01(seed, i * hw + k, 21) - 1.0
    absrow = np.bincount(i, np.abs(v), n) + np.bincount(j, np.abs(v), n)
    idx = np.arange(n, dtype=np.int64)
    diag = 1.0 + 9.0 * uniform01(seed, idx, 22) + absrow
    Q = sp.coo_matrix((np.concatenate([v, v, diag]), (np.concatenate([i, j, idx]), np.concatenate([j, i, idx]))),
                      shape=(n, n)).tocsr()
    Q.sort_indices()
    return dataclasses.replace(qp, name=f"{qp.name}-hess{hw}", qdiag=diag, hess_rowptr=Q.indptr.astype(np.int32),
                               hess_colind=Q.indices.astype(np.int32), hess_vals=Q.data.astype(np.float64))


def with_border_rows(qp: EqQP, s: int, kind: str = "mean", seed: int = 0) -> EqQP:
    """A copy of `qp` with `s` LONG constraint rows appended (rows m .. m + s - 1) and `b` extended by A xhat on them, so
    xhat stays feasible.  Long rows couple with every other row of A A': the case of the bordered band
    (include/fpsq.h "BORDERED BAND").
      kind = "mean":     row r touches every 16th column, r % 16, r % 16 + 16, ... -- a weighted mean over a stride of the
                         variables; values (0.5 + u(seed, entry, 31)) / sqrt(entries of the row), entry = r * n + column.
      kind = "periodic": row r couples the FIRST and the LAST columns, 4 r .. 4 r + 3 and n - 1 - (4 r .. 4 r + 3) -- the
                         wrap-around rows of a periodic boundary; values 2 u(seed, entry, 32) - 1, + 2 on the first (needs
                         n >= 8 s)."""
    s = int(s)
    assert s >= 1
    n = qp.n
    cols, vals = [], []
    for r in range(s):
        if kind == "mean":
            c = np.arange(r % 16, n, 16, dtype=np.int64)
            v = (0.5 + uniform01(seed, r * n + c, 31)) / np.sqrt(c.size)
        elif kind == "periodic":
            assert n >= 8 * s
            k = 4 * r + np.arange(4, dtype=np.int64)
            c = np.concatenate([k, (n - 1 - k)[::-1]])
            v = 2.0 * uniform01(seed, r * n + c, 32) - 1.0
            v[0] += 2.0
        else:
            raise ValueError(f"kind must be 'mean' or 'periodic', not {kind!r}")
        cols.append(c)
        vals.append(v)
    counts = np.array([c.size for c in cols], dtype=np.int64)
    cols, vals = np.concatenate(cols), np.concatenate(vals)
    rowptr = np.concatenate([qp.rowptr.astype(np.int64), qp.rowptr[-1] + np.cumsum(counts)])
    b_new = np.array([np.dot(vals[lo:hi], qp.xhat[cols[lo:hi]])
                      for lo, hi in zip(np.cumsum(counts) - counts, np.cumsum(counts))])
    return dataclasses.replace(qp, name=f"{qp.name}+{s}{kind}", m=qp.m + s, rowptr=rowptr.astype(np.int32),
                               colind=np.concatenate([qp.colind, cols]).astype(np.int32),
                               vals=np.concatenate([qp.vals, vals]), b=np.concatenate([qp.b, b_new]))


def with_long_columns(qp: EqQP, s: int, kind: str = "param", seed: int = 0) -> EqQP:
    """A copy of `qp` with `s` LONG columns appended (variables n .. n + s - 1): variables that appear in constraints all over
    the row range, the case of include/fpsq.h "LONG COLUMNS".
      kind = "param":  column j touches every row -- a global parameter, a free final time;
      kind = "stride": column j touches the rows r with r % 4 == j % 4 -- a control shared by every fourth constraint.
    Values (0.5 + u(seed, j * m + r, 41)) / sqrt(rows the column touches).  qdiag, d, xhat and x are extended by the streams
    `_finish` uses, at index n + j, and b = A xhat is recomputed, so xhat stays feasible.  The QP must have a diagonal Hessian
    (apply `with_sparse_hessian` afterwards for a sparse one)."""
    import scipy.sparse as sp

    s = int(s)
    assert s >= 1 and qp.hess_vals is None
    n, m = qp.n, qp.m
    rows, cols, vals = [], [], []
    for j in range(s):
        if kind == "param":
            r = np.arange(m, dtype=np.int64)
        elif kind == "stride":
            r = np.arange(j % 4, m, 4, dtype=np.int64)
        else:
            raise ValueError(f"kind must be 'param' or 'stride', not {kind!r}")
        rows.append(r)
        cols.append(np.full(r.size, n + j, dtype=np.int64))
        vals.append((0.5 + uniform01(seed, j * m + r, 41)) / np.sqrt(r.size))
    rows0 = np.repeat(np.arange(m, dtype=np.int64), np.diff(qp.rowptr))
    A = sp.csr_matrix((np.concatenate([qp.vals] + vals), (np.concatenate([rows0] + rows),
                                                          np.concatenate([qp.colind.astype(np.int64)] + cols))),
                      shape=(m, n + s))   # (disjoint patterns: nothing is summed, the appended columns end each row)
    A.sort_indices()
    idx = n + np.arange(s)
    xhat = np.concatenate([qp.xhat, 2.0 * uniform01(seed, idx, 3) - 1.0])
    return dataclasses.replace(
        qp, name=f"{qp.name}+{s}{kind}cols", n=n + s, rowptr=A.indptr.astype(np.int32), colind=A.indices.astype(np.int32),
        vals=A.data.astype(np.float64), qdiag=np.concatenate([qp.qdiag, 1.0 + 9.0 * uniform01(seed, idx, 1)]),
        d=np.concatenate([qp.d, 2.0 * uniform01(seed, idx, 2) - 1.0]), xhat=xhat, b=A @ xhat,
        x=np.concatenate([qp.x, xhat[n:] + 0.1 * (2.0 * uniform01(seed, idx, 4) - 1.0)]))


def with_arrow(qp: EqQP, s_rows: int, s_cols: int, row_kind: str = "mean", col_kind: str = "param", seed: int = 0) -> EqQP:
    """A copy of `qp` with `s_rows` long rows AND `s_cols` long columns: `with_long_columns(with_border_rows(qp, ...), ...)`, so
    the columns reach the border rows too (U_s != 0) -- the case of include/fpsq.h "ARROW BAND".  xhat stays feasible."""
    return with_long_columns(with_border_rows(qp, s_rows, kind=row_kind, seed=seed), s_cols, kind=col_kind, seed=seed)


@dataclass
class SepQuadNLP:
    """A QP objective with separable-quadratic equality constraints on the pattern of the QP's Jacobian:
    c_i(x) = sum_j (A_ij + 1/2 H_ij x_j) x_j - b_i, so J(x)_ij = A_ij + H_ij x_j (nlpmodels.SepQuadConModel,
    include/fpsq.h fpsq_band_nlp_*).  `qp` holds the objective, A (rowptr / colind / vals), x and xhat; its own b is that of
    the LINEAR constraints and is not used."""

    qp: EqQP
    hvals: np.ndarray  # H in the CSR order of qp.vals
    b: np.ndarray      # right-hand side, c(xhat) = 0


def with_quadratic_constraints(qp: EqQP, curv: float = 0.1, seed: int = 0) -> SepQuadNLP:
    """`qp` with curvature in every constraint: hvals = curv * vals * U(0.5, 1.5) * (+-1) (numpy's default_rng(seed), one draw
    of each per entry) and b = A xhat + 1/2 H (xhat .* xhat), so that xhat stays feasible.  The QP must have a diagonal
    Hessian."""
    import scipy.sparse as sp

    assert qp.hess_vals is None
    rng = np.random.default_rng(seed)
    hvals = curv * qp.vals * rng.uniform(0.5, 1.5, qp.vals.size) * rng.choice([-1.0, 1.0], qp.vals.size)
    H = sp.csr_matrix((hvals, qp.colind, qp.rowptr), shape=(qp.m, qp.n))
    b = qp.scipy_csr() @ qp.xhat + 0.5 * (H @ (qp.xhat * qp.xhat))
    return SepQuadNLP(qp, np.ascontiguousarray(hvals, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64))


# the function table of include/fpsq.h (FPSQ_FN_*): code -> (phi, phi', phi'') as numpy callables
FN_HALFSQ, FN_CUBE6, FN_SIN, FN_COS, FN_EXP, FN_TANH = range(6)
FN_TABLE = (
    (lambda x: 0.5 * x * x, lambda x: x, lambda x: np.ones_like(x)),
    (lambda x: x * x * x / 6.0, lambda x: 0.5 * x * x, lambda x: x),
    (np.sin, np.cos, lambda x: -np.sin(x)),
    (np.cos, lambda x: -np.sin(x), lambda x: -np.cos(x)),
    (np.exp, np.exp, np.exp),
    (np.tanh, lambda x: 1.0 - np.tanh(x) ** 2, lambda x: -2.0 * np.tanh(x) * (1.0 - np.tanh(x) ** 2)),
)


def fn_apply(codes: np.ndarray, x: np.ndarray, order: int) -> np.ndarray:
    """the order-th derivative (0, 1, 2) of phi_codes[k] at x[k], entry by entry"""
    x = np.asarray(x, float)
    out = np.empty_like(x)
    for c, fns in enumerate(FN_TABLE):
        sel = codes == c
        if sel.any():
            out[sel] = fns[order](x[sel])
    return out


@dataclass
class SepFuncNLP(SepQuadNLP):
    """A SepQuadNLP whose curvature entries carry a FUNCTION each: c_i(x) = sum_j (A_ij x_j + H_ij phi_kij(x_j)) - b_i with
    phi from FN_TABLE by the code byte of the entry (code 0, 1/2 x^2, is SepQuadNLP's term), so J(x)_ij = A_ij + H_ij phi'(x_j)
    keeps the pattern (nlpmodels.SepFuncConModel, include/fpsq.h fpsq_band_nlp_create_fn)."""

    codes: np.ndarray = None  # uint8, in the CSR order of qp.vals


def _sepfunc(qp, hvals, codes) -> SepFuncNLP:
    """the model with b set so that xhat is feasible"""
    import scipy.sparse as sp

    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    assert codes.shape == qp.vals.shape and (codes.size == 0 or int(codes.max()) < len(FN_TABLE))
    H = sp.csr_matrix((hvals * fn_apply(codes, qp.xhat[qp.colind], 0), qp.colind, qp.rowptr), shape=(qp.m, qp.n))
    b = qp.scipy_csr() @ qp.xhat + np.asarray(H.sum(axis=1)).ravel()
    return SepFuncNLP(qp, np.ascontiguousarray(hvals, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64), codes)


def with_function_constraints(qp: EqQP, curv: float = 0.1, seed: int = 0, codes=None) -> SepFuncNLP:
    """`with_quadratic_constraints(qp, curv, seed)` (the same draw of hvals) with a function code on every entry: uniform over
    the table from numpy's default_rng(seed) (a generator of its own, so the hvals do not move) unless `codes` is given.  b is
    set so that xhat stays feasible."""
    hvals = with_quadratic_constraints(qp, curv, seed).hvals
    if codes is None:
        codes = np.random.default_rng(seed).integers(0, len(FN_TABLE), qp.vals.size)
    return _sepfunc(qp, hvals, codes)


def pendulum_like(N=2000, tau=0.05, alpha=0.1, seed=1234) -> SepFuncNLP:
    """A controlled pendulum theta'' = -sin theta + u by explicit Euler steps of length tau: (theta_k, omega_k, u_k)
    interleaved for k = 0 .. N - 1, then the final (theta_N, omega_N): n = 3 N + 2, m = 2 N, a band of width 5.  Rows
        2k:      theta_{k+1} - theta_k - tau omega_k = 0,
        2k + 1:  omega_{k+1} - omega_k + tau sin theta_k - tau u_k = 0;
    the sine sits on the entry (2k + 1, theta_k) with A_ij = 0 stored EXPLICITLY, H_ij = tau and code FN_SIN; every other entry
    has H_ij = 0 and code 0.  xhat is the trajectory simulated from theta_0 = 0.3, omega_0 = 0 under u_k = 1/2 sin(0.1 k), so it
    is feasible with b = 0 up to rounding (b is set from it all the same).  Objective: q = 1 on the states, alpha on the
    controls, d = -1/2 q .* xhat.  x = xhat + 0.1 (2u - 1) from the counter-based generator."""
    n, m = 3 * N + 2, 2 * N
    k = np.arange(N, dtype=np.int64)
    th, om, u = 3 * k, 3 * k + 1, 3 * k + 2
    # row 2k: (theta_k, omega_k, theta_{k+1}); row 2k + 1: (theta_k, omega_k, u_k, omega_{k+1})
    rowptr = np.concatenate([[0], np.cumsum(np.tile([3, 4], N))]).astype(np.int64)
    colind = np.stack([th, om, th + 3, th, om, u, om + 3], axis=1).ravel()
    vals = np.tile(np.array([-1.0, -tau, 1.0, 0.0, -1.0, -tau, 1.0]), N)
    hvals = np.tile(np.array([0.0, 0.0, 0.0, tau, 0.0, 0.0, 0.0]), N)
    codes = np.tile(np.array([0, 0, 0, FN_SIN, 0, 0, 0], dtype=np.uint8), N)
    xhat = np.zeros(n)
    theta, omega = 0.3, 0.0
    for i in range(N):
        ui = 0.5 * np.sin(0.1 * i)
        xhat[3 * i: 3 * i + 3] = theta, omega, ui
        theta, omega = theta + tau * omega, omega - tau * np.sin(theta) + tau * ui
    xhat[3 * N:] = theta, omega
    idx = np.arange(n, dtype=np.int64)
    ctrl = (idx % 3 == 2) & (idx < 3 * N)
    qdiag = np.where(ctrl, alpha, 1.0)
    d = -0.5 * qdiag * xhat
    x = xhat + 0.1 * (2.0 * uniform01(seed, idx, 4) - 1.0)
    qp = EqQP(f"pendulum-N{N}", n, m, rowptr.astype(np.int32), colind.astype(np.int32), vals, qdiag, d, np.zeros(m), x,
              xhat)   # (qp.b is the LINEAR constraints' and is not used)
    return _sepfunc(qp, hvals, codes)


def with_objective_terms(data, w, codes=None):
    """A copy of a SepQuadNLP, SepFuncNLP or CoupledQuadNLP with ELEMENTWISE FUNCTION TERMS IN THE OBJECTIVE:
    f(x) = 1/2 x' diag(q) x + d'x + sum_j w_j psi_kj(x_j), psi from FN_TABLE by one code byte per VARIABLE (`codes`, default
    every code 0); an entry with w_j = 0 contributes nothing and is not evaluated.  The copy carries `obj_w` (float64, n) and
    `obj_codes` (uint8, n) (nlpmodels' host classes and DeviceBandSepQuadNLP honour them; include/fpsq.h
    fpsq_band_nlp_set_objective_terms); without this function the attributes are absent.  The constraints, b among them, stay."""
    import copy

    n = data.qp.n
    w = np.ascontiguousarray(w, dtype=np.float64)
    codes = np.zeros(n, dtype=np.uint8) if codes is None else np.ascontiguousarray(codes, dtype=np.uint8)
    assert w.shape == (n,) and codes.shape == (n,)
    assert not np.any(codes[w != 0.0] >= len(FN_TABLE)), "a function code outside the table under a weight that is not 0"
    out = copy.copy(data)
    out.obj_w, out.obj_codes = w, codes
    return out


def objective_terms(data, x, order):
    """w_j times the order-th derivative (0, 1, 2) of psi_kj at x_j for the terms of `with_objective_terms`, entry by entry
    (0 where w_j = 0, whatever x_j), or None when `data` carries none"""
    w = getattr(data, "obj_w", None)
    if w is None:
        return None
    x = np.asarray(x, float)
    out = np.zeros_like(x)
    on = w != 0.0
    if on.any():
        out[on] = w[on] * fn_apply(data.obj_codes[on], x[on], order)
    return out


def pendulum_energy_like(N=2000, beta=0.5, gamma=0.05, **kwargs) -> SepFuncNLP:
    """`pendulum_like(N)` with the potential energy -beta cos theta_k on every theta (k = 0 .. N) and the control cost
    gamma exp(u_k) on every control in the objective: a problem whose objective is no diagonal QP."""
    data = pendulum_like(N, **kwargs)
    n = data.qp.n
    idx = np.arange(n)
    w, codes = np.zeros(n), np.zeros(n, dtype=np.uint8)
    theta, ctrl = idx % 3 == 0, (idx % 3 == 2) & (idx < 3 * N)
    w[theta], codes[theta] = -beta, FN_COS
    w[ctrl], codes[ctrl] = gamma, FN_EXP
    return with_objective_terms(data, w, codes)


@dataclass
class CoupledQuadNLP(SepQuadNLP):
    """A SepQuadNLP plus coupling terms t = (t_row, t_j, t_k, t_w), each adding t_w x_tj x_tk to c_trow (0-based, t_j != t_k):
    c_i(x) = sum_j (A_ij + 1/2 H_ij x_j) x_j + sum_{t in i} w_t x_jt x_kt - b_i.  Both columns of a term are entries of its row of
    A (an explicit zero where need be), so J(x) keeps the pattern (nlpmodels.CoupledQuadConModel, include/fpsq.h
    fpsq_band_nlp_create_coupled)."""

    t_row: np.ndarray = None  # int32
    t_j: np.ndarray = None    # int32
    t_k: np.ndarray = None    # int32
    t_w: np.ndarray = None    # float64

    @property
    def nterms(self) -> int:
        return int(self.t_w.size)


def _coupled(qp, hvals, t_row, t_j, t_k, t_w) -> CoupledQuadNLP:
    """the model with b set so that xhat is feasible"""
    import scipy.sparse as sp

    xh = qp.xhat
    H = sp.csr_matrix((hvals, qp.colind, qp.rowptr), shape=(qp.m, qp.n))
    b = qp.scipy_csr() @ xh + 0.5 * (H @ (xh * xh)) + np.bincount(t_row, t_w * xh[t_j] * xh[t_k], qp.m)
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
    return CoupledQuadNLP(qp, f64(hvals), f64(b), i32(t_row), i32(t_j), i32(t_k), f64(t_w))


def with_coupled_constraints(qp: EqQP, curv: float = 0.1, pairs: int = 2, seed: int = 0, rows=None) -> CoupledQuadNLP:
    """`with_quadratic_constraints(qp, curv, seed)` (the same draw of hvals) plus up to `pairs` coupling terms per row, between
    columns of that row.  A row with entries e_0 < ... < e_{L-1} has the candidates, in this order: its first `pairs` - 1
    neighbouring pairs (e_0, e_1), (e_1, e_2), ..., then (e_0, e_{L-1}) when L > 2, then the remaining neighbouring pairs; the
    first `pairs` of them are taken (a row of one entry has none).  Weights: curv sqrt|a_j a_k| U(0.5, 1.5) (+-1), drawn after
    the hvals from the same generator, one of each per term in row order.  `rows` (a boolean mask or an index array, default
    all) restricts the rows that get terms.  b is set so that xhat stays feasible."""
    sep = with_quadratic_constraints(qp, curv, seed)
    rng = np.random.default_rng(seed)
    rng.uniform(0.5, 1.5, qp.vals.size), rng.choice([-1.0, 1.0], qp.vals.size)  # (the draws of the hvals)
    take = np.zeros(qp.m, dtype=bool)
    take[np.arange(qp.m) if rows is None else rows] = True
    t_row, e_j, e_k = [], [], []
    for i in np.flatnonzero(take):
        lo, L = int(qp.rowptr[i]), int(qp.rowptr[i + 1] - qp.rowptr[i])
        nb = [(u, u + 1) for u in range(L - 1)]
        cand = nb[:max(pairs - 1, 0)] + ([(0, L - 1)] if L > 2 else []) + nb[max(pairs - 1, 0):]
        for u, v in cand[:pairs]:
            t_row.append(i), e_j.append(lo + u), e_k.append(lo + v)
    t_row, e_j, e_k = (np.asarray(a, dtype=np.int64) for a in (t_row, e_j, e_k))
    t_w = (curv * np.sqrt(np.abs(qp.vals[e_j] * qp.vals[e_k])) * rng.uniform(0.5, 1.5, t_row.size)
           * rng.choice([-1.0, 1.0], t_row.size))
    return _coupled(qp, sep.hvals, t_row, qp.colind[e_j], qp.colind[e_k], t_w)


def bilinear_control_like(N=2000, tau=0.25, alpha=0.1, seed=1234) -> CoupledQuadNLP:
    """Bilinear control of y' = -y + u y + s by explicit Euler steps of length tau: states y_0 .. y_N, controls
    u_0 .. u_{N-1}, interleaved x = (y_0, u_0, y_1, u_1, ..., y_N) (n = 2 N + 1, a band of width 3), rows k = 0 .. N - 1
        y_{k+1} - y_k + tau y_k - tau u_k y_k = b_k,
    objective 1/2 sum (y - yhat)^2 + alpha/2 sum u^2 (up to its constant): q = 1 on the states, alpha on the controls,
    d = -yhat on the states.  Three entries per row -- (k, y_k) = tau - 1, (k, u_k) = 0 stored EXPLICITLY so that the term lies on
    the pattern, (k, y_{k+1}) = 1 -- no separable curvature, and one coupling term (k, y_k, u_k, -tau) per row.  yhat = 1 +
    0.5 sin(2 pi k / N); xhat: states 1 + 0.3 (2u - 1), controls 0.5 (2u - 1) from the counter-based generator; b (the source
    s) makes xhat feasible; x = xhat + 0.1 (2u - 1)."""
    n, m = 2 * N + 1, N
    k = np.arange(N, dtype=np.int64)
    rowptr = 3 * np.arange(m + 1, dtype=np.int64)
    colind = np.stack([2 * k, 2 * k + 1, 2 * k + 2], axis=1).ravel()
    vals = np.tile(np.array([tau - 1.0, 0.0, 1.0]), N)
    idx = np.arange(n, dtype=np.int64)
    state = idx % 2 == 0
    qdiag = np.where(state, 1.0, alpha)
    yhat = 1.0 + 0.5 * np.sin(2.0 * np.pi * (idx // 2) / N)
    d = np.where(state, -yhat, 0.0)
    xhat = np.where(state, 1.0 + 0.3 * (2.0 * uniform01(seed, idx, 3) - 1.0), 0.5 * (2.0 * uniform01(seed, idx, 3) - 1.0))
    x = xhat + 0.1 * (2.0 * uniform01(seed, idx, 4) - 1.0)
    qp = EqQP(f"bilinear-control-N{N}", n, m, rowptr.astype(np.int32), colind.astype(np.int32), vals, qdiag, d,
              np.zeros(m), x, xhat)   # (qp.b is the LINEAR constraints' and is not used)
    return _coupled(qp, np.zeros_like(vals), k, 2 * k, 2 * k + 1, np.full(N, -float(tau)))


def free_final_time_like(N=2000, tau=0.25, a=1.0, beta=1.0, alpha=0.1, gamma=1.0, theta_hat=1.0, seed=1234) -> CoupledQuadNLP:
    """Control of y' = -theta (a y - beta u) + s over a horizon whose length theta is a VARIABLE (a free final time scaled to
    N explicit Euler steps of length tau theta): states y_0 .. y_N and controls u_0 .. u_{N-1} interleaved, then theta,
    x = (y_0, u_0, y_1, u_1, ..., y_N, theta) (n = 2 N + 2), rows k = 0 .. N - 1
        y_{k+1} - y_k + tau theta (a y_k - beta u_k) = b_k,
    and one LONG ROW N, the mean control energy sum_k u_k^2 / (2 N) = b_N (m = N + 1).  theta multiplies the dynamics: row k has
    the two coupling terms (k, y_k, theta, tau a) and (k, u_k, theta, -tau beta), whose second column is a LONG COLUMN, and four
    entries -- (k, y_k) = -1, (k, y_{k+1}) = 1 and the EXPLICIT ZEROS (k, u_k), (k, theta) under the terms.  Row N has the N
    entries (N, u_k) = 0 with the separable curvature h = 1 / N, so a border row carries curvature.  Objective
    1/2 sum (y - yhat)^2 + alpha/2 sum u^2 + gamma/2 (theta - theta_hat)^2 (up to its constant).  yhat, the states and controls
    of xhat and x as in bilinear_control_like; theta of xhat is theta_hat (1 + 0.1 (2u - 1)); b makes xhat feasible."""
    n, m = 2 * N + 2, N + 1
    th = n - 1
    k = np.arange(N, dtype=np.int64)
    rowptr = np.concatenate([4 * np.arange(N + 1, dtype=np.int64), [5 * N]])
    colind = np.concatenate([np.stack([2 * k, 2 * k + 1, 2 * k + 2, np.full(N, th)], axis=1).ravel(), 2 * k + 1])
    vals = np.concatenate([np.tile(np.array([-1.0, 0.0, 1.0, 0.0]), N), np.zeros(N)])
    hvals = np.concatenate([np.zeros(4 * N), np.full(N, 1.0 / N)])
    idx = np.arange(n, dtype=np.int64)
    state = (idx % 2 == 0) & (idx < th)
    ctrl = (idx % 2 == 1) & (idx < th)
    qdiag = np.where(state, 1.0, np.where(ctrl, alpha, gamma))
    yhat = 1.0 + 0.5 * np.sin(2.0 * np.pi * (idx // 2) / N)
    d = np.where(state, -yhat, np.where(ctrl, 0.0, -gamma * theta_hat))
    u3, u4 = 2.0 * uniform01(seed, idx, 3) - 1.0, 2.0 * uniform01(seed, idx, 4) - 1.0
    xhat = np.where(state, 1.0 + 0.3 * u3, np.where(ctrl, 0.5 * u3, theta_hat * (1.0 + 0.1 * u3)))
    x = xhat + 0.1 * u4
    qp = EqQP(f"free-final-time-N{N}", n, m, rowptr.astype(np.int32), colind.astype(np.int32), vals, qdiag, d, np.zeros(m), x,
              xhat)   # (qp.b is the LINEAR constraints' and is not used)
    return _coupled(qp, hvals, np.concatenate([k, k]), np.concatenate([2 * k, 2 * k + 1]), np.full(2 * N, th),
                    np.concatenate([np.full(N, tau * a), np.full(N, -tau * beta)]))


def _stratified_rows(m, n, per_row, start, width, seed, diag_col=None, diag_boost=0.0):
    """Each of the m rows gets `per_row` sorted, distinct columns: one per stratum of
    [start[i], start[i] + width).  If diag_col is given, the stratum containing diag_col[i] is
    placed exactly there and its value gets +diag_boost."""
    rows = np.repeat(np.arange(m, dtype=np.int64), per_row)
    ks = np.tile(np.arange(per_row, dtype=np.int64), m)
    lo = (ks * width) // per_row
    hi = ((ks + 1) * width) // per_row
    eid = rows * per_row + ks
    off = lo + np.floor(uniform01(seed, eid, 11) * (hi - lo)).astype(np.int64)
    vals = 2.0 * uniform01(seed, eid, 12) - 1.0
    cols = np.repeat(start, per_row) + off
    if diag_col is not None:
        rel = np.repeat(diag_col - start, per_row)
        hit = (rel >= lo) & (rel < hi)
        cols = np.where(hit, np.repeat(diag_col, per_row), cols)
        vals = np.where(hit, vals + diag_boost, vals)
    assert cols.min() >= 0 and cols.max() < n
    rowptr = np.arange(m + 1, dtype=np.int64) * per_row
    return rowptr, cols, vals


def random_eqqp(n=100_000, m=10_000, per_row=100, seed=1234) -> EqQP:
    """configs[1]: random sparse eq-QP; every row has `per_row` nonzeros spread over all n columns."""
    start = np.zeros(m, dtype=np.int64)
    rowptr, cols, vals = _stratified_rows(m, n, per_row, start, n, seed)
    return _finish(f"random-eqqp-n{n}-m{m}", n, m, rowptr, cols, vals, seed)


def pde_control_like(n=1_000_000, m=100_000, per_row=100, window=8192, seed=1234) -> EqQP:
    """configs[4] / the headline: row i has `per_row` nonzeros in a column window of width `window`
    centred at floor(i n / m) (clamped), and A[i, floor(i n / m)] carries an extra +4."""
    window = min(window, n)
    center = (np.arange(m, dtype=np.int64) * n) // m
    start = np.clip(center - window // 2, 0, n - window)
    rowptr, cols, vals = _stratified_rows(m, n, per_row, start, window, seed, diag_col=center, diag_boost=4.0)
    return _finish(f"pde-control-like-n{n}-m{m}", n, m, rowptr, cols, vals, seed)


def _hashed_rows(m, n, per_row, start, width, seed, diag_col, diag_boost):
    """SURVEY.md 8(d) as written: row i has `per_row` DISTINCT columns start[i] + off, the offsets hashed over the whole
    window, off = floor(u(seed, entry, 11 + 16 a) * width) with a = 0 and a re-draw (a + 1, a + 2, ...) of every entry that
    collides with an EARLIER entry of its row; entry 0 of a row is its centre column diag_col[i] (value + diag_boost), so a row
    has exactly per_row entries.  Columns sorted within a row; values 2u - 1 by entry."""
    per = per_row
    eid = np.arange(m, dtype=np.int64)[:, None] * per + np.arange(per, dtype=np.int64)[None, :]
    off = np.floor(uniform01(seed, eid, 11) * width).astype(np.int64)
    off[:, 0] = diag_col - start
    attempt = np.zeros((m, per), dtype=np.int64)
    for _ in range(64):
        order = np.argsort(off, axis=1, kind="stable")          # equal offsets keep their entry order
        so = np.take_along_axis(off, order, axis=1)
        dup_sorted = np.zeros((m, per), dtype=bool)
        dup_sorted[:, 1:] = so[:, 1:] == so[:, :-1]              # every entry but the earliest of a run of equal offsets
        if not dup_sorted.any():
            break
        dup = np.zeros((m, per), dtype=bool)
        np.put_along_axis(dup, order, dup_sorted, axis=1)
        attempt[dup] += 1
        off[dup] = np.floor(uniform01(seed, eid[dup], 11 + 16 * attempt[dup]) * width).astype(np.int64)
    else:
        raise RuntimeError("hashed offsets: collisions left after 64 re-draws")
    vals = 2.0 * uniform01(seed, eid, 12) - 1.0
    vals[:, 0] += diag_boost
    cols = start[:, None] + off
    order = np.argsort(cols, axis=1, kind="stable")
    cols = np.take_along_axis(cols, order, axis=1)
    vals = np.take_along_axis(vals, order, axis=1)
    assert cols.min() >= 0 and cols.max() < n and np.all(cols[:, 1:] > cols[:, :-1])
    return np.arange(m + 1, dtype=np.int64) * per, cols.ravel(), vals.ravel()


def pde_control_hashed(n=1_000_000, m=100_000, per_row=100, window=8192, seed=1234) -> EqQP:
    """The headline shape with SURVEY.md 8(d)'s LITERAL column rule: row i has `per_row` nonzeros at distinct HASHED offsets
    of a column window of width `window` centred at floor(i n / m) (clamped), re-drawn on collision, values 2u - 1, and
    A[i, floor(i n / m)] carries an extra +4.  `pde_control_like` (the bench headline since round 1) draws one column per
    equal slice of the window instead -- a more regular gather pattern; this variant shows what the layouts do without that
    regularity (bench.py --workload "pde-control-hashed ...", profiles/r04_configs.md)."""
    window = min(window, n)
    center = (np.arange(m, dtype=np.int64) * n) // m
    start = np.clip(center - window // 2, 0, n - window)
    rowptr, cols, vals = _hashed_rows(m, n, per_row, start, window, seed, center, 4.0)
    return _finish(f"pde-control-hashed-n{n}-m{m}", n, m, rowptr, cols, vals, seed)


def aug2dc_like(N=100, seed=1234) -> EqQP:
    """configs[3] stand-in ("AUG2DC-like", restated from the published description; CUTEst/SIF is not
    available offline, so this is NOT SIF-verified): variables = edges of an N x N grid graph with a
    boundary ring (n = 2N(N+1)), constraints = nodes (m = N^2), A = signed node-edge incidence."""
    m = N * N
    node = lambda i, j: i * N + j
    rows, cols, vals = [], [], []
    e = 0
    # horizontal edges: (i, j-1) -> (i, j) for j = 0..N  (j = 0 and j = N touch one node only)
    for i in range(N):
        for j in range(N + 1):
            if j > 0:
                rows.append(node(i, j - 1)); cols.append(e); vals.append(-1.0)
            if j < N:
                rows.append(node(i, j)); cols.append(e); vals.append(1.0)
            e += 1
    for j in range(N):
        for i in range(N + 1):
            if i > 0:
                rows.append(node(i - 1, j)); cols.append(e); vals.append(-1.0)
            if i < N:
                rows.append(node(i, j)); cols.append(e); vals.append(1.0)
            e += 1
    n = e
    import scipy.sparse as sp

    A = sp.csr_matrix((vals, (rows, cols)), shape=(m, n))
    A.sort_indices()
    return _finish(f"aug2dc-like-N{N}", n, m, A.indptr.astype(np.int64), A.indices.astype(np.int64),
                   A.data.astype(np.float64), seed)


def dense_block(n=4096, m=2048, seed=1234) -> EqQP:
    """configs[2]: dense Jacobian A[i, j] = (2u - 1)/sqrt(n), stored as CSR with every entry present."""
    eid = np.arange(m * n, dtype=np.int64)
    vals = (2.0 * uniform01(seed, eid, 12) - 1.0) / np.sqrt(n)
    rowptr = np.arange(m + 1, dtype=np.int64) * n
    cols = np.tile(np.arange(n, dtype=np.int64), m)
    return _finish(f"dense-block-n{n}-m{m}", n, m, rowptr, cols, vals, seed)
