"""Host-side mirror of the reference's QDSolver plug-in seam, backed by libfpsq (MI355X).

Reference: src/solve_two_systems_struct.jl:16 (`abstract type QDSolver`), the three generic functions
`solve_two_extras` / `solve_two_least_squares` / `solve_two_mixed` (src/solve_linear_system.jl:9,25,43) and the
constructor contract `QDS(nlp, ::T; explicit_linear_constraints = false, kwargs...)` (struct.jl:94-98, call site
src/parameters.jl:299).  Same names, same argument meaning, same error behaviour (numerical failure only warns).
"""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np

from . import _lib


class QDSolver:
    """Abstract back-end for the two systems [I A'; A -delta I] (struct.jl:1-16)."""

    def solve_two_extras(self, nlp, x, rhs1, rhs2):
        raise NotImplementedError

    def solve_two_least_squares(self, nlp, x, rhs1, rhs2):
        raise NotImplementedError

    def solve_two_mixed(self, nlp, x, rhs1, rhs2):
        raise NotImplementedError



def _coord_values(vals):
    """The output of jac_coord! as the library takes it: a contiguous fp64 array on the host, or a torch CUDA tensor
    (a device-resident model: the values never leave HBM; its producer stream is synchronised first, the direct back-ends
    read on their own stream)."""
    if getattr(vals, "is_cuda", False):
        import torch

        vals = vals.contiguous()
        assert vals.dtype == torch.float64
        torch.cuda.current_stream(vals.device).synchronize()
        return vals
    return np.ascontiguousarray(vals, dtype=np.float64)

REG_DROP = 1e200  # include/fpsq.h FPSQ_REG_DROP: a vanishing pivot of M is dropped (its multiplier comes out as zero)


def _ldlt_r2(ldlt_r2):
    """`ldlt_r2` of `LDLtSolver` (src/solve_two_systems_struct.jl:314): the reference's default -sqrt(eps) when omitted;
    "drop" (or any value <= -REG_DROP) asks for the drop rule of include/fpsq.h instead."""
    if ldlt_r2 is None:
        return -float(np.sqrt(np.finfo(float).eps))
    if isinstance(ldlt_r2, str):
        if ldlt_r2 != "drop":
            raise ValueError('ldlt_r2: a number or "drop"')
        return -REG_DROP
    return float(ldlt_r2)

class FpsqError(RuntimeError):
    pass


class HIPQDSolver(QDSolver):
    """`HIPQDSolver(nlp, T(0); kwargs...)`: the MI355X back-end.  Keyword names are those of `IterativeSolver`
    (struct.jl:99-115): ls_atol, ls_rtol, ls_itmax, ln_atol, ln_rtol, ln_btol, ln_conlim, ln_itmax, ne_atol, ne_rtol,
    ne_etol, ne_itmax, ne_conlim; unknown keywords are swallowed like the reference's `kwargs...`."""

    def __init__(self, nlp, _zero=0.0, *, explicit_linear_constraints=False, **kwargs):
        if explicit_linear_constraints:  # the systems then involve the NONLINEAR constraints only (struct.jl:101-103,333)
            from .nlpmodels import NonlinearConstraintsView
            nlp = NonlinearConstraintsView(nlp)
        self.explicit_linear_constraints = bool(explicit_linear_constraints)
        self._lib = _lib.load()
        self.nvar, self.ncon = int(nlp.meta.nvar), int(nlp.meta.ncon)
        opts = _lib.Options()
        self._lib.fpsq_default_options(self.nvar, self.ncon, C.byref(opts))
        names = {f for f, _ in _lib.Options._fields_}
        for k, v in kwargs.items():
            if k in names:
                setattr(opts, k, v)
        self.opts = opts
        h = C.c_void_p()
        rc = self._lib.fpsq_create(C.byref(h), self.nvar, self.ncon, C.byref(opts))
        if rc != 0:
            raise FpsqError(self._lib.fpsq_last_error(None).decode())
        self._h = h
        # structure once, like LDLtSolver's jac_structure! (struct.jl:331-337); COO, 1-based like NLPModels
        rows, cols = nlp.jac_structure()
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        cols = np.ascontiguousarray(cols, dtype=np.int64)
        self._check(self._lib.fpsq_set_jacobian_structure_coo(h, rows.size, rows.ctypes.data, cols.ctypes.data, 1))
        self._delta = None
        self.stats = (_lib.Stats * 2)()

    # -- plumbing
    def _check(self, rc):
        if rc < 0:
            raise FpsqError(self._lib.fpsq_last_error(self._h).decode())
        return rc

    def close(self):
        if getattr(self, "_h", None):
            self._lib.fpsq_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _refresh(self, nlp, x, values=True):
        if values:
            vals = np.ascontiguousarray(nlp.pen.jac_coord(x), dtype=np.float64)  # jac_coord! / jac_nln_coord! (:223-228)
            self._check(self._lib.fpsq_set_jacobian_values(self._h, vals.ctypes.data))
        if self._delta != nlp.delta:
            self._check(self._lib.fpsq_set_delta(self._h, float(nlp.delta)))
            self._delta = nlp.delta

    # -- the seam
    def solve_two_mixed(self, nlp, x, rhs1, rhs2):
        """p1, q1, p2, q2 = solve_two_mixed(nlp, x, rhs1, rhs2)   (src/solve_linear_system.jl:107-140)"""
        self._refresh(nlp, x)  # the reference rebuilds nlp.Aop at x here (:118-122)
        n, m = self.nvar, self.ncon
        rhs1 = np.ascontiguousarray(rhs1, dtype=np.float64)
        rhs2 = np.ascontiguousarray(rhs2, dtype=np.float64)
        p1, q1, p2, q2 = np.empty(n), np.empty(m), np.empty(n), np.empty(m)
        rc = self._check(self._lib.fpsq_solve_two_mixed(self._h, rhs1.ctypes.data, rhs2.ctypes.data, p1.ctypes.data,
                                                        q1.ctypes.data, p2.ctypes.data, q2.ctypes.data, self.stats))
        if rc & 1:
            warnings.warn("Failed solving 1st linear system lsqr in mixed.")
        if rc & 2:
            warnings.warn("Failed solving 2nd linear system craig in mixed.")
        return p1, q1, p2, q2

    def solve_two_least_squares(self, nlp, x, rhs1, rhs2):
        """p1, q1, p2, q2 = solve_two_least_squares(nlp, x, rhs1, rhs2)   (:79-105; Aop is NOT refreshed, :85-86)"""
        self._refresh(nlp, x, values=False)
        n, m = self.nvar, self.ncon
        rhs1 = np.ascontiguousarray(rhs1, dtype=np.float64)
        rhs2 = np.ascontiguousarray(rhs2, dtype=np.float64)
        p1, q1, p2, q2 = np.empty(n), np.empty(m), np.empty(n), np.empty(m)
        rc = self._check(self._lib.fpsq_solve_two_least_squares(self._h, rhs1.ctypes.data, rhs2.ctypes.data,
                                                                p1.ctypes.data, q1.ctypes.data, p2.ctypes.data,
                                                                q2.ctypes.data, self.stats))
        if rc & 1:
            warnings.warn("Failed solving 1st linear system lsqr.")
        if rc & 2:
            warnings.warn("Failed solving 2nd linear system lsqr.")
        return p1, q1, p2, q2

    def solve_two_extras(self, nlp, x, rhs1, rhs2):
        """invJtJJv, invJtJSsv = solve_two_extras(nlp, x, rhs1, rhs2)   (:45-77)"""
        self._refresh(nlp, x, values=False)
        m = self.ncon
        rhs1 = np.ascontiguousarray(rhs1, dtype=np.float64)
        rhs2 = np.ascontiguousarray(rhs2, dtype=np.float64)
        o1, o2 = np.empty(m), np.empty(m)
        rc = self._check(self._lib.fpsq_solve_two_extras(self._h, rhs1.ctypes.data, rhs2.ctypes.data, o1.ctypes.data,
                                                         o2.ctypes.data, self.stats))
        if rc & 1:
            warnings.warn("Failed solving 1st linear system lsqr in extra.")
        if rc & 2:
            warnings.warn("Failed solving 2nd linear system minres in extra.")
        return o1, o2

    def info(self):
        i = _lib.Info()
        self._check(self._lib.fpsq_get_info(self._h, C.byref(i)))
        return i.as_dict()


# src/parameters.jl:197 -- the registry fps_solve(...; qds_solver = :sym) looks back-ends up in
qdsolver_correspondence = {"hip": HIPQDSolver}


class _DirectQDSolver(QDSolver):
    """What the two direct back-ends share: the constructor contract of `LDLtSolver`, the solves on the cached factor and the
    lazy restore of the delta factor.  A back-end supplies `_prefix` (its entry points are fpsq_<prefix>_*), `_Info`,
    `_create(rows, cols, device)` (sets the handle `_h` up with the COO structure; raises FpsqError) and
    `_hand_over(vals, delta, info)` (values to the device and factorisation; returns the library's code)."""

    def __init__(self, nlp, _zero=0.0, *, explicit_linear_constraints=False, ldlt_tol=None, ldlt_r1=None, ldlt_r2=None,
                 **kwargs):
        if explicit_linear_constraints:
            from .nlpmodels import NonlinearConstraintsView
            nlp = NonlinearConstraintsView(nlp)
        self.explicit_linear_constraints = bool(explicit_linear_constraints)
        self._lib = _lib.load()
        self.nvar, self.ncon = int(nlp.meta.nvar), int(nlp.meta.ncon)
        # jac_structure! once (struct.jl:331-337), in the model's COO order (1-based, duplicates allowed): the library sorts it
        # and keeps the order on the device; per x only the output of jac_coord! crosses the boundary (host or device memory)
        rows, cols = nlp.jac_structure()
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        cols = np.ascontiguousarray(cols, dtype=np.int64)
        self._create(rows, cols, int(kwargs.get("device", 0)))
        self.factorized = False
        se = float(np.sqrt(np.finfo(float).eps))
        self.ldlt_tol = se if ldlt_tol is None else float(ldlt_tol)        # struct.jl:312
        self.ldlt_r2 = _ldlt_r2(ldlt_r2)                                   # struct.jl:314: -sqrt(eps) unless given ("drop": see HIPDirectQDSolver)
        self._check(self._fn("set_regularization")(self._h, self.ldlt_tol, -self.ldlt_r2))
        self._fact_key = None
        self._owed = self._mixed_at = None

    def _fn(self, name):
        return getattr(self._lib, f"fpsq_{self._prefix}_{name}")

    def _check(self, rc):
        if rc < 0:
            raise FpsqError(self._fn("last_error")(self._h).decode())
        return rc

    def close(self):
        if getattr(self, "_h", None):
            self._fn("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _factorize(self, nlp, x, delta=None):
        delta = float(nlp.delta if delta is None else delta)
        vals = _coord_values(nlp.pen.jac_coord(x))                                     # linear_system.jl:223-228
        rc = self._hand_over(vals, delta, C.c_int32())
        self.factorized = rc == 0
        self._fact_key = (np.asarray(x, dtype=np.float64).tobytes(), delta) if rc == 0 else None
        return rc

    def _solve(self, name, rhs1, rhs2):
        n, m = self.nvar, self.ncon
        rhs1 = np.ascontiguousarray(rhs1, dtype=np.float64)
        rhs2 = np.ascontiguousarray(rhs2, dtype=np.float64)
        p1, q1, p2, q2 = np.zeros(n), np.zeros(m), np.zeros(n), np.zeros(m)
        if not self.factorized:
            warnings.warn("_solve_ldlt_factorization: failed _factorization")
            return p1, q1, p2, q2
        self._check(self._fn(name)(self._h, rhs1.ctypes.data, rhs2.ctypes.data, p1.ctypes.data, q1.ctypes.data,
                                   p2.ctypes.data, q2.ctypes.data))
        return p1, q1, p2, q2

    def solve_two_mixed(self, nlp, x, rhs1, rhs2):
        self._factorize(nlp, x)
        self._owed, self._mixed_at = None, (np.array(x, dtype=np.float64), float(nlp.delta))
        return self._solve("solve_two_mixed", rhs1, rhs2)

    def solve_two_least_squares(self, nlp, x, rhs1, rhs2):
        self._restore_factor(nlp)
        return self._solve("solve_two_least_squares", rhs1, rhs2)

    def _restore_factor(self, nlp):
        """solve_two_extras may have left the factor of A A' + tau I (tau != delta) in the handle; the reference's extras never
        touch its LDL' factors, so `solve_two_least_squares` must find the factor of delta at the x of the last
        `solve_two_mixed` (linear_system.jl:194-195).  Put back LAZILY: only when such a solve actually comes (an hprod!
        Val(1) then pays one extra factorisation, not two)."""
        if self._owed is not None:
            x, delta = self._owed
            self._owed = None
            self._factorize(nlp, x, delta)

    def solve_two_extras(self, nlp, x, rhs1, rhs2):
        """invJtJJv = (AA' + tau I)^-1 A rhs1, invJtJSsv = (AA' + tau I)^-1 rhs2 (src/solve_linear_system.jl:142-159).
        The reference's LDL' back-end runs `cgls` / `minres` on the operator with tau = max(delta, 1e-14); here both
        come out of a Cholesky factor of AA' + tau I at x (q1 and -q2 of a mixed solve): like the reference this
        variant looks at the Jacobian at x itself (:148-152), so the factor is rebuilt unless the cached one belongs to
        exactly this x and tau."""
        tau = max(float(nlp.delta), 1e-14)                                            # :148
        if self._fact_key != (np.asarray(x, dtype=np.float64).tobytes(), tau):
            if tau != float(nlp.delta) and self._owed is None and self._mixed_at is not None:
                self._owed = self._mixed_at  # (the factor a later solve_two_least_squares is entitled to: restored lazily)
            self._factorize(nlp, x, tau)
        _, q1, _, q2 = self._solve("solve_two_mixed", rhs1, rhs2)
        return q1, -q2

    def info(self):
        i = self._Info()
        self._check(self._fn("get_info")(self._h, C.byref(i)))
        return i.as_dict()


class HIPDirectQDSolver(_DirectQDSolver):
    """`HIPDirectQDSolver(nlp, T(0))`: the DIRECT back-end on the MI355X for small / dense Jacobians -- the role
    `LDLtSolver` plays in the reference (src/solve_two_systems_struct.jl:299-353; it is the reference's default,
    src/parameters.jl:290).  Instead of an LDL' of K it factorises the normal equations M = A A' + delta I (fp64 MFMA
    SYRK + blocked Cholesky) and solves both systems with two right-hand sides; like `ldl_factorize!` it refactorises
    on every `solve_two_mixed` (src/solve_linear_system.jl:233-234) and re-uses the factors in
    `solve_two_least_squares` (:194-195).  A non positive definite M only warns (:244-246).
    Keywords of `LDLtSolver` (struct.jl:308-316): ldlt_tol (sqrt(eps)) and ldlt_r2 drive the DYNAMIC REGULARISATION of
    the factorisation; ldlt_r1 concerns the identity block of K, whose pivots are 1 and never regularised.  A pivot of M
    not above ldlt_tol marks a constraint row that depends linearly on the earlier ones at working precision.
    * ldlt_r2 (default -sqrt(eps), the reference's `LDLtSolver` default, struct.jl:314): the pivot is replaced by -ldlt_r2 --
      the value LDLFactorizations.jl puts in the (2,2) block of K.
    * ldlt_r2 = "drop" (or -REG_DROP): the pivot is DROPPED instead (FPSQ_REG_DROP = 1e200: that row's multiplier comes out
      as zero, the basic solution of the consistent normal equations).  An OPTION, not the default: the reference's
      -sqrt(eps) acts on pivots of K in a fill-reducing order (on FLT, test/test-2.jl:264-287, AMD eliminates both
      constraint nodes first, which amounts to the uniform shift M + sqrt(eps) I); the same number on a pivot of M in
      natural order is not the same rule, and either way the multiplier estimates grow like 1 / sqrt(eps) on an
      inconsistent right-hand side (phi ~ 1e10 at FLT's x0: a Newton-CG sub-solver crawls).  Dropping keeps them bounded
      like the exact back-end's minimum-norm solve.
    Dense storage: m <= 65536."""

    _prefix, _Info = "dense", _lib.DenseInfo

    def _create(self, rows, cols, device):
        d = C.c_void_p()
        if self._lib.fpsq_dense_create(C.byref(d), self.nvar, self.ncon, device) != 0:
            raise FpsqError(self._lib.fpsq_dense_last_error(None).decode())
        self._h = d
        self._check(self._lib.fpsq_dense_set_structure_coo(d, rows.size, rows.ctypes.data, cols.ctypes.data, 1))

    def _hand_over(self, vals, delta, info):
        self._check(self._lib.fpsq_dense_set_jacobian_coo(self._h, _lib.ptr(vals)))
        return self._check(self._lib.fpsq_dense_factorize(self._h, delta, C.byref(info)))


qdsolver_correspondence["hip_direct"] = HIPDirectQDSolver


class HIPBandedDirectQDSolver(_DirectQDSolver):
    """`HIPBandedDirectQDSolver(nlp, T(0))`: the DIRECT back-end for SPARSE Jacobians whose normal-equations matrix is
    banded (PDE-like models) -- `LDLtSolver`'s role at sizes where a dense M does not fit (include/fpsq.h, fpsq_band_*).
    The constructor is the symbolic phase (struct.jl:326-344), `solve_two_mixed` refactorises at x
    (solve_linear_system.jl:223-234), `solve_two_least_squares` re-uses the factor (:194-195); ldlt_tol / ldlt_r2 as in
    HIPDirectQDSolver.  border (0 .. 16): at most that many long constraint rows -- rows that couple with every other row
    of M, such as a mean-value constraint -- are eliminated last as a border instead of widening the band
    (include/fpsq.h "BORDERED BAND"); `info()["border_rows"]` says how many were taken.  cols (0 .. 16): the same for long
    COLUMNS, such as a global parameter (include/fpsq.h "LONG COLUMNS"; `info()["border_cols"]`); one kind per handle."""

    _prefix, _Info = "band", _lib.BandInfo

    def __init__(self, nlp, _zero=0.0, *, border=0, cols=0, **kwargs):
        self.border = int(border)
        self.cols = int(cols)
        super().__init__(nlp, _zero, **kwargs)

    def _create(self, rows, cols, device):
        b = C.c_void_p()
        rc = self._lib.fpsq_band_create_coo_bordered_cols(C.byref(b), self.nvar, self.ncon, rows.size, rows.ctypes.data,
                                                          cols.ctypes.data, 1, self.border, self.cols, device)
        if rc != 0:
            raise FpsqError(self._lib.fpsq_band_last_error(None).decode())
        self._h = b

    def _hand_over(self, vals, delta, info):
        return self._check(self._lib.fpsq_band_factorize_coo(self._h, _lib.ptr(vals), delta, C.byref(info)))


qdsolver_correspondence["hip_ldlt"] = HIPBandedDirectQDSolver


class HIPArrowBandedDirectQDSolver(HIPBandedDirectQDSolver):
    """HIPBandedDirectQDSolver with border rows AND long columns on one handle (include/fpsq.h "ARROW BAND"): at most `border`
    long constraint rows and at most `cols` long columns, both 0 .. 16, independently; `info()["border_rows"]` and
    `info()["border_cols"]` say what was taken."""

    def __init__(self, nlp, _zero=0.0, *, border=16, cols=16, **kwargs):
        super().__init__(nlp, _zero, border=border, cols=cols, **kwargs)

    def _create(self, rows, cols, device):
        b = C.c_void_p()
        rc = self._lib.fpsq_band_create_coo_arrow(C.byref(b), self.nvar, self.ncon, rows.size, rows.ctypes.data,
                                                  cols.ctypes.data, 1, self.border, self.cols, device)
        if rc != 0:
            raise FpsqError(self._lib.fpsq_band_last_error(None).decode())
        self._h = b


qdsolver_correspondence["hip_ldlt_arrow"] = HIPArrowBandedDirectQDSolver


# ---------------------------------------------------------------------------------------------- back-end selection

AUTO_MAX_BAND_BLOCKS = 4    # half bandwidth of M = A A' + delta I (in 128-row blocks) up to which "auto" goes direct
AUTO_MAX_BLOCKS = 512       # ... and length of the elimination chain (128-row blocks of M) up to which it does


def band_analysis(nlp, explicit_linear_constraints=False, border=0, cols=0):
    """The symbolic phase alone (fpsq_band_analyze_bordered_cols: host only, no device): blocks / half bandwidth / factor
    bytes / reordered / chains / border rows / long columns of the block-banded structure
    `HIPBandedDirectQDSolver(..., border=border, cols=cols)` would set up for this model's Jacobian pattern."""
    return _band_analysis(nlp, explicit_linear_constraints, border, cols, "fpsq_band_analyze_bordered_cols")


def band_analysis_arrow(nlp, explicit_linear_constraints=False, border=16, cols=16):
    """The same for `HIPArrowBandedDirectQDSolver(..., border=border, cols=cols)` (fpsq_band_analyze_arrow): border rows and
    long columns on one handle."""
    return _band_analysis(nlp, explicit_linear_constraints, border, cols, "fpsq_band_analyze_arrow")


def _band_analysis(nlp, explicit_linear_constraints, border, cols, entry):
    import scipy.sparse as sp

    if explicit_linear_constraints:
        from .nlpmodels import NonlinearConstraintsView
        nlp = NonlinearConstraintsView(nlp)
    n, m = int(nlp.meta.nvar), int(nlp.meta.ncon)
    jrows, jcols = nlp.jac_structure()
    pat = sp.csr_matrix((np.ones(len(jrows)), (np.asarray(jrows) - 1, np.asarray(jcols) - 1)), shape=(m, n))
    pat.sum_duplicates()
    pat.sort_indices()
    rp, ci = pat.indptr.astype(np.int32), pat.indices.astype(np.int32)
    info = _lib.BandInfo()
    rc = getattr(_lib.load(), entry)(n, m, rp.ctypes.data, ci.ctypes.data, int(border), int(cols), None, None, C.byref(info))
    return None if rc != 0 else info.as_dict()


def AutoQDSolver(nlp, _zero=0.0, *, explicit_linear_constraints=False, **kwargs):
    """`qdsolver_correspondence["ldlt"]` -- the reference's key and DEFAULT (`qds_solver = :ldlt`, src/parameters.jl:290), hence
    the default of `fps_solve` here (also registered as "auto").  The reference's general sparse LDL' copes with any
    pattern; on the device the direct route is the block-banded factorisation of M = A A' + delta I ("hip_ldlt"), which is
    exact AND fast only when that band is narrow (small models, grid / PDE-like Jacobians: cfg4 runs at 295 evaluations/s
    there against 206, unsolved, on the iterative path), and falls off an O(m^3) cliff when the band is full (cfg2: the
    random Jacobian makes A A' dense).  So: direct when the symbolic phase reports a half bandwidth <=
    AUTO_MAX_BAND_BLOCKS blocks and <= AUTO_MAX_BLOCKS blocks (chain length), the iterative back-end ("hip" = "iterative",
    the reference's `:iterative`) otherwise.  WHICH one was taken is on record: the solver object carries
    `qds_backend` ("hip_ldlt" | "hip") and `qds_routed_from`, and `fps_solve` copies both into
    `stats.solver_specific`.  `"hip_ldlt"` forces the direct factorisation whatever the band, `"hip"` the matrix-free one."""
    info = band_analysis(nlp, explicit_linear_constraints)
    q = None
    if info is not None and info["bandwidth_blocks"] <= AUTO_MAX_BAND_BLOCKS and info["nblocks"] <= AUTO_MAX_BLOCKS:
        try:
            q = HIPBandedDirectQDSolver(nlp, _zero, explicit_linear_constraints=explicit_linear_constraints, **kwargs)
        except FpsqError:
            q = None   # (does not fit the device after all)
    if q is None:
        kw = {k: v for k, v in kwargs.items() if not k.startswith("ldlt_")}   # (LDLtSolver's keywords mean nothing to Krylov)
        q = HIPQDSolver(nlp, _zero, explicit_linear_constraints=explicit_linear_constraints, **kw)
    q.qds_backend = "hip_ldlt" if isinstance(q, HIPBandedDirectQDSolver) else "hip"
    q.qds_routed_from = "ldlt"
    return q


qdsolver_correspondence["ldlt"] = AutoQDSolver        # src/parameters.jl:197: the reference's :ldlt (its default, :290)
qdsolver_correspondence["auto"] = AutoQDSolver        # (the name of rounds 3-4)
qdsolver_correspondence["iterative"] = HIPQDSolver    # src/parameters.jl:197: the reference's :iterative
