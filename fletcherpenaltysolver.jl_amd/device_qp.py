"""Device-resident penalty evaluation on the synthetic eq-QP model: the benchmark's unit of work.

One `objgrad(x)` = one `objgrad!(::FletcherPenaltyNLP, x, gx)` at a fresh x
(src/model-Fletcherpenaltynlp.jl:403-437) executed entirely on the MI355X through `fpsq_qp_objgrad`.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .qdsolver import FpsqError


class DeviceEqQP:
    """`comm`: None (single GPU), ("rccl", nranks, rank, id_bytes) or ("local", group_ptr, shard) for a row-sharded
    model; `qp` is then the rank's row block (distributed.shard_qp).  `halo` = (overlap_left, overlap_right): the
    n-vectors are column windows (distributed.shard_qp_halo / HaloPlan.overlaps) instead of replicated.
    `comm_route` ("auto" | "rccl" | "p2p", with comm = ("rccl", ...)): how the exchanges of the halo-sharded loop travel
    (include/fpsq.h fpsq_comm_set_route; "auto" = peer to peer over hipIpc-mapped buffers when every rank can, else RCCL);
    `info()["comm_route"]` says what the handle ended up with after its first solve."""

    ROUTES = {"auto": 0, "rccl": 1, "p2p": 2}
    ROUTE_NAMES = {0: "single GPU", 1: "rccl", 2: "p2p-ipc", 3: "local", 4: "local-p2p"}

    sparse_hessian = False   # (DeviceSparseHessianEqQP: a QP that carries hess_* is created with fpsq_qp_create_csr)

    def __init__(self, qp, sigma=1e3, rho=1.0, delta=0.0, eta=0.0, device=0, comm=None, halo=None, comm_route=None,
                 **opt_overrides):
        sparse = getattr(qp, "hess_vals", None) is not None
        if sparse and not self.sparse_hessian:   # fpsq_qp_create knows diag(q) alone: never evaluate the diagonal part silently
            raise ValueError("DeviceEqQP (the iterative back-end) takes a diagonal objective Hessian only; a QP with a "
                             "sparse Hessian (EqQP.hess_vals) runs on DeviceBandEqQP or, on the iterative back-end, on "
                             "DeviceSparseHessianEqQP")
        if self.sparse_hessian and (comm is not None or halo is not None):
            raise ValueError("DeviceSparseHessianEqQP is single-GPU: comm / halo are not supported (in halo mode the n-vectors "
                             "are column windows, and the products with the Hessian would need an exchange of their own)")
        self._lib = _lib.load()
        self.qp, self.sigma, self.rho, self.delta, self.eta = qp, sigma, rho, delta, eta
        opts = _lib.Options()
        self._lib.fpsq_default_options(qp.n, qp.m, C.byref(opts))
        opts.device = device
        for k, v in opt_overrides.items():
            setattr(opts, k, v)
        self.opts = opts
        self.device = int(opts.device)
        h = C.c_void_p()
        if self._lib.fpsq_create(C.byref(h), qp.n, qp.m, C.byref(opts)) != 0:
            raise FpsqError(self._lib.fpsq_last_error(None).decode())
        self._h = h
        rp = np.ascontiguousarray(qp.rowptr, dtype=np.int32)
        ci = np.ascontiguousarray(qp.colind, dtype=np.int32)
        self._check(self._lib.fpsq_set_jacobian_structure_csr(h, rp.ctypes.data, ci.ctypes.data))
        self._check(self._lib.fpsq_set_jacobian_values(h, np.ascontiguousarray(qp.vals).ctypes.data))
        self._check(self._lib.fpsq_set_delta(h, float(delta)))
        q = C.c_void_p()
        if sparse:   # sparse symmetric Q (full storage): fpsq_qp_create_csr
            hrp = np.ascontiguousarray(qp.hess_rowptr, dtype=np.int32)
            hci = np.ascontiguousarray(qp.hess_colind, dtype=np.int32)
            hv = np.ascontiguousarray(qp.hess_vals, dtype=np.float64)
            self._check(self._lib.fpsq_qp_create_csr(h, hrp.ctypes.data, hci.ctypes.data, hv.ctypes.data, qp.d.ctypes.data,
                                                     qp.b.ctypes.data, C.byref(q)))
        else:
            self._check(self._lib.fpsq_qp_create(h, qp.qdiag.ctypes.data, qp.d.ctypes.data, qp.b.ctypes.data, C.byref(q)))
        self._q = q
        self.stats = (_lib.Stats * 2)()
        self.stats4 = (_lib.Stats * 4)()   # hprod with hessian_approx = 1: + the two recurrences of solve_two_extras
        self._in_stream = -1
        try:
            self._attach_comm(comm, halo, comm_route)
        except Exception:
            self.close()
            raise

    def _attach_comm(self, comm, halo, comm_route=None):
        h = self._h
        if comm is not None:
            if comm[0] == "rccl":
                _, nranks, rank, ident = comm
                buf = (C.c_uint8 * 128).from_buffer_copy(bytes(ident))
                self._check(self._lib.fpsq_comm_init(h, nranks, rank, C.addressof(buf)))
                if comm_route is not None:
                    self._check(self._lib.fpsq_comm_set_route(h, self.ROUTES[comm_route]))
            elif comm[0] == "local":
                self._check(self._lib.fpsq_comm_init_local(h, comm[1], comm[2]))
            else:
                raise ValueError(comm[0])
            if halo is not None:
                self._check(self._lib.fpsq_comm_set_halo(h, int(halo[0]), int(halo[1])))

    def _check(self, rc):
        if rc < 0:
            raise FpsqError(self._lib.fpsq_last_error(self._h).decode())
        return rc

    def _order(self, *args):
        """Device tensors among the arguments are produced on torch's current stream: register it so the library's
        stream waits for it (fpsq_set_input_stream; include/fpsq.h "INPUT READINESS").  No host synchronisation."""
        st = _lib.producer_stream(*args)
        if st is not None and st != self._in_stream:
            self._check(self._lib.fpsq_set_input_stream(self._h, 1, st))
            # torch consumes the device-resident outputs on that same stream: let the library order them there instead of
            # blocking the host until the last kernel has ended (include/fpsq.h, "STREAM-ORDERED OUTPUTS")
            self._check(self._lib.fpsq_set_output_ordering(self._h, 1))
            self._in_stream = st

    def set_delta(self, delta):
        self.delta = delta
        self._check(self._lib.fpsq_set_delta(self._h, float(delta)))

    def set_jacobian_values(self, vals):
        """`jac_coord!` output at a new x (src/solve_linear_system.jl:223-228), in the order of the structure call: numpy array,
        torch tensor (host or device) or raw address.  Device-resident values are read in place by ONE gather launch, ordered
        on torch's current stream (no host synchronisation): include/fpsq.h fpsq_set_jacobian_values."""
        self._order(vals)
        return self._check(self._lib.fpsq_set_jacobian_values(self._h, _lib.ptr(vals)))

    def set_profiling(self, on):
        self._check(self._lib.fpsq_set_profiling(self._h, int(on)))

    def objgrad(self, x, gx=None, ys=None, gs=None, xk=None):
        """x / gx / ys / gs / xk: numpy arrays, torch tensors (host or device) or raw addresses.
        Returns (fx, rc): rc > 0 flags a Krylov solve that stopped unsolved (the reference warns)."""
        fx = C.c_double()
        self._order(x, gx, ys, gs, xk)
        rc = self._check(self._lib.fpsq_qp_objgrad(self._h, self._q, _lib.ptr(x), self.sigma, self.rho, self.eta,
                                                   _lib.ptr(xk), C.byref(fx), _lib.ptr(gx), _lib.ptr(ys),
                                                   _lib.ptr(gs), self.stats))
        return fx.value, rc

    # -- the QDSolver seam on the same handle; every argument: numpy array, torch tensor (host or device) or address
    def solve_two_mixed(self, rhs1, rhs2, p1, q1, p2, q2):
        """src/solve_linear_system.jl:107-140 on the Jacobian the model holds (outputs are caller-owned buffers)."""
        self._order(rhs1, rhs2, p1, q1, p2, q2)
        return self._check(self._lib.fpsq_solve_two_mixed(self._h, _lib.ptr(rhs1), _lib.ptr(rhs2), _lib.ptr(p1),
                                                          _lib.ptr(q1), _lib.ptr(p2), _lib.ptr(q2), self.stats))

    def solve_two_least_squares(self, rhs1, rhs2, p1, q1, p2, q2):
        """src/solve_linear_system.jl:79-105: the two solves of every hprod! (two LSQR recurrences, fused)."""
        self._order(rhs1, rhs2, p1, q1, p2, q2)
        return self._check(self._lib.fpsq_solve_two_least_squares(self._h, _lib.ptr(rhs1), _lib.ptr(rhs2),
                                                                  _lib.ptr(p1), _lib.ptr(q1), _lib.ptr(p2),
                                                                  _lib.ptr(q2), self.stats))

    def ys_gs(self, g, c, gs, ys, v, w):
        """_compute_ys_gs! after the user-model evaluations (src/model-Fletcherpenaltynlp.jl:242-248)."""
        self._order(g, c, gs, ys, v, w)
        return self._check(self._lib.fpsq_ys_gs(self._h, _lib.ptr(g), _lib.ptr(c), self.sigma, _lib.ptr(gs),
                                                _lib.ptr(ys), _lib.ptr(v), _lib.ptr(w), self.stats))

    def jac_mul(self, trans, alpha, x, beta, y):
        """y = alpha op(A) x + beta y with the model's Jacobian (fpsq_jac_mul; trans = 0: A, 1: A')."""
        self._order(x, y)
        return self._check(self._lib.fpsq_jac_mul(self._h, int(trans), float(alpha), _lib.ptr(x), float(beta), _lib.ptr(y)))

    def hprod(self, v, Hv, hessian_approx=2):
        """hprod!(::FletcherPenaltyNLP, x, v, Hv) on the device, hessian_approx = Val(2) (model-Fletcherpenaltynlp.jl:521-570)
        or Val(1) (:572-634: additionally the solve_two_extras lanes; their statistics land in self.stats4[2:4]); the model
        is quadratic with linear constraints, so the product does not depend on x.  Returns rc."""
        self._order(v, Hv)
        rc = self._check(self._lib.fpsq_qp_hprod(self._h, self._q, _lib.ptr(v), self.sigma, self.rho, self.eta,
                                                 int(hessian_approx), _lib.ptr(Hv), self.stats4))
        self.stats[0], self.stats[1] = self.stats4[0], self.stats4[1]
        return rc

    def info(self):
        i = _lib.Info()
        self._check(self._lib.fpsq_get_info(self._h, C.byref(i)))
        return i.as_dict()

    def close(self):
        if getattr(self, "_h", None):
            self._lib.fpsq_qp_destroy(self._q)
            self._lib.fpsq_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceSparseHessianEqQP(DeviceEqQP):
    """DeviceEqQP for a QP with a sparse symmetric objective Hessian (`EqQP.hess_*`, `problems.with_sparse_hessian`): the model
    is created with `fpsq_qp_create_csr` and evaluated with that Hessian -- an objgrad is two launches longer than on the
    diagonal model, an hprod one (include/fpsq.h).  A QP without `hess_vals` gives the diagonal model.  Single GPU, LSQR + CRAIG /
    LNLQ only: `comm` / `halo` raise ValueError.  Everything else is DeviceEqQP's surface; `fps_solve_device` takes it as it is."""

    sparse_hessian = True


class DeviceBandEqQP:
    """The same device-resident eq-QP model on the DIRECT back-end: the block-banded factorisation of M = A A' + delta I
    (`fpsq_band_*`, the device counterpart of the reference's default `qds_solver = :ldlt`) with `fpsq_band_qp_objgrad` /
    `fpsq_band_qp_hprod` on the CACHED factor.  A QP with a sparse symmetric objective Hessian (`EqQP.hess_*`,
    `problems.with_sparse_hessian`) is evaluated with that Hessian (`fpsq_band_qp_create_csr`).  The factor is rebuilt lazily -- once, at the next evaluation -- after
    `set_delta` or `set_jacobian_values`; `info()["factorizations"]` counts how many this object has run.
    ldlt_tol / ldlt_r2: the dynamic regularisation of `LDLtSolver`, defaults as in qdsolver._DirectQDSolver (sqrt(eps),
    -sqrt(eps); "drop" drops a vanishing pivot).  Has the surface `fps_solve_device` uses on DeviceEqQP.
    `border`, `cols` (class attributes, 0 .. 16; DeviceBorderedBandEqQP sets them per object): the max_border / max_cols the
    handle is created with.  `_create_entry` (class attribute): the C entry that creates it (DeviceArrowBandEqQP names
    `fpsq_band_create_arrow`)."""

    border = 0
    cols = 0
    _create_entry = "fpsq_band_create_bordered_cols"

    def __init__(self, qp, sigma=1e3, rho=1.0, delta=0.0, eta=0.0, device=0, ldlt_tol=None, ldlt_r2=None):
        from .qdsolver import _ldlt_r2

        self._lib = _lib.load()
        self.qp, self.sigma, self.rho, self.delta, self.eta = qp, sigma, rho, float(delta), eta
        self.device = int(device)
        self._h = self._q = None
        rp = np.ascontiguousarray(qp.rowptr, dtype=np.int32)
        ci = np.ascontiguousarray(qp.colind, dtype=np.int32)
        h = C.c_void_p()
        if getattr(self._lib, self._create_entry)(C.byref(h), qp.n, qp.m, rp.ctypes.data, ci.ctypes.data, int(self.border),
                                                  int(self.cols), self.device) != 0:
            raise FpsqError(self._lib.fpsq_band_last_error(None).decode())
        self._h = h
        try:
            se = float(np.sqrt(np.finfo(float).eps))
            self.ldlt_tol = se if ldlt_tol is None else float(ldlt_tol)
            self.ldlt_r2 = _ldlt_r2(ldlt_r2)
            self._check(self._lib.fpsq_band_set_regularization(h, self.ldlt_tol, -self.ldlt_r2))
            q = C.c_void_p()
            dv, bv = np.ascontiguousarray(qp.d, dtype=np.float64), np.ascontiguousarray(qp.b, dtype=np.float64)
            if getattr(qp, "hess_vals", None) is not None:   # sparse symmetric Q (full storage): fpsq_band_qp_create_csr
                hrp = np.ascontiguousarray(qp.hess_rowptr, dtype=np.int32)
                hci = np.ascontiguousarray(qp.hess_colind, dtype=np.int32)
                hv = np.ascontiguousarray(qp.hess_vals, dtype=np.float64)
                self._check(self._lib.fpsq_band_qp_create_csr(h, hrp.ctypes.data, hci.ctypes.data, hv.ctypes.data,
                                                              dv.ctypes.data, bv.ctypes.data, C.byref(q)))
            else:
                self._check(self._lib.fpsq_band_qp_create(h, np.ascontiguousarray(qp.qdiag).ctypes.data, dv.ctypes.data,
                                                          bv.ctypes.data, C.byref(q)))
            self._q = q
        except Exception:
            self.close()
            raise
        self._vals = np.ascontiguousarray(qp.vals, dtype=np.float64)   # CSR-order values the next factorisation takes
        self._stale, self._fact_rc, self.factorizations = True, 0, 0
        self._in_stream = -1

    def _check(self, rc):
        if rc < 0:
            raise FpsqError(self._lib.fpsq_band_last_error(self._h).decode())
        return rc

    def _order(self, *args):
        """Device tensors among the arguments are produced on torch's current stream: register it, so that the handle's
        stream waits for it at the start of every call (fpsq_band_set_input_stream).  No host synchronisation."""
        st = _lib.producer_stream(*args)
        if st is not None and st != self._in_stream:
            self._check(self._lib.fpsq_band_set_input_stream(self._h, 1, st))
            self._in_stream = st

    def set_delta(self, delta):
        if float(delta) != self.delta:
            self._stale = True
        self.delta = float(delta)

    def set_jacobian_values(self, vals):
        """`jac_coord!` output at a new x in CSR order (numpy array, torch tensor on the host or the device, or a raw address);
        the factor is stale from here on and is rebuilt at the next evaluation.  The values are read THEN: keep them unchanged."""
        self._vals = vals
        self._stale = True

    def _factor(self):
        """The lazy (re-)factorisation; returns its soft code (1: M not positive definite and no regularisation)."""
        if self._stale:
            self._order(self._vals)
            self._fact_rc = self._check(self._lib.fpsq_band_factorize(self._h, _lib.ptr(self._vals), self.delta, None))
            self.factorizations += 1
            self._stale = False
        if self._fact_rc:
            import warnings
            warnings.warn("DeviceBandEqQP: A A' + delta I is not positive definite (no valid factorisation)")
        return self._fact_rc

    def objgrad(self, x, gx=None, ys=None, gs=None, xk=None):
        """x / gx / ys / gs / xk: numpy arrays, torch tensors (host or device) or raw addresses.  Returns (fx, rc); with
        rc = 1 (failed factorisation) nothing was evaluated: fx is nan and the outputs are untouched."""
        if self._factor():
            return float("nan"), self._fact_rc
        fx = C.c_double()
        self._order(x, gx, ys, gs, xk)
        self._check(self._lib.fpsq_band_qp_objgrad(self._h, self._q, _lib.ptr(x), self.sigma, self.rho, self.eta,
                                                   _lib.ptr(xk), C.byref(fx), _lib.ptr(gx), _lib.ptr(ys), _lib.ptr(gs)))
        return fx.value, 0

    def hprod(self, v, Hv, hessian_approx=2):
        """hprod!(::FletcherPenaltyNLP, x, v, Hv) on the device (include/fpsq.h fpsq_band_qp_hprod).  Returns rc."""
        if self._factor():
            return self._fact_rc
        self._order(v, Hv)
        return self._check(self._lib.fpsq_band_qp_hprod(self._h, self._q, _lib.ptr(v), self.sigma, self.rho, self.eta,
                                                        int(hessian_approx), _lib.ptr(Hv)))

    @staticmethod
    def _block(a, name, k, length, optional=False):
        """A block argument: a C-contiguous float64 (k, length) numpy array or torch tensor (k = None: any k >= 1); returns k."""
        if a is None:
            if optional:
                return k
            raise ValueError(f"{name}: a block is required")
        shape = tuple(getattr(a, "shape", ()))
        if isinstance(a, np.ndarray):
            ok, contiguous = a.dtype == np.float64, a.flags["C_CONTIGUOUS"]
        elif hasattr(a, "data_ptr"):
            import torch

            ok, contiguous = a.dtype == torch.float64, a.is_contiguous()
        else:
            raise ValueError(f"{name}: a numpy array or a torch tensor is expected, not {type(a).__name__}")
        if not ok:
            raise ValueError(f"{name}: float64 expected, got {a.dtype}")
        if len(shape) != 2 or shape[1] != length or shape[0] < 1 or (k is not None and shape[0] != k):
            want = f"({'k' if k is None else k}, {length})"
            raise ValueError(f"{name}: shape {want} expected, got {shape}")
        if not contiguous:
            raise ValueError(f"{name}: the block must be C-contiguous")
        return shape[0]

    def hprod_block(self, V, HV, hessian_approx=2):
        """Row j of HV = hprod on row j of V: (k, n) float64 blocks, numpy arrays or torch tensors (host or device), C-contiguous
        (include/fpsq.h fpsq_band_qp_hprod_block: 8 vectors per pass over the factor).  Returns rc."""
        k = self._block(V, "V", None, self.qp.n)
        self._block(HV, "HV", k, self.qp.n)
        if self._factor():
            return self._fact_rc
        self._order(V, HV)
        return self._check(self._lib.fpsq_band_qp_hprod_block(self._h, self._q, k, _lib.ptr(V), self.sigma, self.rho,
                                                              self.eta, int(hessian_approx), _lib.ptr(HV)))

    def solve_two_least_squares_block(self, rhs1, rhs2, p1=None, q1=None, p2=None, q2=None):
        """Row j of (p1, q1, p2, q2) = solve_two_least_squares(rhs1[j], rhs2[j]) on the cached factor: (k, n) / (k, m) float64
        blocks as in hprod_block; outputs that are None are not produced (fpsq_band_solve_two_least_squares_block)."""
        n, m = self.qp.n, self.qp.m
        k = self._block(rhs1, "rhs1", None, n)
        self._block(rhs2, "rhs2", k, n)
        for a, name, length in ((p1, "p1", n), (q1, "q1", m), (p2, "p2", n), (q2, "q2", m)):
            self._block(a, name, k, length, optional=True)
        if self._factor():
            return self._fact_rc
        self._order(rhs1, rhs2, p1, q1, p2, q2)
        return self._check(self._lib.fpsq_band_solve_two_least_squares_block(
            self._h, k, _lib.ptr(rhs1), _lib.ptr(rhs2), _lib.ptr(p1), _lib.ptr(q1), _lib.ptr(p2), _lib.ptr(q2)))

    def objgrad_block(self, X, GX=None, YS=None, GS=None, XK=None, D=None, B=None):
        """Row j = objgrad at X[j] on this QP with its linear term replaced by D[j] and its right-hand side by B[j] (None: the
        model's own d / b for every row): k points of one QP, or a family of QPs that share A and Q, in one pass over the
        cached factor per 8 rows (include/fpsq.h fpsq_band_qp_objgrad_block).  X, GX, GS, XK, D: (k, n), YS, B: (k, m) float64
        blocks as in hprod_block; outputs that are None are not produced.  Returns (fx, rc), fx a numpy (k,) array; with
        rc = 1 (failed factorisation) nothing was evaluated: fx is all nan and the outputs are untouched."""
        n, m = self.qp.n, self.qp.m
        k = self._block(X, "X", None, n)
        for a, name, length in ((GX, "GX", n), (YS, "YS", m), (GS, "GS", n), (XK, "XK", n), (D, "D", n), (B, "B", m)):
            self._block(a, name, k, length, optional=True)
        fx = np.full(k, np.nan)
        if self._factor():
            return fx, self._fact_rc
        self._order(X, GX, YS, GS, XK, D, B)
        self._check(self._lib.fpsq_band_qp_objgrad_block(self._h, self._q, k, _lib.ptr(X), _lib.ptr(D), _lib.ptr(B), self.sigma,
                                                         self.rho, self.eta, _lib.ptr(XK), fx.ctypes.data, _lib.ptr(GX),
                                                         _lib.ptr(YS), _lib.ptr(GS)))
        return fx, 0

    def jac_mul(self, trans, alpha, x, beta, y):
        """y = alpha op(A) x + beta y with the model's Jacobian (fpsq_band_jac_mul; trans = 0: A, 1: A')."""
        self._factor()   # (the values reach the handle with a factorisation)
        self._order(x, y)
        return self._check(self._lib.fpsq_band_jac_mul(self._h, int(trans), float(alpha), _lib.ptr(x), float(beta),
                                                       _lib.ptr(y)))

    def info(self):
        i = _lib.BandInfo()
        self._check(self._lib.fpsq_band_get_info(self._h, C.byref(i)))
        return {**i.as_dict(), "factorizations": self.factorizations}

    def close(self):
        if getattr(self, "_q", None):
            self._lib.fpsq_band_qp_destroy(self._q)
            self._q = None
        if getattr(self, "_h", None):
            self._lib.fpsq_band_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceBorderedBandEqQP(DeviceBandEqQP):
    """DeviceBandEqQP on a BORDERED band: at most `border` (0 .. 16) long constraint rows -- rows that couple with every other
    row of M = A A' + delta I, such as a mean-value, volume or mass-conservation constraint or the wrap-around rows of a
    periodic boundary -- are eliminated last instead of widening the band (include/fpsq.h "BORDERED BAND").  Every method
    is the base class's; `info()["border_rows"]` says how many rows were taken (0: the handle is DeviceBandEqQP's).
    `cols` (0 .. 16) is the transposed case: at most that many long COLUMNS -- a global parameter, a free final time, a
    scalar control -- are taken out of the band and every M-solve is corrected by a low-rank term (include/fpsq.h "LONG
    COLUMNS"); `info()["border_cols"]` says how many were taken and `info()["border_pivot_ratio"]` what the correction costs
    in digits.  A handle of THIS class takes ONE kind: pass `border=0` with `cols`; DeviceArrowBandEqQP takes both.  The other
    keywords are DeviceBandEqQP's (whose parameter list stays as it is)."""

    def __init__(self, qp, border=16, cols=0, **kwargs):
        self.border = int(border)
        self.cols = int(cols)
        super().__init__(qp, **kwargs)


class DeviceArrowBandEqQP(DeviceBandEqQP):
    """DeviceBandEqQP on an ARROW band: at most `border` long constraint rows AND at most `cols` long columns on one handle
    (both 0 .. 16, independently; include/fpsq.h "ARROW BAND") -- a model with a global parameter or a free final time that
    also has an integral, mean-value or mass constraint.  Every method is the base class's; `info()["border_rows"]` and
    `info()["border_cols"]` say what was taken (nothing of one kind: the handle is DeviceBorderedBandEqQP's of the other).
    The other keywords are DeviceBandEqQP's."""

    _create_entry = "fpsq_band_create_arrow"

    def __init__(self, qp, border=16, cols=16, **kwargs):
        self.border = int(border)
        self.cols = int(cols)
        super().__init__(qp, **kwargs)


class DeviceBandSepQuadNLP:
    """The device-resident model with NONLINEAR equality constraints on the banded direct back-end (`fpsq_band_nlp_*`):
    `nlp_data` is a `problems.SepQuadNLP` (`problems.with_quadratic_constraints`) -- the QP's objective with
    c_i(x) = sum_j (A_ij + 1/2 H_ij x_j) x_j - b_i.  The Jacobian moves with x, so every `objgrad` writes J(x) into the handle
    and refactorises J J' + delta I (`info()["factorizations"]` counts them); `hprod` runs at the point of the last objgrad, on
    its factor, and the two `hessian_approx` modes differ.  `objgrad` / `hprod` have DeviceBandEqQP's parameter lists;
    `fps_solve_device` takes the object (`nonlinear = True` selects the penalty wrapper that keeps track of that point).
    `qp` is the underlying EqQP (objective, pattern, x, xhat).
    `_create_entry`, `_limits`, `_model_entry` (class attributes): the C entry that creates the handle, the (max_border,
    max_cols) it takes behind the pattern (none: `fpsq_band_create`), and the entry that creates the model on it
    (DeviceArrowBandSepQuadNLP names `fpsq_band_create_arrow` and `fpsq_band_nlp_create_arrow`)."""

    nonlinear = True
    _create_entry = "fpsq_band_create"
    _limits = ()
    _model_entry = "fpsq_band_nlp_create"

    def __init__(self, nlp_data, sigma=1e3, rho=1.0, delta=0.0, eta=0.0, device=0, ldlt_tol=None, ldlt_r2=None):
        from .qdsolver import _ldlt_r2

        self._lib = _lib.load()
        qp = nlp_data.qp
        self.nlp_data, self.qp = nlp_data, qp
        self.sigma, self.rho, self.delta, self.eta = sigma, rho, float(delta), eta
        self.device = int(device)
        self._h = self._q = None
        self.obj_w = self.obj_codes = None   # host copies of the objective's function terms (set_objective_terms), or None
        self.factorizations = 0
        self._in_stream = -1
        rp = np.ascontiguousarray(qp.rowptr, dtype=np.int32)
        ci = np.ascontiguousarray(qp.colind, dtype=np.int32)
        h = C.c_void_p()
        if getattr(self._lib, self._create_entry)(C.byref(h), qp.n, qp.m, rp.ctypes.data, ci.ctypes.data,
                                                  *(int(v) for v in self._limits), self.device) != 0:
            raise FpsqError(self._lib.fpsq_band_last_error(None).decode())
        self._h = h
        try:
            se = float(np.sqrt(np.finfo(float).eps))
            self.ldlt_tol = se if ldlt_tol is None else float(ldlt_tol)
            self.ldlt_r2 = _ldlt_r2(ldlt_r2)
            self._check(self._lib.fpsq_band_set_regularization(h, self.ldlt_tol, -self.ldlt_r2))
            f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
            q = C.c_void_p()
            keep = [f64(a) for a in (qp.qdiag, qp.d, nlp_data.b, qp.vals, nlp_data.hvals)] + list(self._model_extra(nlp_data))
            self._check(getattr(self._lib, self._model_entry)(h, *(a.ctypes.data if isinstance(a, np.ndarray) else a
                                                                   for a in keep), C.byref(q)))
            self._q = q
            if getattr(nlp_data, "obj_w", None) is not None:   # problems.with_objective_terms
                self.set_objective_terms(nlp_data.obj_w, getattr(nlp_data, "obj_codes", None))
        except Exception:
            self.close()
            raise

    _check = DeviceBandEqQP._check
    _order = DeviceBandEqQP._order
    _refusal = "a non-finite value in the objective's function terms"   # what an objgrad with info = -1 has met

    def _model_extra(self, nlp_data):
        """what `_model_entry` takes between h_vals and the model's address: numpy arrays (kept alive over the call) or scalars"""
        return ()

    def set_objective_terms(self, w, codes=None):
        """Elementwise function terms in the objective, f += sum_j w_j psi_kj(x_j) (include/fpsq.h
        fpsq_band_nlp_set_objective_terms): `w` n weights, `codes` n code bytes of the table FPSQ_FN_* (None: every code 0), numpy
        arrays or torch tensors on the host or the device, copied.  `w=None` removes the terms.  Allowed at any time; the next
        `hprod` needs a new `objgrad`.  Returns rc."""
        if w is None:
            rc = self._check(self._lib.fpsq_band_nlp_set_objective_terms(self._h, self._q, None, None))
            self.obj_w = self.obj_codes = None
            return rc
        if isinstance(w, np.ndarray) or not hasattr(w, "data_ptr"):
            w = np.ascontiguousarray(w, dtype=np.float64)
        if codes is not None and (isinstance(codes, np.ndarray) or not hasattr(codes, "data_ptr")):
            codes = np.ascontiguousarray(codes, dtype=np.uint8)
        assert w.shape[0] == self.qp.n and (codes is None or codes.shape[0] == self.qp.n)
        assert str(w.dtype).endswith("float64") and (codes is None or str(codes.dtype).endswith("uint8"))
        self._order(w, codes)
        rc = self._check(self._lib.fpsq_band_nlp_set_objective_terms(self._h, self._q, _lib.ptr(w), _lib.ptr(codes)))
        host = lambda a: a.copy() if isinstance(a, np.ndarray) else a.cpu().numpy()  # noqa: E731
        self.obj_w = host(w)
        self.obj_codes = np.zeros(self.qp.n, dtype=np.uint8) if codes is None else host(codes)
        return rc

    def set_delta(self, delta):
        """The delta of the NEXT objgrad's factorisation (an hprod stays on the factor of the last one)."""
        self.delta = float(delta)

    def objgrad(self, x, gx=None, ys=None, gs=None, xk=None):
        """One objgrad at a fresh x, its factorisation included.  Returns (fx, rc); with rc = 1 (J J' + delta I not positive
        definite and no regularisation) nothing was evaluated: fx is nan and the outputs are untouched."""
        fx = C.c_double()
        where = C.c_int32(0)
        self._order(x, gx, ys, gs, xk)
        rc = self._check(self._lib.fpsq_band_nlp_objgrad(self._h, self._q, _lib.ptr(x), self.sigma, self.rho, self.eta,
                                                         self.delta, _lib.ptr(xk), C.byref(fx), _lib.ptr(gx), _lib.ptr(ys),
                                                         _lib.ptr(gs), C.byref(where)))
        if rc and where.value == -1:   # refused before the factorisation, which is therefore not counted
            import warnings
            warnings.warn(f"{type(self).__name__}: {self._refusal} (nothing was factorised or evaluated)")
            return float("nan"), rc
        self.factorizations += 1
        if rc:
            import warnings
            warnings.warn(f"{type(self).__name__}: J J' + delta I is not positive definite (no valid factorisation)")
            return float("nan"), rc
        return fx.value, 0

    def hprod(self, v, Hv, hessian_approx=2):
        """hprod!(::FletcherPenaltyNLP, x, v, Hv) at the x of the last objgrad (include/fpsq.h fpsq_band_nlp_hprod).  Returns rc."""
        self._order(v, Hv)
        return self._check(self._lib.fpsq_band_nlp_hprod(self._h, self._q, _lib.ptr(v), self.sigma, self.rho, self.eta,
                                                         int(hessian_approx), _lib.ptr(Hv)))

    def cons(self, x, c):
        """c = c(x), in the caller's row order (no factorisation needed)."""
        self._order(x, c)
        return self._check(self._lib.fpsq_band_nlp_cons(self._h, self._q, _lib.ptr(x), _lib.ptr(c)))

    def jac_mul(self, trans, alpha, x, beta, y):
        """y = alpha op(J) x + beta y with J = the Jacobian at the x of the last objgrad (fpsq_band_jac_mul)."""
        self._order(x, y)
        return self._check(self._lib.fpsq_band_jac_mul(self._h, int(trans), float(alpha), _lib.ptr(x), float(beta),
                                                       _lib.ptr(y)))

    def info(self):
        i = _lib.BandInfo()
        self._check(self._lib.fpsq_band_get_info(self._h, C.byref(i)))
        return {**i.as_dict(), "factorizations": self.factorizations}

    def close(self):
        if getattr(self, "_q", None):
            self._lib.fpsq_band_nlp_destroy(self._q)
            self._q = None
        if getattr(self, "_h", None):
            self._lib.fpsq_band_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceArrowBandSepQuadNLP(DeviceBandSepQuadNLP):
    """DeviceBandSepQuadNLP on an ARROW band: at most `border` long constraint rows and at most `cols` long columns (both
    0 .. 16, independently; include/fpsq.h "ARROW BAND") stay out of the band of J J' + delta I -- a nonlinear model with a
    free final time or a global parameter and an integral, mean-value or mass constraint.  The handle comes from
    `fpsq_band_create_arrow`, the model from `fpsq_band_nlp_create_arrow`; every method is the base class's.
    `info()["border_rows"]` and `info()["border_cols"]` say what was taken; `border=0` or `cols=0` gives the handle of one
    kind, both the plain one.  The other keywords are DeviceBandSepQuadNLP's (whose parameter list stays as it is)."""

    _create_entry = "fpsq_band_create_arrow"
    _model_entry = "fpsq_band_nlp_create_arrow"

    def __init__(self, nlp_data, border=16, cols=16, **kwargs):
        self._limits = (int(border), int(cols))
        super().__init__(nlp_data, **kwargs)


class DeviceBandCoupledQuadNLP(DeviceBandSepQuadNLP):
    """DeviceBandSepQuadNLP with COUPLING TERMS w x_j x_k between columns of a constraint row (`nlp_data`: a
    `problems.CoupledQuadNLP` -- `problems.with_coupled_constraints`, `problems.bilinear_control_like`; host view:
    `nlpmodels.CoupledQuadConModel`): a state times a control, a state times a parameter.  The model comes from
    `fpsq_band_nlp_create_coupled` (include/fpsq.h); every method is the base class's, and `fps_solve_device` takes the object
    unchanged.  Without terms the model is DeviceBandSepQuadNLP's, bit for bit."""

    _model_entry = "fpsq_band_nlp_create_coupled"

    def _model_extra(self, nlp_data):
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
        return (C.c_int64(int(nlp_data.t_w.size)), i32(nlp_data.t_row), i32(nlp_data.t_j), i32(nlp_data.t_k),
                np.ascontiguousarray(nlp_data.t_w, dtype=np.float64))


class DeviceArrowBandCoupledQuadNLP(DeviceBandCoupledQuadNLP):
    """DeviceBandCoupledQuadNLP on an ARROW band (DeviceArrowBandSepQuadNLP's handle): at most `border` long constraint rows and
    at most `cols` long columns (both 0 .. 16) stay out of the band, and the coupling terms may lie in every row and between
    every two columns of a row, long columns included -- a free final time or a global parameter MULTIPLIES the dynamics
    (theta y_k, theta u_k in every row: terms whose second column is a long column; `problems.free_final_time_like`), which
    neither parent class can state.  The handle comes from `fpsq_band_create_arrow`, the model from
    `fpsq_band_nlp_create_coupled_arrow` (include/fpsq.h); every method is the base class's and `fps_solve_device` takes the
    object.  Without terms the model is DeviceArrowBandSepQuadNLP's, on a handle without border rows and long columns
    DeviceBandCoupledQuadNLP's, bit for bit.  The other keywords are DeviceBandSepQuadNLP's."""

    _create_entry = "fpsq_band_create_arrow"
    _model_entry = "fpsq_band_nlp_create_coupled_arrow"

    def __init__(self, nlp_data, border=16, cols=16, **kwargs):
        self._limits = (int(border), int(cols))
        super().__init__(nlp_data, **kwargs)


class DeviceBandSepFuncNLP(DeviceBandSepQuadNLP):
    """DeviceBandSepQuadNLP with an ELEMENTWISE FUNCTION on every curvature entry (`nlp_data`: a `problems.SepFuncNLP` --
    `problems.with_function_constraints`, `problems.pendulum_like`; host view: `nlpmodels.SepFuncConModel`):
    c_i(x) = sum_j (A_ij x_j + H_ij phi(x_j)) - b_i with phi from the table FPSQ_FN_* of include/fpsq.h by the entry's code byte
    (1/2 x^2, x^3/6, sin, cos, exp, tanh).  The model comes from `fpsq_band_nlp_create_fn`; every method is the base class's
    and `fps_solve_device` takes the object unchanged.  With every code 0 the model is DeviceBandSepQuadNLP's, bit for bit.
    An objgrad whose J(x) holds a non-finite value (exp above 709) returns (nan, 1) like a failed factorisation, but runs
    none: `info()["factorizations"]` does not count it (the base class's objgrad; fpsq_band_last_error says which terms)."""

    _model_entry = "fpsq_band_nlp_create_fn"
    _refusal = "a non-finite value in J(x) or in the objective's function terms"

    def _model_extra(self, nlp_data):
        return (np.ascontiguousarray(nlp_data.codes, dtype=np.uint8),)


class DeviceArrowBandSepFuncNLP(DeviceBandSepFuncNLP):
    """DeviceBandSepFuncNLP on an ARROW band (DeviceArrowBandSepQuadNLP's handle): at most `border` long constraint rows and at
    most `cols` long columns (both 0 .. 16) stay out of the band; function codes may sit on the entries of border rows and of
    long columns like on any other.  The handle comes from `fpsq_band_create_arrow`; with every code 0 the model is
    DeviceArrowBandSepQuadNLP's, with `border=0, cols=0` DeviceBandSepFuncNLP's, bit for bit."""

    _create_entry = "fpsq_band_create_arrow"

    def __init__(self, nlp_data, border=16, cols=16, **kwargs):
        self._limits = (int(border), int(cols))
        super().__init__(nlp_data, **kwargs)


def rccl_unique_id() -> bytes:
    """128-byte RCCL id (call on rank 0, broadcast, pass to every rank's DeviceEqQP(comm=("rccl", ...)))."""
    lib = _lib.load()
    buf = (C.c_uint8 * 128)()
    if lib.fpsq_comm_unique_id(C.addressof(buf)) != 0:
        raise FpsqError(lib.fpsq_last_error(None).decode())
    return bytes(buf)


class LocalGroup:
    """In-process stand-in for RCCL: `nshards` row-shard models on ONE GPU, one host thread each."""

    def __init__(self, nshards, p2p=False):
        """p2p: the shards exchange peer to peer (records written into the peers' buffers + sequence flags, no collective call
        in the Krylov loop: include/fpsq.h fpsq_local_group_set_p2p) instead of through event-ordered copy kernels."""
        self._lib = _lib.load()
        g = C.c_void_p()
        if self._lib.fpsq_local_group_create(nshards, C.byref(g)) != 0:
            raise FpsqError("local_group_create failed")
        self.ptr, self.nshards = g, nshards
        if p2p:
            self._lib.fpsq_local_group_set_p2p(g, 1)

    def run(self, fns):
        """Run one callable per shard concurrently (collectives rendezvous across the threads)."""
        import threading

        out, err = [None] * len(fns), [None] * len(fns)

        def work(i):
            try:
                out[i] = fns[i]()
            except BaseException as e:  # noqa: BLE001
                err[i] = e

        ts = [threading.Thread(target=work, args=(i,)) for i in range(len(fns))]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        for e in err:
            if e is not None:
                raise e
        return out

    def close(self):
        if self.ptr:
            self._lib.fpsq_local_group_destroy(self.ptr)
            self.ptr = None
