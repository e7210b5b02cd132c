"""The raw C ABI behind a small handle class, shared by the GPU parity tests (test infrastructure)."""
import ctypes as C

import numpy as np
import scipy.sparse as sp

import fps_amd  # noqa: F401
from fps_amd import _lib


class _Handle:
    """Thin test helper around the raw C ABI for a CSR matrix."""

    def __init__(self, A, delta=0.0, **opts):
        self.lib = _lib.load()
        A = sp.csr_matrix(A)
        self.m, self.n = A.shape
        o = _lib.Options()
        self.lib.fpsq_default_options(self.n, self.m, C.byref(o))
        for k, v in opts.items():
            setattr(o, k, v)
        self.h = C.c_void_p()
        assert self.lib.fpsq_create(C.byref(self.h), self.n, self.m, C.byref(o)) == 0, self.lib.fpsq_last_error(None)
        rp, ci = A.indptr.astype(np.int32), A.indices.astype(np.int32)
        assert self.lib.fpsq_set_jacobian_structure_csr(self.h, rp.ctypes.data, ci.ctypes.data) == 0, self.err()
        v = np.ascontiguousarray(A.data, dtype=np.float64)
        assert self.lib.fpsq_set_jacobian_values(self.h, v.ctypes.data) == 0, self.err()
        assert self.lib.fpsq_set_delta(self.h, delta) == 0
        self.st = (_lib.Stats * 2)()

    def err(self):
        return self.lib.fpsq_last_error(self.h)

    def jac_mul(self, trans, alpha, x, beta, y):
        y = np.array(y, dtype=np.float64)
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert self.lib.fpsq_jac_mul(self.h, trans, alpha, x.ctypes.data, beta, y.ctypes.data) == 0, self.err()
        return y

    def two(self, fn, r1, r2, sizes):
        r1 = np.ascontiguousarray(r1, dtype=np.float64)
        r2 = np.ascontiguousarray(r2, dtype=np.float64)
        outs = [np.full(k, np.nan) for k in sizes]   # (preset: an output the call leaves untouched shows)
        rc = fn(self.h, r1.ctypes.data, r2.ctypes.data, *[o.ctypes.data for o in outs], self.st)
        assert rc >= 0, self.err()
        return (*outs, rc)

    def solve_two_mixed(self, r1, r2):
        return self.two(self.lib.fpsq_solve_two_mixed, r1, r2, (self.n, self.m, self.n, self.m))

    def solve_two_least_squares(self, r1, r2):
        return self.two(self.lib.fpsq_solve_two_least_squares, r1, r2, (self.n, self.m, self.n, self.m))

    def solve_two_extras(self, r1, r2):
        return self.two(self.lib.fpsq_solve_two_extras, r1, r2, (self.m, self.m))

    def ys_gs(self, g, c, sigma):
        """fpsq_ys_gs -> (gs, ys, v, w, rc)"""
        fn = self.lib.fpsq_ys_gs
        return self.two(lambda h, a, b, *rest: fn(h, a, b, sigma, *rest), g, c, (self.n, self.m, self.n, self.m))

    def expect(self, iterations):
        """The run-ahead count of the NEXT solve call only (fpsq_debug_expect_iterations)."""
        assert self.lib.fpsq_debug_expect_iterations(self.h, iterations) == 0, self.err()

    def stats(self):
        """(niter, status, solved, rnorm, arnorm, inconsistent) of the two systems of the last call: lane_cases.restate(full=True)"""
        return [(s.niter, s.status, s.solved, s.rnorm, s.arnorm, s.inconsistent) for s in self.st]

    def counters(self):
        i = _lib.Info()
        assert self.lib.fpsq_get_info(self.h, C.byref(i)) == 0
        return (i.fuse_fallbacks, i.wait_timeouts, i.p2p_timeouts)

    def close(self):
        self.lib.fpsq_destroy(self.h)


def _rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)
