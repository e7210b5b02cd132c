"""One SETTING of the tail's A' product (tests/test_gpu_tail_three_lanes.py) in a process of its own -- the handle reads
FPSQ_TAIL_LANES / FPSQ_CRAIG_X when it is created, so the caller sets them in this process's environment:

    python tests/tail_lanes_worker.py OUT.npz

Runs every case x delta x rho through the entry points that form or use v = -A'q2 (fpsq_solve_two_mixed, fpsq_ys_gs,
fpsq_qp_objgrad twice -- the second with a speculative tail -- and fpsq_qp_hprod behind it) and writes all outputs, statistics,
launch counts and the handles' cumulative counters to OUT.npz under the keys "<case>/<delta index>/<rho>/<what>"."""
import ctypes as C
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SE = float(np.sqrt(np.finfo(float).eps))
DELTAS = [0.0, SE]
RHOS = [0.0, 1.0]
SIGMA = 1e3
CASES = ["one-block", "partial-last-block", "aligned-blocks", "empty-rows", "row-across-slot-1024", "pde-20000"]


def at_row_slots(A):
    """First slot of every row of A' in a row-major numbering of its entries (= slot in its block for the rows of the first block)."""
    return np.concatenate([[0], np.cumsum(np.diff(sp.csc_matrix(A).indptr))])


def case_matrix(name):
    from fps_amd import problems
    from structures import random_structure

    if name == "one-block":                # 800 entries: ONE A' block
        A = problems.pde_control_like(n=600, m=40, per_row=20, window=512, seed=41).scipy_csr()
    elif name == "partial-last-block":     # 3000 entries: two blocks, the last one partly filled
        A = problems.pde_control_like(n=1500, m=150, per_row=20, window=512, seed=43).scipy_csr()
    elif name == "aligned-blocks":         # 10000 entries: several blocks, boundaries cut at multiples of 8 rows
        A = problems.pde_control_like(n=5000, m=500, per_row=20, window=512, seed=47).scipy_csr()
    elif name == "empty-rows":             # columns 600 .. 4999 of A are empty: row blocks of A' made of empty rows only
        A = random_structure("empty-columns", np.random.default_rng(29))
    elif name == "row-across-slot-1024":   # the longest row of A' (600 entries) lies across slot 1024 of the first block
        A = problems.pde_control_like(n=3000, m=600, per_row=4, window=512, seed=53).scipy_csr().tolil()
        first = at_row_slots(sp.csr_matrix(A))
        j = int(np.searchsorted(first, 800))
        A[:, j] = np.random.default_rng(59).standard_normal((600, 1))
        A = sp.csr_matrix(A)
        first = at_row_slots(A)
        assert first[j] < 1024 < first[j + 1] <= 2048 and first[j + 1] - first[j] == 600, (j, first[j], first[j + 1])
    elif name == "pde-20000":              # the headline generator's small case (padded blocks without values of their own)
        A = problems.pde_control_like(n=20000, m=2000, per_row=40, window=1024, seed=3).scipy_csr()
    else:
        raise ValueError(name)
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A


def main():
    out_path = sys.argv[1]
    import torch  # noqa: F401  (first: one HIP runtime per process)

    import fps_amd  # noqa: F401
    from fps_amd import _lib

    lib = _lib.load()
    res = {}
    for name in CASES:
        A = case_matrix(name)
        m, n = A.shape
        rng = np.random.default_rng(31)
        qdiag, d = 1.0 + rng.random(n), rng.standard_normal(n)
        x, b, hv_in = rng.standard_normal(n), rng.standard_normal(m), rng.standard_normal(n)
        g, c = qdiag * x + d, A @ x - b
        rp, ci = A.indptr.astype(np.int32), A.indices.astype(np.int32)
        vals = np.ascontiguousarray(A.data, dtype=np.float64)
        for di, delta in enumerate(DELTAS):
            for rho in RHOS:
                o = _lib.Options()
                lib.fpsq_default_options(n, m, C.byref(o))
                h, q = C.c_void_p(), C.c_void_p()
                assert lib.fpsq_create(C.byref(h), n, m, C.byref(o)) == 0, lib.fpsq_last_error(None)
                assert lib.fpsq_set_jacobian_structure_csr(h, rp.ctypes.data, ci.ctypes.data) == 0, lib.fpsq_last_error(h)
                assert lib.fpsq_set_jacobian_values(h, vals.ctypes.data) == 0, lib.fpsq_last_error(h)
                assert lib.fpsq_set_delta(h, float(delta)) == 0
                assert lib.fpsq_qp_create(h, qdiag.ctypes.data, d.ctypes.data, b.ctypes.data, C.byref(q)) == 0, lib.fpsq_last_error(h)
                st = (_lib.Stats * 2)()
                info = _lib.Info()
                key = f"{name}/{di}/{int(rho)}/"

                def stats():
                    return np.array([[s.solved, s.inconsistent, s.niter, s.status, s.rnorm, s.arnorm] for s in st]).ravel()

                def launches():
                    assert lib.fpsq_get_info(h, C.byref(info)) == 0
                    return np.array([info.last_kernel_launches, info.last_loop_launches, info.last_loop_iterations])

                for call in range(2):  # (the second call of a kind knows its iteration count: nothing depends on timing)
                    outs = [np.full(k, np.nan) for k in (n, m, n, m)]
                    rc = lib.fpsq_solve_two_mixed(h, g.ctypes.data, c.ctypes.data, *[a.ctypes.data for a in outs], st)
                    assert rc >= 0, lib.fpsq_last_error(h)
                    for k, a in zip(("p1", "q1", "v", "q2"), outs):
                        res[key + f"mixed{call}/{k}"] = a
                    res[key + f"mixed{call}/st"] = np.concatenate([[rc], stats()])
                    res[key + f"mixed{call}/launches"] = launches()
                for call in range(2):
                    outs = [np.full(k, np.nan) for k in (n, m, n, m)]
                    rc = lib.fpsq_ys_gs(h, g.ctypes.data, c.ctypes.data, SIGMA, *[a.ctypes.data for a in outs], st)
                    assert rc >= 0, lib.fpsq_last_error(h)
                    for k, a in zip(("gs", "ys", "v", "w"), outs):
                        res[key + f"ys_gs{call}/{k}"] = a
                    res[key + f"ys_gs{call}/st"] = np.concatenate([[rc], stats()])
                    res[key + f"ys_gs{call}/launches"] = launches()
                for call in range(2):
                    fx = C.c_double()
                    gx, ys, gs = np.full(n, np.nan), np.full(m, np.nan), np.full(n, np.nan)
                    rc = lib.fpsq_qp_objgrad(h, q, x.ctypes.data, SIGMA, rho, 0.0, None, C.byref(fx), gx.ctypes.data, ys.ctypes.data,
                                             gs.ctypes.data, st)
                    assert rc >= 0, lib.fpsq_last_error(h)
                    # v of the evaluation (Cx) is not an output of objgrad: gs = fma(sigma, v, p1) carries its bits, and the
                    # Hessian product below reads the stored vector itself
                    for k, a in zip(("fx", "gx", "ys", "gs"), (np.array([fx.value]), gx, ys, gs)):
                        res[key + f"objgrad{call}/{k}"] = a
                    res[key + f"objgrad{call}/st"] = np.concatenate([[rc], stats()])
                    res[key + f"objgrad{call}/launches"] = launches()
                    hv = np.full(n, np.nan)
                    rc = lib.fpsq_qp_hprod(h, q, hv_in.ctypes.data, SIGMA, rho, 0.0, 2, hv.ctypes.data, st)
                    assert rc >= 0, lib.fpsq_last_error(h)
                    res[key + f"hprod{call}/hv"] = hv
                    res[key + f"hprod{call}/st"] = np.concatenate([[rc], stats()])
                assert lib.fpsq_get_info(h, C.byref(info)) == 0
                res[key + "at_sorted"] = np.array([info.at_sorted])
                res[key + "counters"] = np.array([info.fuse_fallbacks, info.wait_timeouts, info.p2p_timeouts])
                lib.fpsq_qp_destroy(q)
                lib.fpsq_destroy(h)
    np.savez(out_path, **res)


if __name__ == "__main__":
    main()
