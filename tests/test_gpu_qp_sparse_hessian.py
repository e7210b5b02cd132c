"""Device-resident objgrad / hprod on the ITERATIVE back-end with a SPARSE SYMMETRIC objective Hessian (fpsq_qp_create_csr,
DeviceSparseHessianEqQP).  oracle/ knows diag(q) only, so the yardsticks are the exact evaluation in scipy
(tests/sparse_hessian_ref.py), the host mirror through HIPQDSolver, and the diagonal model on the same handle.  The bars are the
ones tests/test_gpu_parity.py holds the diagonal iterative model to: max|a - b| / max|b| < 1e-9 against the exact solve at TIGHT
tolerances, < 1e-5 at the default tolerances, < 1e-8 where two evaluations run the same algorithm at the same tolerances.
With ln_method = LNLQ and delta > 0 the exact evaluation solves the least-norm system unregularised, as that method does (_LnlqRef).

Lanes per row of R = Q - diag(Q) follow lane_group(nnz(R), n): half_width 1 / 2 / 8 give groups of 1 / 2 / 8 lanes, with rows of R
that have no entry (with_sparse_hessian leaves every 7th row empty); n = 4000 is a multiple of the rows per workgroup of the
8-lane group and not of the 1-lane group's, n = 6000 of neither (asserted below through the same rule)."""
import ctypes as C
import dataclasses
import functools
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

sys.path.insert(0, os.path.dirname(__file__))
import fps_amd  # noqa: E402,F401
from fps_amd import _lib, nlpmodels, problems  # noqa: E402
from fps_amd.device_qp import DeviceEqQP, DeviceSparseHessianEqQP, LocalGroup  # noqa: E402
from fps_amd.penalty_nlp import FletcherPenaltyNLP  # noqa: E402
from fps_amd.qdsolver import HIPQDSolver  # noqa: E402
from sparse_hessian_ref import SparseHessianRef  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(float).eps)
SE = float(np.sqrt(EPS))
SIGMA = 1e3
TIGHT = dict(ls_atol=1e-15, ls_rtol=1e-15, ls_axtol=1e-15, ls_btol=1e-15, ls_etol=1e-15,
             ln_atol=1e-15, ln_rtol=1e-15, ln_btol=1e-15, ln_conlim=0.0)
SHAPES = {
    "n4000": lambda: problems.pde_control_like(n=4000, m=400, per_row=16, window=512, seed=21),
    "n6000": lambda: problems.pde_control_like(n=6000, m=640, per_row=16, window=512, seed=23),
    # large enough for one launch per iteration and the column-sorted A' blocks of the one-launch tail
    "n24000": lambda: problems.pde_control_like(n=24000, m=2400, per_row=20, window=512, seed=23),
}


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


@functools.lru_cache(maxsize=None)
def _qp(shape, hw):
    return problems.with_sparse_hessian(SHAPES[shape](), hw, 11)


class _LnlqRef(SparseHessianRef):
    """The exact evaluation of what ln_method = FPSQ_LN_LNLQ solves (include/fpsq.h; tests/test_gpu_parity.py
    test_lnlq_method_parity: "delta only preconditions: unregularised answer"): LNLQ runs the reference's generic solve_least_norm
    with M = (1/delta) I WITHOUT sqd, so the least-norm system K [p2; q2] = [0; c] of objgrad is solved with delta = 0, while the
    LSQR systems (objgrad's first, both of hprod) keep K = [I A'; A -delta I].  Same scipy evaluation, same formulas; the one
    solve with a zero top block goes through a second factorisation.  (Against SparseHessianRef itself the LNLQ lane is
    O(delta) away by construction -- measured 1.05e-9 in ys at delta = sqrt(eps), n = 4000, hw = 1 -- with the diagonal model
    exactly as with a sparse Hessian: c = A x - b does not involve Q.)"""

    def __init__(self, qp, delta):
        super().__init__(qp, delta)
        K0 = sp.bmat([[sp.identity(qp.n), self.A.T], [self.A, None]], format="csc")
        self._lu0 = spla.splu(K0)

    def _solve(self, top, bottom):
        if not np.any(top):          # the least-norm system (0, c): the only solve of an evaluation with a zero top block
            sol = self._lu0.solve(np.concatenate([top, bottom]))
            return sol[:self.n], sol[self.n:]
        return super()._solve(top, bottom)


@functools.lru_cache(maxsize=None)
def _ref(shape, hw, delta, ln_method=0):
    """the exact reference of a case: factorised once, shared, never modified"""
    return (_LnlqRef if ln_method == 1 and delta > 0.0 else SparseHessianRef)(_qp(shape, hw), delta)


def _small():
    return SHAPES["n4000"]()


def _lanes(qp):
    """lane_group(nnz(R), n) of csrc/fpsq_lanegroup.h"""
    mean = (int(qp.hess_vals.size) - int(np.count_nonzero(qp.hess_csr().diagonal()))) // qp.n
    lg = 1
    while lg < 64 and 2 * lg <= mean:
        lg *= 2
    return lg


class _H:
    """One iterative handle on a QP's Jacobian through the raw C ABI, with any number of models on it."""

    def __init__(self, qp, delta=0.0, **opts):
        self.lib = lib = _lib.load()
        self.qp, self.n, self.m = qp, qp.n, qp.m
        o = _lib.Options()
        lib.fpsq_default_options(qp.n, qp.m, C.byref(o))
        for k, v in opts.items():
            setattr(o, k, v)
        self.h = C.c_void_p()
        assert lib.fpsq_create(C.byref(self.h), qp.n, qp.m, C.byref(o)) == 0, lib.fpsq_last_error(None)
        rp, ci = np.ascontiguousarray(qp.rowptr, dtype=np.int32), np.ascontiguousarray(qp.colind, dtype=np.int32)
        assert lib.fpsq_set_jacobian_structure_csr(self.h, rp.ctypes.data, ci.ctypes.data) == 0, self.err()
        assert lib.fpsq_set_jacobian_values(self.h, np.ascontiguousarray(qp.vals).ctypes.data) == 0, self.err()
        assert lib.fpsq_set_delta(self.h, float(delta)) == 0
        self.models = []
        self.st = (_lib.Stats * 4)()

    def err(self):
        return self.lib.fpsq_last_error(self.h).decode()

    def diag(self, qdiag=None):
        q = C.c_void_p()
        qd = np.ascontiguousarray(self.qp.qdiag if qdiag is None else qdiag, dtype=np.float64)
        assert self.lib.fpsq_qp_create(self.h, qd.ctypes.data, self.qp.d.ctypes.data, self.qp.b.ctypes.data, C.byref(q)) == 0
        self.models.append(q)
        return q

    def try_csr(self, rp, ci, va):
        q = C.c_void_p()
        rc = self.lib.fpsq_qp_create_csr(self.h, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, self.qp.d.ctypes.data,
                                         self.qp.b.ctypes.data, C.byref(q))
        return rc, self.err(), q

    def csr(self, qp=None):
        qp = self.qp if qp is None else qp
        rc, msg, q = self.try_csr(qp.hess_rowptr, qp.hess_colind, qp.hess_vals)
        assert rc == 0 and q.value, msg
        self.models.append(q)
        return q

    def info(self):
        i = _lib.Info()
        assert self.lib.fpsq_get_info(self.h, C.byref(i)) == 0
        return i

    def stats(self, k=2):
        return [(s.solved, s.inconsistent, s.niter, s.status) for s in self.st[:k]]

    def objgrad(self, q, x, rho, eta, xk=None):
        fx = C.c_double()
        gx, ys, gs = np.full(self.n, np.nan), np.full(self.m, np.nan), np.full(self.n, np.nan)
        rc = self.lib.fpsq_qp_objgrad(self.h, q, x.ctypes.data, SIGMA, rho, eta, None if xk is None else xk.ctypes.data,
                                      C.byref(fx), gx.ctypes.data, ys.ctypes.data, gs.ctypes.data, self.st)
        assert rc >= 0, self.err()
        return dict(fx=fx.value, rc=rc, gx=gx, ys=ys, gs=gs, st=self.stats(), launches=int(self.info().last_kernel_launches))

    def hprod(self, q, v, rho, eta, approx=2):
        hv = np.full(self.n, np.nan)
        rc = self.lib.fpsq_qp_hprod(self.h, q, v.ctypes.data, SIGMA, rho, eta, approx, hv.ctypes.data, self.st)
        assert rc >= 0, self.err()
        return dict(hv=hv, rc=rc, st=self.stats(), launches=int(self.info().last_kernel_launches))

    def close(self):
        i = self.info()
        for q in self.models:
            assert self.lib.fpsq_qp_destroy(q) == 0
        self.lib.fpsq_destroy(self.h)
        assert (i.fuse_fallbacks, i.wait_timeouts, i.p2p_timeouts) == (0, 0, 0)


def _close(dev):
    """closes a Device*EqQP after checking that no call was silently repeated and no bounded wait expired"""
    i = dev.info()
    dev.close()
    assert (i["fuse_fallbacks"], i["wait_timeouts"], i["p2p_timeouts"]) == (0, 0, 0)


def _same(a, b, keys=("fx", "rc", "gx", "ys", "gs", "st")):
    return all(np.array_equal(a[k], b[k]) for k in keys)


def test_half_widths_give_the_lane_groups_and_ragged_tiles_the_cases_rely_on():
    lanes = {hw: _lanes(_qp("n4000", hw)) for hw in (1, 2, 8)}
    assert lanes == {1: 1, 2: 2, 8: 8}
    assert _lanes(_qp("n6000", 1)) == 1 and _lanes(_qp("n6000", 8)) == 8
    # n that is no multiple of the rows of a tile, 256 / LG, and one that is
    assert 4000 % (256 // lanes[1]) != 0 and 4000 % (256 // lanes[8]) == 0
    assert 6000 % (256 // lanes[1]) != 0 and 6000 % (256 // lanes[8]) != 0 and 24000 % (256 // lanes[2]) != 0
    # rows of R without an entry, next to full ones
    rows = np.diff(_qp("n4000", 8).hess_rowptr) - 1
    assert np.any(rows == 0) and rows.max() > 8
    # more than one workgroup in every case
    assert 4000 // (256 // lanes[8]) > 1 and 4000 // 256 > 1


# ------------------------------------------------------------------------------------------------ 1. the exact reference

@pytest.mark.parametrize("ln_method", [0, 1], ids=["craig", "lnlq"])
@pytest.mark.parametrize("delta", [0.0, SE, 1e-2], ids=["delta0", "sqrt-eps", "1e-2"])
@pytest.mark.parametrize("hw", [1, 8])
@pytest.mark.parametrize("shape", ["n4000", "n6000"])
def test_objgrad_and_hprod_with_a_sparse_hessian_match_the_exact_reference(shape, hw, delta, ln_method):
    qp, ref = _qp(shape, hw), _ref(shape, hw, delta, ln_method)
    x = qp.x
    v = np.random.default_rng(0).standard_normal(qp.n)
    zeros = np.zeros(qp.n)
    for label, opts, bar, need_rc0 in (("tight", TIGHT, 1e-9, False), ("default", {}, 1e-5, True)):
        H = _H(qp, delta, ln_method=ln_method, **opts)
        q = H.csr()
        qd = H.diag()        # the diagonal part alone, on the same handle
        for rho, eta in ((0.0, 0.0), (1.0, 0.5)):
            for xk in (qp.xhat, None):
                how = "given" if xk is not None else "None"
                e = ref.objgrad(x, SIGMA, rho, eta, xk)
                if xk is None and eta > 0.0:
                    # the iterative entry wants xk whenever eta > 0 (include/fpsq.h): NULL is refused, the reference's xk = 0 is passed
                    fx = C.c_double()
                    assert H.lib.fpsq_qp_objgrad(H.h, q, x.ctypes.data, SIGMA, rho, eta, None, C.byref(fx), None, None, None,
                                                 H.st) == -1
                    xk = zeros
                o = H.objgrad(q, x, rho, eta, xk)
                errs = {k: _rel(o[k], e[k]) for k in ("gx", "ys", "gs")}
                errs["fx"] = abs(o["fx"] - e["fx"]) / abs(e["fx"])
                print(f"\n{shape} hw={hw} delta={delta:g} ln={ln_method} {label} rho={rho} eta={eta} "
                      f"xk={how}: {errs} rc={o['rc']} its={[s[2] for s in o['st']]}")
                assert not need_rc0 or o["rc"] == 0
                assert errs["gx"] < bar and errs["ys"] < bar and errs["gs"] < bar
                assert abs(o["fx"] - e["fx"]) <= bar * abs(e["fx"])
            h2, h1 = H.hprod(q, v, rho, eta, 2), H.hprod(q, v, rho, eta, 1)
            err = _rel(h2["hv"], ref.hprod(v, SIGMA, rho, eta))
            print(f"{shape} hw={hw} delta={delta:g} ln={ln_method} {label} rho={rho} eta={eta} hprod: {err:.3e} rc={h2['rc']}")
            assert not need_rc0 or (h2["rc"] == 0 and h1["rc"] == 0)
            assert err < bar
            assert np.array_equal(h1["hv"], h2["hv"])      # Val(1): its extra terms vanish for linear constraints
        # the Hessian matters: the diagonal part alone is far from the reference
        od = H.objgrad(qd, x, 1.0, 0.5, qp.xhat)
        assert _rel(od["gx"], ref.objgrad(x, SIGMA, 1.0, 0.5, qp.xhat)["gx"]) > 1e-3
        H.close()


# ------------------------------------------------------------------------------------------------ 2. the host mirror

@pytest.mark.parametrize("hw", [1, 8])
def test_device_model_matches_the_host_mirror_through_the_same_back_end(hw):
    """FletcherPenaltyNLP on the host model, its solves on the same HIP recurrences at the same (default) tolerances."""
    qp = _qp("n4000", hw)
    model = nlpmodels.EqQPModel(qp)
    v = np.random.default_rng(5).standard_normal(qp.n)
    for rho in (1.0, 0.0):
        qds = HIPQDSolver(model, 0.0)
        fp = FletcherPenaltyNLP(model, SIGMA, rho, SE, 2, qds=qds)
        f_host, g_host = fp.objgrad(qp.x)
        hv_host = fp.hprod(qp.x, v)
        dev = DeviceSparseHessianEqQP(qp, sigma=SIGMA, rho=rho, delta=SE)
        g_dev, hv_dev = np.empty(qp.n), np.empty(qp.n)
        f_dev, rc = dev.objgrad(qp.x, gx=g_dev)
        assert rc == 0 and dev.hprod(v, hv_dev) == 0
        errs = (_rel(g_dev, g_host), abs(f_dev - f_host) / abs(f_host), _rel(hv_dev, hv_host))
        print(f"\nhw={hw} rho={rho}: gx {errs[0]:.3e} phi {errs[1]:.3e} Hv {errs[2]:.3e}")
        assert errs[0] < 1e-8 and errs[1] <= 1e-8 and errs[2] < 1e-8
        _close(dev)
        qds.close()


# ------------------------------------------------------------------------------------------------ 3. stored zeros, several models

def test_stored_zeros_agree_with_the_diagonal_model_and_models_do_not_disturb_each_other():
    qp = _small()
    pattern = _qp("n4000", 2)
    Q = pattern.hess_csr().copy()
    Q.data[:] = 0.0                     # every off-diagonal entry STORED, with value 0.0 ...
    Q.setdiag(qp.qdiag)                 # ... and the diagonal model's diagonal
    zeros = dataclasses.replace(pattern, qdiag=qp.qdiag, hess_vals=Q.data.copy())
    assert zeros.hess_vals.size == pattern.hess_vals.size and np.count_nonzero(zeros.hess_vals) == qp.n
    x, xk = qp.point(1), qp.xhat
    v = np.random.default_rng(2).standard_normal(qp.n)
    H = _H(qp, SE)
    qd = H.diag()

    def both(q):
        H.objgrad(q, x, 1.0, 0.5, xk)   # (the call after which the expected iteration count is this evaluation's own)
        return H.objgrad(q, x, 1.0, 0.5, xk), H.hprod(q, v, 1.0, 0.5), H.hprod(q, v, 1.0, 0.5)

    first = both(qd)
    qz, qs = H.csr(zeros), H.csr(pattern)
    got = both(qz)
    # iteration counts and statuses are identical; each element differs at most by the order in which a few fp64 terms (exact
    # zeros among them) are added; f is summed over another partition of the rows
    assert got[0]["st"] == first[0]["st"] and got[0]["rc"] == first[0]["rc"] == 0
    assert got[2]["st"] == first[2]["st"] and got[2]["rc"] == first[2]["rc"] == 0
    assert abs(got[0]["fx"] - first[0]["fx"]) <= 1e-13 * abs(first[0]["fx"])
    for k in ("gx", "ys", "gs"):
        assert _rel(got[0][k], first[0][k]) <= 1e-14, (k, _rel(got[0][k], first[0][k]))
    assert _rel(got[2]["hv"], first[2]["hv"]) <= 1e-14
    # the same iterations, the same kernels around them: an objgrad is two launches longer, an hprod one
    assert got[0]["launches"] == first[0]["launches"] + 2, (got[0]["launches"], first[0]["launches"])
    assert got[2]["launches"] == first[2]["launches"] + 1, (got[2]["launches"], first[2]["launches"])
    sparse = both(qs)
    assert _rel(sparse[0]["gx"], first[0]["gx"]) > 1e-3          # (a different model)
    # the diagonal model after the sparse ones, and a diagonal model created after them: bitwise the first answer
    for q in (qd, H.diag()):
        after = both(q)
        assert _same(after[0], first[0]) and np.array_equal(after[2]["hv"], first[2]["hv"]) and after[2]["st"] == first[2]["st"]
    # ... and the sparse one is bitwise repeatable in between
    sparse2 = both(qs)
    assert _same(sparse2[0], sparse[0]) and np.array_equal(sparse2[2]["hv"], sparse[2]["hv"])
    H.close()


# ------------------------------------------------------------------------------------------------ 4. speculation

@pytest.mark.parametrize("delta", [0.0, SE])
def test_speculative_epilogue_every_alignment_is_bitwise_neutral_with_a_sparse_hessian(delta):
    """fpsq_debug_expect_iterations places the speculative (gated) epilogue -- with the gated gx -= R p2 / Hv -= R (v - p1)
    launches behind its tail -- at EVERY position relative to the true iteration counts of the two lanes; an epilogue whose gates
    stay closed is enqueued again behind the loop.  Every result is bitwise that of a handle that never speculates: the gating,
    and the out-of-place form of the subtraction."""
    qp = _qp("n4000", 2)
    ref, dev = _H(qp, delta), _H(qp, delta)
    qr, qv = ref.csr(), dev.csr()
    lib = dev.lib
    rng = np.random.default_rng(1)
    x = qp.xhat + 0.3 * rng.standard_normal(qp.n)
    v = rng.standard_normal(qp.n)

    def run(H, q, which):
        if which == "objgrad":
            o = H.objgrad(q, x, 1.0, 0.5, qp.xhat)
            return (np.array([o["fx"]]), o["gx"], o["ys"], o["gs"]), o["rc"], o["st"]
        o = H.hprod(q, v, 1.0, 0.5)
        return (o["hv"],), o["rc"], o["st"]

    for which in ("objgrad", "hprod"):
        assert lib.fpsq_debug_expect_iterations(ref.h, 0) == 0   # never speculates
        want, rc0, st0 = run(ref, qr, which)
        its = (st0[0][2], st0[1][2])
        assert min(its) >= 2, its
        for e in range(0, max(its) + 4):
            assert lib.fpsq_debug_expect_iterations(dev.h, e) == 0
            got, rc, st = run(dev, qv, which)
            assert rc == rc0 and st == st0, (which, e)
            for a_, b_ in zip(want, got):
                assert np.array_equal(a_, b_), (which, e, its)
    ref.close()
    dev.close()


# ------------------------------------------------------------------------------------------------ 5. the tail's variants

def _tail_run(monkeypatch, env, qp, delta, rho, x, xk, v):
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    H = _H(qp, delta, **TIGHT)
    q = H.csr()
    # (p2 = v of solve_two_mixed at this point, for the rounding bound of the FPSQ_CRAIG_X=1 comparison)
    g, c = qp.hess_csr() @ x + qp.d, qp.scipy_csr() @ x - qp.b
    p1, q1, p2, q2 = np.empty(qp.n), np.empty(qp.m), np.empty(qp.n), np.empty(qp.m)
    st = (_lib.Stats * 2)()
    assert H.lib.fpsq_solve_two_mixed(H.h, g.ctypes.data, c.ctypes.data, p1.ctypes.data, q1.ctypes.data, p2.ctypes.data,
                                      q2.ctypes.data, st) >= 0, H.err()
    out = dict(og=[H.objgrad(q, x, rho, 0.5, xk), H.objgrad(q, x, rho, 0.5, xk)],      # (the second: a speculative tail)
               hp=[H.hprod(q, v, rho, 0.5), H.hprod(q, v, rho, 0.5)], p2=p2, craig_iters=int(st[1].niter),
               at_sorted=int(H.info().at_sorted))
    H.close()
    for k in env:
        monkeypatch.delenv(k)
    return out


def test_every_tail_variant_carries_the_sparse_hessian(monkeypatch):
    """The gated gx -= R p2 stands behind whichever tail ran -- the one-launch tail, the raw product + k_qp_penalty_grad
    (FPSQ_FUSE_TAIL=0), the unpaired branch (rho = 0), CRAIG with x in its loop (FPSQ_CRAIG_X=1) -- and finds p2 in the same place.
    Bitwise between the tails where tests/test_gpu_parity.py and tests/test_gpu_craig_x_from_y.py establish that for the diagonal
    model; the FPSQ_CRAIG_X=1 recurrence within the rounding bound of the latter, extended by the R p2 term."""
    qp, delta = _qp("n24000", 2), SE
    ref = _ref("n24000", 2, delta)
    rng = np.random.default_rng(13)
    x, xk, v = qp.xhat + 0.5 * rng.standard_normal(qp.n), qp.xhat, rng.standard_normal(qp.n)
    base = _tail_run(monkeypatch, {}, qp, delta, 1.0, x, xk, v)
    assert base["at_sorted"] != 0               # (the one-launch tail with v formed inside it is what the default handle ran)
    two = _tail_run(monkeypatch, {"FPSQ_FUSE_TAIL": "0"}, qp, delta, 1.0, x, xk, v)
    rec = _tail_run(monkeypatch, {"FPSQ_CRAIG_X": "1"}, qp, delta, 1.0, x, xk, v)
    unp = _tail_run(monkeypatch, {}, qp, delta, 0.0, x, xk, v)
    # each within bar 1 of the exact reference
    for name, run, rho in (("default", base, 1.0), ("two-launch", two, 1.0), ("craig-x", rec, 1.0), ("rho0", unp, 0.0)):
        e, ehv = ref.objgrad(x, SIGMA, rho, 0.5, xk), ref.hprod(v, SIGMA, rho, 0.5)
        for o in run["og"]:
            errs = {k: _rel(o[k], e[k]) for k in ("gx", "ys", "gs")}
            errs["fx"] = abs(o["fx"] - e["fx"]) / abs(e["fx"])
            print(f"\n{name}: {errs}")
            assert all(err < 1e-9 for err in errs.values()), (name, errs)
        for o in run["hp"]:
            assert _rel(o["hv"], ehv) < 1e-9, name
        assert _same(run["og"][0], run["og"][1]) and np.array_equal(run["hp"][0]["hv"], run["hp"][1]["hv"])
    # the two-launch tail: everything bitwise, one launch more per enqueued tail
    for k in range(2):
        assert _same(two["og"][k], base["og"][k]), k
        assert np.array_equal(two["hp"][k]["hv"], base["hp"][k]["hv"]) and two["hp"][k]["st"] == base["hp"][k]["st"]
    assert two["og"][1]["launches"] == base["og"][1]["launches"] + 1
    # CRAIG with x in its loop: what does not depend on p2 is bitwise, the rest within rounding
    iters = rec["craig_iters"]
    longest = int(np.max(np.diff(sp.csc_matrix(qp.scipy_csr()).indptr)))
    R = qp.hess_csr() - sp.diags(qp.hess_csr().diagonal())
    rnorm = float(abs(R).sum(axis=1).max())              # ||R||_2 <= ||R||_inf (symmetric)
    rrow = int(np.diff(R.tocsr().indptr).max())
    nv = float(np.linalg.norm(rec["p2"]))
    bound_v = 8 * EPS * (iters + longest) * nv           # tests/test_gpu_craig_x_from_y.py, (ii)
    dv = float(np.linalg.norm(base["p2"] - rec["p2"]))
    print(f"\nCRAIG iterations {iters}, longest row of A' {longest}, ||dv|| = {dv:.3e}, bound {bound_v:.3e}")
    assert dv <= bound_v and not np.array_equal(base["p2"], rec["p2"])
    q2s, qmax = float(np.max(np.abs(2 * SIGMA - qp.qdiag))), float(np.max(qp.qdiag))
    for k in range(2):
        a_, b_ = base["og"][k], rec["og"][k]
        for key in ("rc", "st", "ys", "fx"):
            assert np.array_equal(a_[key], b_[key]), key
        ngs, ngx = float(np.linalg.norm(b_["gs"])), float(np.linalg.norm(b_["gx"]))
        bound_gs = SIGMA * bound_v + 4 * EPS * (ngs + SIGMA * nv)
        # gx = (the tail's gx) - R p2: dv times (max|2 sigma - q| + ||R||), the tail's own roundings, and those of the row sums of
        # R p2 (rrow products and additions) and of the subtraction
        bound_gx = (q2s + rnorm) * bound_v + 4 * EPS * (ngs + ngx + (SIGMA + qmax) * nv) + (rrow + 2) * EPS * (rnorm * nv + ngx)
        dgs, dgx = float(np.linalg.norm(a_["gs"] - b_["gs"])), float(np.linalg.norm(a_["gx"] - b_["gx"]))
        print(f"  objgrad[{k}]: ||dgs|| = {dgs:.3e} (bound {bound_gs:.3e}), ||dgx|| = {dgx:.3e} (bound {bound_gx:.3e})")
        assert dgs <= bound_gs and dgx <= bound_gx
    # (hprod runs two LSQR lanes: no CRAIG lane, nothing of FPSQ_CRAIG_X in it)
    for k in range(2):
        assert np.array_equal(rec["hp"][k]["hv"], base["hp"][k]["hv"])


# ------------------------------------------------------------------------------------------------ 6. arguments

def _dev_objgrad(dev, x, xk, on=None, want=("gx", "ys", "gs")):
    """one evaluation; `on`: a torch device to run it on device tensors, None: numpy arrays; outputs not in `want` are null"""
    qp = dev.qp
    size = {"gx": qp.n, "ys": qp.m, "gs": qp.n}
    if on is None:
        out = {k: np.full(size[k], np.nan) for k in want}
        fx, rc = dev.objgrad(x, xk=xk, **out)
        return fx, rc, out
    import torch

    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(on)  # noqa: E731
    out = {k: torch.full((size[k],), float("nan"), dtype=torch.float64, device=on) for k in want}
    fx, rc = dev.objgrad(t(x), xk=t(xk), **out)   # (every vector on the GPU: the stream-ordered return)
    torch.cuda.current_stream().synchronize()
    return fx, rc, {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("hw", [1, 8])
def test_host_and_device_arguments_repeats_and_null_outputs_are_bitwise_the_same(hw):
    import torch

    qp = _qp("n6000", hw)
    x, xk = qp.point(2), qp.xhat
    on = torch.device("cuda", 0)
    dev = DeviceSparseHessianEqQP(qp, sigma=SIGMA, rho=1.0, delta=SE, eta=0.5)
    host = _dev_objgrad(dev, x, xk)
    again = _dev_objgrad(dev, x, xk)
    devt = _dev_objgrad(dev, x, xk, on=on)
    devt2 = _dev_objgrad(dev, x, xk, on=on)
    for other in (again, devt, devt2):
        assert other[0] == host[0] and other[1] == host[1] == 0
        for k in ("gx", "ys", "gs"):
            assert np.array_equal(other[2][k], host[2][k]), k
    # every subset of the output vectors, host- and device-resident: the others (and phi) do not change a bit
    for want in ((), ("gx",), ("ys",), ("gs",), ("gx", "ys"), ("gx", "gs"), ("ys", "gs")):
        for where in (None, on):
            fx, rc, o = _dev_objgrad(dev, x, xk, on=where, want=want)
            assert fx == host[0] and rc == 0
            for k in want:
                assert np.array_equal(o[k], host[2][k]), (want, k)
    v = np.random.default_rng(1).standard_normal(qp.n)
    Hh, Hh2, Hd = np.empty(qp.n), np.empty(qp.n), torch.empty(qp.n, dtype=torch.float64, device=on)
    assert dev.hprod(v, Hh) == 0 and dev.hprod(v, Hh2) == 0 and dev.hprod(torch.from_numpy(v).to(on), Hd) == 0
    assert np.array_equal(Hh, Hh2) and np.array_equal(Hh, Hd.cpu().numpy())
    e = _ref("n6000", hw, SE).objgrad(x, SIGMA, 1.0, 0.5, xk)
    assert _rel(host[2]["gx"], e["gx"]) < 1e-5 and abs(host[0] - e["fx"]) <= 1e-5 * abs(e["fx"])
    _close(dev)


# ------------------------------------------------------------------------------------------------ 7. refusals

def test_create_csr_refuses_an_unsymmetric_duplicate_or_out_of_range_hessian():
    qp = _qp("n4000", 2)
    H = _H(qp, 0.0, **TIGHT)
    q0 = H.csr()
    x = qp.x
    before = H.objgrad(q0, x, 1.0, 0.0)
    rp, ci, va = qp.hess_rowptr, qp.hess_colind, qp.hess_vals
    k = int(rp[7])                                    # row 7, first entry: column 5 (rows 5 .. 9 have every neighbour)
    assert ci[k] == 5 and rp[8] - rp[7] == 5
    bad_val = va.copy()
    bad_val[k] += 1e-9                                # Q[7, 5] != Q[5, 7]
    bad_pat = ci.copy()
    bad_pat[k] = 4                                    # (7, 4) has no transpose: half_width 2
    dup = ci.copy()
    dup[k] = ci[k + 1]                                # column 6 twice in row 7
    oob, neg = ci.copy(), ci.copy()
    oob[k], neg[k] = qp.n, -1
    for what, args in (("values", (rp, ci, bad_val)), ("pattern", (rp, bad_pat, va)), ("duplicate", (rp, dup, va)),
                       ("range", (rp, oob, va)), ("range", (rp, neg, va))):
        rc, msg, q = H.try_csr(*args)
        print(what, "->", rc, msg)
        assert rc == -1 and not q.value and msg.startswith("qp_create_csr:") and what in msg, (what, rc, msg)
    # unsorted columns are fine, and stored sorted: the same bits
    flip = ci.copy(), va.copy()
    for a in flip:
        a[k:k + 5] = a[k:k + 5][::-1].copy()
    rc, msg, q = H.try_csr(rp, *flip)
    assert rc == 0 and q.value, msg
    H.models.append(q)
    assert _same(H.objgrad(q, x, 1.0, 0.0), before)
    # an absent diagonal is zero, and that model meets the bar of the exact reference
    Q = qp.hess_csr().tolil()
    Q.setdiag(0.0)
    Q = Q.tocsr()
    Q.eliminate_zeros()
    nodiag = dataclasses.replace(qp, qdiag=np.zeros(qp.n), hess_rowptr=Q.indptr.astype(np.int32),
                                 hess_colind=Q.indices.astype(np.int32), hess_vals=Q.data.copy())
    assert nodiag.hess_vals.size == qp.hess_vals.size - qp.n
    o = H.objgrad(H.csr(nodiag), x, 1.0, 0.0)
    e = SparseHessianRef(nodiag, 0.0).objgrad(x, SIGMA, 1.0)
    assert _rel(o["gx"], e["gx"]) < 1e-9 and _rel(o["ys"], e["ys"]) < 1e-9 and _rel(o["gs"], e["gs"]) < 1e-9
    assert abs(o["fx"] - e["fx"]) <= 1e-9 * abs(e["fx"])
    # the handle and its first model stay usable
    assert _same(H.objgrad(q0, x, 1.0, 0.0), before)
    H.close()


def test_a_handle_with_a_communicator_refuses_the_sparse_hessian():
    qp = _qp("n4000", 2)
    group = LocalGroup(1)
    H = _H(qp, 0.0)
    assert H.lib.fpsq_comm_init_local(H.h, group.ptr, 0) == 0, H.err()
    rc, msg, q = H.try_csr(qp.hess_rowptr, qp.hess_colind, qp.hess_vals)
    assert rc == -3 and not q.value and msg.startswith("qp_create_csr:") and "communicator" in msg, (rc, msg)
    H.close()
    with pytest.raises(ValueError, match="single-GPU"):
        DeviceSparseHessianEqQP(qp, comm=("local", group.ptr, 0))
    with pytest.raises(ValueError, match="single-GPU"):
        DeviceSparseHessianEqQP(qp, halo=(0, 0))
    group.close()
    # MINRES on K is out of scope too
    H = _H(qp, 0.0, kkt_method=1)
    rc, msg, q = H.try_csr(qp.hess_rowptr, qp.hess_colind, qp.hess_vals)
    assert rc == -3 and not q.value and "MINRES" in msg, (rc, msg)
    H.close()


def test_the_class_takes_a_diagonal_qp_and_the_base_class_keeps_its_guard():
    qp = _small()
    a, b = DeviceSparseHessianEqQP(qp, delta=SE), DeviceEqQP(qp, delta=SE)
    ga, gb = np.empty(qp.n), np.empty(qp.n)
    assert a.objgrad(qp.x, gx=ga) == b.objgrad(qp.x, gx=gb) and np.array_equal(ga, gb)
    _close(a)
    _close(b)
    with pytest.raises(ValueError, match="DeviceBandEqQP"):
        DeviceEqQP(_qp("n4000", 1))


# ------------------------------------------------------------------------------------------------ 8. the outer loop

@pytest.mark.parametrize("sub", ["trunk", "lbfgs"])
def test_fps_solve_device_with_a_sparse_hessian_on_the_iterative_back_end(sub):
    """The device-resident outer loop at the default tolerances, to the bounds
    tests/test_gpu_band_qp_sparse_hessian.py::test_fps_solve_device_with_a_sparse_hessian holds the banded back-end to."""
    import torch

    from fps_amd.fps_solve import fps_solve_device

    qp = _qp("n4000", 2)
    xstar, lam = _ref("n4000", 2, 0.0).kkt_point()
    dev = DeviceSparseHessianEqQP(qp)
    x0 = torch.from_numpy(qp.x).to(torch.device("cuda", 0))
    stats = fps_solve_device(dev, x0, subproblem_solver=sub, max_time=120)
    x, y = stats.solution.cpu().numpy(), stats.multipliers.cpu().numpy()
    print(f"\n{sub}: {stats.status}, |x - x*|/|x*| = {np.linalg.norm(x - xstar) / np.linalg.norm(xstar):.2e}, "
          f"|y - y*| = {np.linalg.norm(y - lam):.2e} (|y*| = {np.linalg.norm(lam):.2e})")
    assert stats.status == "first_order", (stats.status, stats.solver_specific)
    assert np.linalg.norm(x - xstar) <= 1e-6 * np.linalg.norm(xstar)
    assert np.linalg.norm(y - lam) <= 1e-5 * max(1.0, np.linalg.norm(lam))
    _close(dev)
