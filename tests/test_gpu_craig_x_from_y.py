"""On one GPU the CRAIG lane carries no x through its loop: p2 = v = -A'q2 is formed once behind it, from the final y
(csrc/fpsq.hip two_mixed_device; tests/test_craig_x_is_at_y.py pins the identity x_k = A'y_k on the CPU restatement).
FPSQ_CRAIG_X=1 keeps the recurrence xs += e0 v~ -- the handle these tests compare with.

 (i)   what does not depend on x -- return codes, iteration counts, statistics, q1, q2, ys, phi (and p1) -- is BITWISE the
       recurrence handle's;
 (ii)  v / p2, gs and grad(phi) agree with it within a rounding-error bound computed per case, not a tuned tolerance.  Both v
       are sums of the same terms in another order (the recurrence adds `iterations` multiples of Golub-Kahan vectors, the
       product sums a row of A'), so norm-wise  ||dv|| <= K eps (iterations + longest row of A') ||v||  with K = 8: the CPU
       restatement gives ||x - A'y|| <= 8.8e-16 ||x|| at <= 83 iterations and rows of <= 100 entries, K = 8 leaves an order
       of magnitude.  gs = fma(sigma, v, p1) and gx = fma(sigma, v, fma(-q, v, gs)) (+ terms without v) take dv times
       sigma resp. max|2 sigma - q| and add their own roundings, at most 4 eps (||gs|| + ||gx|| + (sigma + max|q|) ||v||);
 (iii) v is bitwise the same from fpsq_solve_two_mixed and fpsq_ys_gs, with one launch per iteration and with two
       (FPSQ_FUSE_ITER), and gs / grad(phi) of fpsq_qp_objgrad -- the only places its v shows -- bitwise the same with the
       one-launch and the two-launch tail (FPSQ_FUSE_TAIL), FPSQ_FUSE_ITER 0 / 2, and with v summed inside the tail's launch
       or by the stand-alone single-lane product the other two entry points use (FPSQ_CRAIG_X=2: one launch more);
 (iv)  no bounded wait expired, no call was repeated.

Largest ratios observed on the MI355X over the 21 cases (7 structures x 3 delta): ||dv|| / bound = 0.011 (wide-window,
delta = sqrt(eps): ||dv|| = 3.3e-14 against 3.0e-12), and no more than 0.011 for gs and grad(phi) against their bounds either;
the rank-deficient and the itmax cases included."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import fps_amd  # noqa: F401
from fps_amd import _lib, problems
from structures import random_structure

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
SE = np.sqrt(EPS)
K = 8
SIGMA = 1e3


class _Model:
    """An equality-constrained QP on a given Jacobian through the raw C ABI: the three entry points that hand out v or use it."""

    def __init__(self, A, qdiag, d, b, delta, **opts):
        self.lib = lib = _lib.load()
        A = sp.csr_matrix(A)
        self.m, self.n = A.shape
        o = _lib.Options()
        lib.fpsq_default_options(self.n, self.m, C.byref(o))
        for k, v in opts.items():
            setattr(o, k, v)
        self.h = C.c_void_p()
        assert lib.fpsq_create(C.byref(self.h), self.n, self.m, C.byref(o)) == 0, lib.fpsq_last_error(None)
        rp, ci = A.indptr.astype(np.int32), A.indices.astype(np.int32)
        assert lib.fpsq_set_jacobian_structure_csr(self.h, rp.ctypes.data, ci.ctypes.data) == 0, self.err()
        vals = np.ascontiguousarray(A.data, dtype=np.float64)
        assert lib.fpsq_set_jacobian_values(self.h, vals.ctypes.data) == 0, self.err()
        assert lib.fpsq_set_delta(self.h, float(delta)) == 0
        self.q = C.c_void_p()
        self.keep = [np.ascontiguousarray(a, dtype=np.float64) for a in (qdiag, d, b)]
        assert lib.fpsq_qp_create(self.h, *[a.ctypes.data for a in self.keep], C.byref(self.q)) == 0, self.err()
        self.st = (_lib.Stats * 2)()

    def err(self):
        return self.lib.fpsq_last_error(self.h)

    def stats(self):
        return np.array([[s.solved, s.inconsistent, s.niter, s.status, s.rnorm, s.arnorm] for s in self.st]).ravel()

    def mixed(self, g, c):
        out = [np.full(k, np.nan) for k in (self.n, self.m, self.n, self.m)]
        rc = self.lib.fpsq_solve_two_mixed(self.h, g.ctypes.data, c.ctypes.data, *[o.ctypes.data for o in out], self.st)
        assert rc >= 0, self.err()
        return dict(rc=rc, st=self.stats(), p1=out[0], q1=out[1], v=out[2], q2=out[3])

    def ys_gs(self, g, c):
        out = [np.full(k, np.nan) for k in (self.n, self.m, self.n, self.m)]
        rc = self.lib.fpsq_ys_gs(self.h, g.ctypes.data, c.ctypes.data, SIGMA, *[o.ctypes.data for o in out], self.st)
        assert rc >= 0, self.err()
        return dict(rc=rc, st=self.stats(), gs=out[0], ys=out[1], v=out[2], q2=out[3])

    def objgrad(self, x):
        fx = C.c_double()
        gx, ys, gs = np.full(self.n, np.nan), np.full(self.m, np.nan), np.full(self.n, np.nan)
        rc = self.lib.fpsq_qp_objgrad(self.h, self.q, x.ctypes.data, SIGMA, 1.0, 0.0, None, C.byref(fx), gx.ctypes.data,
                                      ys.ctypes.data, gs.ctypes.data, self.st)
        assert rc >= 0, self.err()
        i = _lib.Info()
        assert self.lib.fpsq_get_info(self.h, C.byref(i)) == 0
        return dict(rc=rc, st=self.stats(), fx=np.array([fx.value]), gx=gx, ys=ys, gs=gs, launches=int(i.last_kernel_launches),
                    at_sorted=int(i.at_sorted))

    def counters(self):
        i = _lib.Info()
        assert self.lib.fpsq_get_info(self.h, C.byref(i)) == 0
        return (i.fuse_fallbacks, i.wait_timeouts, i.p2p_timeouts)

    def close(self):
        self.lib.fpsq_qp_destroy(self.q)
        self.lib.fpsq_destroy(self.h)


def _case(name):
    """(A, options, zero_c): the small structures of the parity tests."""
    rng = np.random.default_rng(29)
    opts, zero_c = {}, False
    if name in ("pde", "pde-plain-csr", "pde-zero-c", "pde-itmax"):
        qp = problems.pde_control_like(n=4000, m=400, per_row=20, window=512, seed=7)
        A = qp.scipy_csr()
        if name == "pde-plain-csr":
            opts["jac_format"] = 1
        if name == "pde-itmax":  # both recurrences stop at the limit, unsolved (a soft return code)
            opts["ls_itmax"] = opts["ln_itmax"] = 5
        zero_c = name == "pde-zero-c"
    elif name == "pde-fused":  # large enough for one launch per iteration and the column-sorted A' layout of the one-launch tail
        A = problems.pde_control_like(n=60000, m=6000, per_row=20, window=512, seed=23).scipy_csr()
    elif name == "wide-window":
        A = random_structure("wide-window", rng)
    elif name == "rank-deficient":  # two identical constraint rows (test_rank_deficient_jacobian_is_handled_softly)
        A = problems.pde_control_like(n=600, m=40, per_row=20, window=512, seed=41).scipy_csr().tolil()
        A[7, :] = A[3, :]
    else:
        raise ValueError(name)
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A, opts, zero_c


CASES = ["pde", "pde-plain-csr", "pde-zero-c", "pde-itmax", "pde-fused", "wide-window", "rank-deficient"]


def _run(monkeypatch, env, A, opts, zero_c, delta):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m, n = A.shape
    rng = np.random.default_rng(31)
    qdiag, d = 1.0 + rng.random(n), rng.standard_normal(n)
    x = np.zeros(n) if zero_c else rng.standard_normal(n)
    b = np.zeros(m) if zero_c else rng.standard_normal(m)
    if A.shape == (40, 600):
        b[7] = b[3]  # (a consistent right-hand side: rows 3 and 7 are the same)
    g, c = qdiag * x + d, A @ x - b
    M = _Model(A, qdiag, d, b, delta, **opts)
    res = dict(mixed=M.mixed(g, c), ys_gs=M.ys_gs(g, c), objgrad=[M.objgrad(x), M.objgrad(x)])  # (the second: a speculative tail)
    res["counters"] = M.counters()
    M.close()
    for k in env:
        monkeypatch.delenv(k)
    return res, float(np.max(np.abs(2 * SIGMA - qdiag))), float(np.max(qdiag))


@pytest.mark.parametrize("delta", [0.0, SE, 0.25])
@pytest.mark.parametrize("name", CASES)
def test_v_from_the_product_against_the_recurrence(monkeypatch, name, delta):
    A, opts, zero_c = _case(name)
    new, q2s, qmax = _run(monkeypatch, {}, A, opts, zero_c, delta)
    old, _, _ = _run(monkeypatch, {"FPSQ_CRAIG_X": "1"}, A, opts, zero_c, delta)
    assert new["counters"] == old["counters"] == (0, 0, 0)                                   # (iv)
    # (i) bitwise: nothing of this depends on x
    for key in ("rc", "st", "p1", "q1", "q2"):
        assert np.array_equal(new["mixed"][key], old["mixed"][key]), key
    for key in ("rc", "st", "ys", "q2"):
        assert np.array_equal(new["ys_gs"][key], old["ys_gs"][key]), key
    for a_, b_ in zip(new["objgrad"], old["objgrad"]):
        for key in ("rc", "st", "ys", "fx"):
            assert np.array_equal(a_[key], b_[key]), key
    # (ii) v, gs, grad(phi): the rounding-error bound
    iters = int(new["mixed"]["st"][6 + 2])
    longest = int(np.max(np.diff(sp.csc_matrix(A).indptr)))
    v_new, v_old = new["mixed"]["v"], old["mixed"]["v"]
    assert np.all(np.isfinite(v_new))
    nv = np.linalg.norm(v_old)
    bound_v = K * EPS * (iters + longest) * nv
    dv = np.linalg.norm(v_new - v_old)
    print(f"\n{name} delta={delta:g}: CRAIG iterations {iters}, longest row of A' {longest}, ||dv|| = {dv:.3e}, bound {bound_v:.3e}, "
          f"ratio {dv / bound_v if bound_v > 0 else 0.0:.3f}")
    ratios = []
    for what, a_, b_ in [("ys_gs gs", new["ys_gs"]["gs"], old["ys_gs"]["gs"])] + \
                        [(f"objgrad[{k}] gs", new["objgrad"][k]["gs"], old["objgrad"][k]["gs"]) for k in range(2)]:
        bound = SIGMA * bound_v + 4 * EPS * (np.linalg.norm(b_) + SIGMA * nv)
        dd = np.linalg.norm(a_ - b_)
        ratios.append((what, dd, bound))
    for k in range(2):
        a_, b_ = new["objgrad"][k], old["objgrad"][k]
        bound = q2s * bound_v + 4 * EPS * (np.linalg.norm(b_["gs"]) + np.linalg.norm(b_["gx"]) + (SIGMA + qmax) * nv)
        ratios.append((f"objgrad[{k}] gx", np.linalg.norm(a_["gx"] - b_["gx"]), bound))
    for what, dd, bound in ratios:
        print(f"  {what}: ||d|| = {dd:.3e}, bound {bound:.3e}, ratio {dd / bound if bound > 0 else 0.0:.3f}")
    assert dv <= bound_v
    for what, dd, bound in ratios:
        assert dd <= bound, what
    # the new path is the one that ran: another order of summation leaves other bits (the degenerate cases aside: v = 0 when c = 0)
    if not zero_c:
        assert not np.array_equal(v_new, v_old)
        assert not np.array_equal(new["objgrad"][1]["gs"], old["objgrad"][1]["gs"])


@pytest.mark.parametrize("delta", [0.0, SE, 0.25])
@pytest.mark.parametrize("name", CASES)
def test_v_is_bitwise_the_same_from_every_entry_point_and_variant(monkeypatch, name, delta):
    A, opts, zero_c = _case(name)
    runs = {}
    for fi in ("0", "2"):
        for ft in ("0", "1"):
            # FPSQ_CRAIG_X=2: v ALWAYS by the stand-alone single-lane product k_spmv<1, ..> (what fpsq_solve_two_mixed / fpsq_ys_gs
            # use), never by the pass inside the tail's launch: the independent kernel the in-launch v is compared with -- through
            # gs = fma(sigma, v, p1) and grad(phi) of fpsq_qp_objgrad, whose other operands are the same bits in both runs
            for cx in ("0", "2"):
                # (FPSQ_AT_ROW_ALIGN=8: the two-launch handle gets the one-launch handle's A' block partition -- the norm partials
                # of the loop are per block, so q2 itself is only bitwise the same on the same partition)
                env = {"FPSQ_FUSE_ITER": fi, "FPSQ_FUSE_TAIL": ft, "FPSQ_AT_ROW_ALIGN": "8", "FPSQ_CRAIG_X": cx}
                runs[fi, ft, cx], _, _ = _run(monkeypatch, env, A, opts, zero_c, delta)
                assert runs[fi, ft, cx]["counters"] == (0, 0, 0)
            # ... and the two really are different launches: where the tail can form v itself (column-sorted A' blocks), the
            # stand-alone product is one launch more (second call: the expected iteration count is known, nothing depends on timing)
            a_, b_ = runs[fi, ft, "0"]["objgrad"][1], runs[fi, ft, "2"]["objgrad"][1]
            if name != "pde-itmax":
                assert b_["launches"] == a_["launches"] + (1 if a_["at_sorted"] else 0), (fi, ft, a_["launches"], b_["launches"])
    assert name != "pde-fused" or all(r["objgrad"][1]["at_sorted"] for r in runs.values())  # (the in-launch v is under test at all)
    ref = runs["0", "0", "2"]
    assert np.array_equal(ref["mixed"]["v"], ref["ys_gs"]["v"])
    for key, r in runs.items():
        assert np.array_equal(r["mixed"]["v"], ref["mixed"]["v"]), key
        assert np.array_equal(r["ys_gs"]["v"], ref["mixed"]["v"]), key
        for k in range(2):
            for out in ("gs", "gx", "ys", "fx", "st"):
                assert np.array_equal(r["objgrad"][k][out], ref["objgrad"][k][out]), (key, k, out)
